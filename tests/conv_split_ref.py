"""CPU model of nn.conv1d(..., precision="split_bf16") (not a test module): the layer's four results in split arithmetic with an
EXACT (float64) accumulator, built on tests/split_bf16_model.py's ``split`` and three-term product.  Yardstick of
tests/test_conv_split_ref_cpu.py and tests/test_gpu_conv1d_split_bf16.py.

  forward          sm.conv1d_ref: the leaky ReLU in fp32 as the kernel applies it on load, then the three products of
                   split(lrelu(x)) against split(w), + bias;
  data gradient    the same conv on split(gy) and the split transposed, tap-flipped weights (no activation, no bias), times the
                   leaky ReLU's derivative (torch's rule at x = 0: the slope);
  weight gradient  the three-term correlation of split(gy) with split(lrelu(x));
  bias gradient    plain: the sum of gy.

``sp`` is a parameter, as in split_bf16_model: the identity (the model is then float64 autograd on the fp32 activation), hi-only
and two-terms (the controls a dropped term cannot pass).  Every utterance is evaluated alone on its valid columns: zeros beyond
a length are the "same" padding.  ``mask`` replaces the leaky ReLU's own branch decision (True: identity), as
tests/conv_grad_ref.py's resblock chain takes it."""
import torch
import torch.nn.functional as F

import split_bf16_model as sm


def lrelu32(x, slope, mask=None):
    """the activation as the kernels apply it on load: in fp32"""
    x = x.float()
    if slope == 1.0:
        return x
    return torch.where(x > 0 if mask is None else mask, x, x * slope)


def _conv(a, w, k, d, sp):
    """three-term "same" conv of the fp32 activation a [1, Cin, n] with w [Cout, Cin, k] -> float64"""
    return sm._three(lambda u, v: F.conv1d(u, v, None, padding=(k - 1) * d // 2, dilation=d), a, w, sp)


def _corr(gy, a, k, d, sp):
    """three-term correlation gw[co][ci][j] = sum_t gy[co][t] a[ci][t + j d - pad] of gy [1, Cout, n] with a [1, Cin, n]"""
    pad, n = (k - 1) * d // 2, a.shape[2]

    def op(g, v):
        vp = F.pad(v, (pad, pad))
        return torch.stack([g[0] @ vp[0, :, j * d:j * d + n].T for j in range(k)], dim=2)

    return sm._three(op, gy, a, sp)


def utterance(x, w, b, gy, d, slope, sp=sm.split, mask=None):
    """one utterance's valid columns x [1, Cin, n], gy [1, Cout, n] (fp32) -> float64 (y, gx, gw, gb)"""
    k = w.shape[2]
    a = lrelu32(x, slope, mask)
    y = _conv(a, w, k, d, sp)
    if b is not None:
        y = y + b.double()[None, :, None]
    wt = w.transpose(0, 1).flip(2).contiguous()
    deriv = torch.ones_like(x, dtype=torch.float64) if slope == 1.0 else \
        torch.where(x > 0 if mask is None else mask, 1.0, float(torch.tensor(slope, dtype=torch.float32))).double()
    gx = _conv(gy.float(), wt, k, d, sp) * deriv
    gw = _corr(gy.float(), a, k, d, sp)
    return y, gx, gw, gy.double().sum(dim=(0, 2))


def layer(x, w, b, gy, lengths, d, slope, sp=sm.split):
    """the ragged batch x [B, Cin, ld], gy [B, Cout, ld], lengths (None = ld) -> float64 (y, gx, gw, gb), y and gx zero beyond
    the lengths, gw and gb summed over the utterances; what lies beyond a length (NaN in the GPU tests) is never touched"""
    B, cin, ld = x.shape
    cout, _, k = w.shape
    y = torch.zeros(B, cout, ld, dtype=torch.float64)
    gx = torch.zeros(B, cin, ld, dtype=torch.float64)
    gw = torch.zeros(cout, cin, k, dtype=torch.float64)
    gb = torch.zeros(cout, dtype=torch.float64)
    for i in range(B):
        n = ld if lengths is None else int(lengths[i])
        if n <= 0:
            continue
        yi, gxi, gwi, gbi = utterance(x[i:i + 1, :, :n], w, b, gy[i:i + 1, :, :n], d, slope, sp)
        y[i, :, :n], gx[i, :, :n] = yi[0], gxi[0]
        gw += gwi
        gb += gbi
    return y, gx, gw, gb


def autograd64(x, w, b, gy, lengths, d, slope):
    """float64 torch autograd on the fp32 activation: what ``layer`` must reduce to under sm.split_identity"""
    B, cin, ld = x.shape
    k = w.shape[2]
    w64 = w.double().requires_grad_(True)
    b64 = None if b is None else b.double().requires_grad_(True)
    y, gx = torch.zeros(B, w.shape[0], ld, dtype=torch.float64), torch.zeros(B, cin, ld, dtype=torch.float64)
    loss = 0
    acts = []
    for i in range(B):
        n = ld if lengths is None else int(lengths[i])
        if n <= 0:
            acts.append(None)
            continue
        a = lrelu32(x[i:i + 1, :, :n], slope).double().requires_grad_(True)
        acts.append(a)
        yi = F.conv1d(a, w64, b64, padding=(k - 1) * d // 2, dilation=d)
        y[i, :, :n] = yi[0].detach()
        loss = loss + (yi * gy[i:i + 1, :, :n].double()).sum()
    loss.backward()
    s32 = float(torch.tensor(slope, dtype=torch.float32))
    for i, a in enumerate(acts):
        if a is not None:
            n = a.shape[2]
            gx[i, :, :n] = a.grad[0] * (1.0 if slope == 1.0 else torch.where(x[i, :, :n] > 0, 1.0, s32).double())
    return y, gx, w64.grad, None if b64 is None else b64.grad


def resblock1(x, w, k, dilations, gy, lengths, masks, sp=sm.split, slope=0.1):
    """nn.resblock1(..., precision="split_bf16") as the device chains it: every conv through ``utterance`` with its results
    rounded to fp32 (what the layers store), the residual added in fp32; the backward layer by layer in reverse, cotangents in
    fp32, the residual's cotangent added in fp32 as autograd does.  w: {"convs1.<m>.weight" / ".bias", "convs2.<m>..."} fp32;
    masks: the six conv inputs' branch decisions [B, C, ld] in call order.  -> (y [B, C, ld] fp32, gx fp32, {name: float64
    gradient})"""
    B, C, ld = x.shape
    y, gx = torch.zeros(B, C, ld), torch.zeros(B, C, ld)
    grads = {n: torch.zeros(t.shape, dtype=torch.float64) for n, t in w.items()}
    for i in range(B):
        n = int(lengths[i])
        if n <= 0:
            continue
        mk = lambda j: masks[j][i:i + 1, :, :n].cpu()
        zero = torch.zeros(1, C, n)
        h, ins = x[i:i + 1, :, :n].float(), []
        for m, d in enumerate(dilations):
            t = utterance(h, w[f"convs1.{m}.weight"], w[f"convs1.{m}.bias"], zero, d, slope, sp, mk(2 * m))[0].float()
            ins.append((h, t))
            h = (utterance(t, w[f"convs2.{m}.weight"], w[f"convs2.{m}.bias"], zero, 1, slope, sp, mk(2 * m + 1))[0].float() + h)
        y[i, :, :n] = h[0]
        g = gy[i:i + 1, :, :n].float()
        for m in reversed(range(len(dilations))):
            hm, t = ins[m]
            _, gt, gw2, gb2 = utterance(t, w[f"convs2.{m}.weight"], None, g, 1, slope, sp, mk(2 * m + 1))
            _, gh, gw1, gb1 = utterance(hm, w[f"convs1.{m}.weight"], None, gt.float(), dilations[m], slope, sp, mk(2 * m))
            for name, v in ((f"convs2.{m}.weight", gw2), (f"convs2.{m}.bias", gb2), (f"convs1.{m}.weight", gw1), (f"convs1.{m}.bias", gb1)):
                grads[name] += v
            g = g + gh.float()
        gx[i, :, :n] = g[0]
    return y, gx, grads


def rel_rms(a, ref):
    """rms(a - ref) / rms(ref), float64"""
    ref = ref.double()
    return float((a.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-300))


def row_rms(a, ref, dim):
    """per channel (dim = 1 of [B, C, L]) or weight row (dim = 0 of [Cout, Cin, k]): rms(a - ref) / rms(ref) of each -> [C]"""
    dims = tuple(i for i in range(ref.dim()) if i != dim)
    ref = ref.double()
    return (a.double() - ref).pow(2).mean(dim=dims).sqrt() / ref.pow(2).mean(dim=dims).sqrt().clamp_min(1e-300)


ROW_DIM = {"y": 1, "gx": 1, "gw": 0}


def bars(name, got, model, r64, r32, k_whole=sm.KERNEL_RATIO, k_row=sm.KERNEL_RATIO):
    """one tensor of a split launch against the model: (violations, figures).  Whole tensor and every channel / weight row:
    rms(got - model) / rms(model) <= K x max(torch fp32's own rms error against float64 on the same operands, sm.FLOOR); K =
    sm.KERNEL_RATIO (sm.launch_bar) unless the caller holds an exception by tests/train_stage_cases.py's rule."""
    e, e32 = rel_rms(got, model), rel_rms(r32, r64)
    rows, rows32 = row_rms(got, model, ROW_DIM[name]), row_rms(r32, r64, ROW_DIM[name])
    ratios = rows / rows32.clamp_min(sm.FLOOR)
    fig = {"e": e, "e_fp32": e32, "ratio": e / max(e32, sm.FLOOR), "worst_row_ratio": float(ratios.max())}
    bad = []
    if not fig["ratio"] <= k_whole:
        bad.append((name, "whole", fig["ratio"], k_whole))
    if not fig["worst_row_ratio"] <= k_row:
        bad.append((name, "worst row", fig["worst_row_ratio"], k_row))
    return bad, fig


# ---- the input sets of the GPU test, rehearsed on the CPU by tests/test_conv_split_ref_cpu.py ------------------------------------
SLOPE = 0.1
# (Cin, Cout, k, dilation): the smallest instance; Cin no multiple of the chunk; span 50, rows pad to the tile, 11 accumulators;
# four channel blocks per workgroup; class-3 rows for the data gradient and class-0 rows for the forward; the discriminators' layer
LAYERS = [(32, 32, 3, 1), (33, 64, 7, 1), (64, 48, 11, 5), (128, 128, 7, 3), (256, 32, 5, 1), (1024, 1024, 5, 1)]
MPD_ROWS = [11, 12, 55, 56, 1, 2]  # the period discriminators' short rows, for 1024 -> 1024
STEP_EDGES = [15, 16, 17, 63, 64, 65, 71, 72, 73, 129]  # MFMA-step (16) and chunk (64) edges


def tile_widths(lib, cin, cout, k, d, B, ld):
    """the conv_bf3_kernel tile widths in play: the forward's (rows = Cout) and the data gradient's (rows = Cin), from
    dissc_bf3_info at this batch"""
    return sorted({lib.bf3_conv_info(cin, cout, k, d, B, ld)["bn"], lib.bf3_conv_info(cout, cin, k, d, B, ld)["bn"]})


def lengths_for(lib, layer):
    """(lengths, ld) of the layer's one ragged batch: 0, 1, 2, pad, pad + 1, the step and chunk edges, every tile width +- 1, and
    one utterance of exactly ld = the largest length rounded up to 4 columns"""
    cin, cout, k, d = layer
    if layer == (1024, 1024, 5, 1):
        return list(MPD_ROWS), max(MPD_ROWS)
    pad = (k - 1) * d // 2
    base = [0, 1, 2, pad, pad + 1] + STEP_EDGES
    widths = tile_widths(lib, cin, cout, k, d, len(base) + 7, 260)
    lengths = base + [w + e for w in widths for e in (-1, 0, 1)]
    ld = (max(lengths) + 3) // 4 * 4
    lengths.append(ld)
    assert tile_widths(lib, cin, cout, k, d, len(lengths), ld) == widths, "the widths were taken at another batch"
    return lengths, ld


def inputs(lib, layer, seed=None):
    """(x, w, b, gy, lengths, ld) on the CPU: tests/conv_grad_harness.py's seeded data, x and gy NaN beyond every length"""
    import conv_grad_harness as H
    cin, cout, k, d = layer
    lengths, ld = lengths_for(lib, layer)
    x, w, b, gy = H.case(H.Spec("conv1d", cin, cout, k, d), len(lengths), ld, seed=cin + cout + k if seed is None else seed)
    for i, n in enumerate(lengths):
        x[i, :, n:] = float("nan")
        gy[i, :, n:] = float("nan")
    return x, w, b, gy, lengths, ld


def references(x, w, b, gy, lengths, d, slope=SLOPE):
    """(model, r64, r32): the split model and torch autograd in float64 / float32 on the unsplit operands, each (y, gx, gw, gb)"""
    import conv_grad_ref as R
    xz, gz = torch.nan_to_num(x), torch.nan_to_num(gy)
    r64 = R.layer_ref(xz, w, b, gz, lengths, R.conv_op(d), slope, torch.float64)
    r32 = R.layer_ref(xz, w, b, gz, lengths, R.conv_op(d), slope, torch.float32)
    return layer(x, w, b, gy, lengths, d, slope), r64, r32
