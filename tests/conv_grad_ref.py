"""Shared by tests/test_conv_grad_cpu.py and tests/test_gpu_conv_grad.py (not a test module): the float64 / float32 torch
restatement of dissc_amd.nn's layers, the generator's layer shapes, and the bars the gradients are held to."""
import collections
import math

import torch
import torch.nn.functional as F

from oracle import train_stages_ref as S
import train_stage_cases as C

SLOPE = 0.1  # reference sr/models.py:13


def generator_layer_shapes(frames=28):
    """every stride-1 conv of the reference generator (synthdata.VCTK_CONFIG) as (Cin, Cout, k, dilation, L) at ``frames``
    input frames: conv_pre, the ResBlock convs of the five stages, conv_post"""
    import synthdata as synth
    cfg = synth.VCTK_CONFIG
    shapes = [(cfg["model_in_dim"], cfg["upsample_initial_channel"], 7, 1, frames)]
    L, ch = frames, cfg["upsample_initial_channel"]
    for u in cfg["upsample_rates"]:
        L, ch = L * u, ch // 2
        for k, dils in zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]):
            for d in sorted(set(dils) | {1}):
                shapes.append((ch, ch, k, d, L))
    shapes.append((ch, 1, 7, 1, L))
    return shapes


Op = collections.namedtuple("Op", "apply mul cout_dim")  # apply(lrelu(x), w, b); rows of y per row of x; Cout's dim in w


def conv_op(dilation):
    """F.conv1d, "same" padding: w [Cout, Cin, k]"""
    return Op(lambda xa, w, b: F.conv1d(xa, w, b, padding=(w.shape[2] - 1) * dilation // 2, dilation=dilation), 1, 0)


def conv_transpose_op(stride):
    """F.conv_transpose1d, padding (k - stride) // 2: w [Cin, Cout, k], stride outputs per input"""
    return Op(lambda xa, w, b: F.conv_transpose1d(xa, w, b, stride=stride, padding=(w.shape[2] - stride) // 2), stride, 1)


def _ragged(x, lengths, gy, cout, mul, fn):
    """y [B, cout, mul ld]: fn(i, n, x_i) of every utterance alone on its valid part x_i = x[i:i + 1, :, :n] (n = lengths[i], or
    ld), zero beyond mul n.  With gy (same dtype as x) the backward of sum(y gy) has run on return.  Returns (y, gx), gx zero
    beyond n."""
    B, _, ld = x.shape
    y = torch.zeros(B, cout, mul * ld, dtype=x.dtype)
    gx = torch.zeros_like(x)
    loss, xs = 0, []
    for i in range(B):
        n = ld if lengths is None else int(lengths[i])
        if n <= 0:
            xs.append(None)
            continue
        xi = x[i:i + 1, :, :n].clone().requires_grad_(gy is not None)
        xs.append(xi)
        yi = fn(i, n, xi)
        assert yi.shape[2] == mul * n
        y[i, :, :mul * n] = yi[0].detach()
        if gy is not None:
            loss = loss + (yi * gy[i:i + 1, :, :mul * n]).sum()
    if torch.is_tensor(loss):
        loss.backward()
    for i, xi in enumerate(xs):
        if xi is not None and xi.grad is not None:
            gx[i, :, :xi.shape[2]] = xi.grad[0]
    return y, gx


def _grad(t):
    return (t.grad if t.grad is not None else torch.zeros_like(t)).detach()


def layer_ref(x, w, b, gy, lengths, op, in_slope, dtype):
    """(y, gx, gw, gb) of y = b + op(lrelu(x, in_slope), w) by torch autograd, op = conv_op(dilation) or
    conv_transpose_op(stride), per utterance on its valid INPUT length n (op.mul * n outputs); y and gx are zero beyond.
    b may be None (gb is then None)."""
    x = x.detach().to("cpu", dtype)
    gy = gy.detach().to("cpu", dtype)
    w = w.detach().to("cpu", dtype).requires_grad_(True)
    bb = None if b is None else b.detach().to("cpu", dtype).requires_grad_(True)
    y, gx = _ragged(x, lengths, gy, w.shape[op.cout_dim], op.mul, lambda i, n, xi: op.apply(F.leaky_relu(xi, in_slope), w, bb))
    return y, gx, _grad(w), None if bb is None else _grad(bb)


def _lrelu(x, slope, mask):
    """leaky ReLU whose branch comes from ``mask`` (True: identity) when given, else from x's own sign"""
    if mask is None:
        return F.leaky_relu(x, slope)
    return torch.where(mask, x, x * slope)


def resblock_chain(h, wd, k, dilations, mask, tap=None):
    """ResBlock1 on one utterance h [1, C, n]; wd: resblock1_ref's dict.  mask(j): the branch decisions of conv input j
    (call order) or None; tap(j, t), if given, receives conv input j."""
    for m, d in enumerate(dilations):
        t = F.conv1d(_lrelu(h, SLOPE, mask(2 * m)), wd[f"convs1.{m}.weight"], wd[f"convs1.{m}.bias"], padding=(k - 1) * d // 2,
                     dilation=d)
        if tap is not None:
            tap(2 * m, h), tap(2 * m + 1, t)
        t = F.conv1d(_lrelu(t, SLOPE, mask(2 * m + 1)), wd[f"convs2.{m}.weight"], wd[f"convs2.{m}.bias"], padding=(k - 1) // 2)
        h = t + h
    return h


def mask_of(masks, i, cols):
    """resblock_chain's ``mask`` for utterance i: conv input j's decisions masks[j][i, :, :cols] (masks None: its own sign)"""
    return (lambda j: None) if masks is None else (lambda j: masks[j][i:i + 1, :, :cols].cpu())


def resblock1_ref(w, x, k, dilations, dtype, masks=None, lengths=None, gy=None, taps=None):
    """ResBlock1 on the CPU in ``dtype``; w: {"convs1.<m>.weight" / ".bias", "convs2.<m>..."}.  masks: a list of six
    boolean tensors (x > 0 of every conv's input, in call order) that replace each leaky ReLU's own branch decision.
    lengths: per-utterance valid lengths (each utterance is run alone on its valid part).  Returns y, or with ``gy``
    (y, gx, {name: gradient}) by autograd.  taps: a list that receives this evaluation's own six conv inputs ([B, C, ld],
    zero beyond lengths)."""
    wd = {n: t.detach().to("cpu", dtype).requires_grad_(gy is not None) for n, t in w.items()}
    x = x.detach().to("cpu", dtype)
    if taps is not None:
        taps.extend(torch.zeros_like(x) for _ in range(2 * len(dilations)))

    def block(i, n, xi):
        tap = None if taps is None else (lambda j, t: taps[j][i, :, :n].copy_(t[0].detach()))
        return resblock_chain(xi, wd, k, dilations, mask_of(masks, i, n), tap)

    y, gx = _ragged(x, lengths, None if gy is None else gy.detach().to("cpu", dtype), x.shape[1], 1, block)
    return y if gy is None else (y, gx, {n: _grad(t) for n, t in wd.items()})


# ---- the bars (tests/train_stage_cases.py): e <= K * max(e_cpu, 2^-24 rms(R64)), whole tensor and worst channel / row ----
K_WHOLE, K_CH = C.K_WHOLE, C.K_CH


def k_cap(n):
    """the most an exception may ask: min(32, max(4, sqrt(n))), n = products in one output's sum"""
    return min(32.0, max(4.0, math.sqrt(n)))


def compare(kind, y, r64, r32):
    """kind: "act" ([B, C, L]: per channel), "weight" ([Cout, Cin, k]: per row), "vec" (no per-channel figure).
    Returns oracle.train_stages_ref.compare's dict (ratio, ch_ratio, e_gpu, e_cpu, ref, finite)."""
    key = {"act": "layer/x", "weight": "grad/w", "vec": "vec"}[kind]
    return S.compare(key, y.detach().cpu(), r64, r32)


def check(tag, kind, y, r64, r32, k_whole=K_WHOLE, k_ch=K_CH, verbose=True):
    """holds one tensor to the bars; prints the figures first; returns the list of violations"""
    m = compare(kind, y, r64, r32)
    if verbose:
        print(f"CG {tag:44s} e {m['e_gpu']:.3e} e_cpu {m['e_cpu']:.3e} ref {m['ref']:.3e} ratio {m['ratio']:6.3f} bar {k_whole:g}"
              f" | worst channel {m['ch_ratio']:6.3f} bar {k_ch:g}")
    bad = []
    if not m["finite"]:
        bad.append((tag, "not finite"))
    if not m["ratio"] <= k_whole:
        bad.append((tag, "ratio", m["ratio"], k_whole))
    if not m["ch_ratio"] <= k_ch:
        bad.append((tag, "ch_ratio", m["ch_ratio"], k_ch))
    return bad
