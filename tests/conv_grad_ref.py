"""Shared by the tests of dissc_amd.nn's differentiable layers (not a test module): the float64 / float32 torch restatement of
the four conv layers (one layer_ref over an Op, every utterance alone on its valid part), the row-length and mask helpers, the
kernels' phase form of the strided and grouped layers (for seeding defects), the ResBlock chain, the generator's layer shapes,
and the bars the gradients are held to."""
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


# apply(lrelu(x), w, b); out_len(n): the outputs of n valid inputs; Cout's dim in w
Op = collections.namedtuple("Op", "apply out_len cout_dim")


def cdiv(a, b):
    return -(-a // b)


def ceil4(n):
    return (n + 3) // 4 * 4


def out_ld(ld, s):
    """the row length of a stride-s layer's y for a row length ld of x"""
    return ceil4(cdiv(ld, s))


def conv_op(dilation):
    """F.conv1d, "same" padding: w [Cout, Cin, k], n outputs"""
    return Op(lambda xa, w, b: F.conv1d(xa, w, b, padding=(w.shape[2] - 1) * dilation // 2, dilation=dilation), lambda n: n, 0)


def conv_transpose_op(stride):
    """F.conv_transpose1d, padding (k - stride) // 2: w [Cin, Cout, k], stride n outputs"""
    return Op(lambda xa, w, b: F.conv_transpose1d(xa, w, b, stride=stride, padding=(w.shape[2] - stride) // 2),
              lambda n: stride * n, 1)


def strided_op(stride, groups=1):
    """F.conv1d at a stride, padding (k - 1) // 2, in groups: w [Cout, Cin / groups, k], ceil(n / stride) outputs"""
    return Op(lambda xa, w, b: F.conv1d(xa, w, b, stride=stride, padding=(w.shape[2] - 1) // 2, groups=groups),
              lambda n: cdiv(n, stride), 0)


def y_ld(ld, op):
    """the row length of y for a row length ld of x: out_len(ld) rounded up to a multiple of 4, as the library allocates it (its
    rows of x are multiples of 4; the float64 cases on other rows, CPU only, keep out_len(ld))"""
    return ceil4(op.out_len(ld)) if ld % 4 == 0 else op.out_len(ld)


def valid_masks(lengths, ld, op):
    """([B, 1, ld], [B, 1, y_ld]) float masks of the valid input / output positions: n and out_len(n)"""
    vi, vo = torch.zeros(len(lengths), 1, ld), torch.zeros(len(lengths), 1, y_ld(ld, op))
    for i, n in enumerate(lengths):
        vi[i, :, :n] = 1
        vo[i, :, :op.out_len(n)] = 1
    return vi, vo


def _ragged(x, lengths, gy, cout, op, fn):
    """y [B, cout, y_ld]: fn(i, n, x_i) of every utterance alone on its valid part x_i = x[i:i + 1, :, :n] (n = lengths[i], or
    ld), zero beyond its op.out_len(n) outputs.  With gy (same dtype as x) the backward of sum(y gy) has run on return.  Returns
    (y, gx), gx zero beyond n."""
    B, _, ld = x.shape
    y = torch.zeros(B, cout, y_ld(ld, op), dtype=x.dtype)
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
        m = op.out_len(n)
        assert yi.shape[2] == m
        y[i, :, :m] = yi[0].detach()
        if gy is not None:
            loss = loss + (yi * gy[i:i + 1, :, :m]).sum()
    if torch.is_tensor(loss):
        loss.backward()
    for i, xi in enumerate(xs):
        if xi is not None and xi.grad is not None:
            gx[i, :, :xi.shape[2]] = xi.grad[0]
    return y, gx


def _grad(t):
    return (t.grad if t.grad is not None else torch.zeros_like(t)).detach()


def layer_ref(x, w, b, gy, lengths, op, in_slope, dtype):
    """(y, gx, gw, gb) of y = b + op(lrelu(x, in_slope), w) by torch autograd, op = conv_op(dilation), conv_transpose_op(stride)
    or strided_op(stride, groups), per utterance on its valid INPUT length n (op.out_len(n) outputs); y and gx are zero beyond.
    b may be None (gb is then None)."""
    x = x.detach().to("cpu", dtype)
    gy = gy.detach().to("cpu", dtype)
    w = w.detach().to("cpu", dtype).requires_grad_(True)
    bb = None if b is None else b.detach().to("cpu", dtype).requires_grad_(True)
    y, gx = _ragged(x, lengths, gy, w.shape[op.cout_dim], op, lambda i, n, xi: op.apply(F.leaky_relu(xi, in_slope), w, bb))
    return y, gx, _grad(w), None if bb is None else _grad(bb)


def taps(k, s, pad=None):
    """[(plane, shift)] of tap kk of a stride-s layer: kk - pad = s * shift + plane, 0 <= plane < s"""
    pad = (k - 1) // 2 if pad is None else pad
    return [((kk - pad) % s, (kk - pad - (kk - pad) % s) // s) for kk in range(k)]


def phase_layer(xa, w, b, gym, lengths, s, g=1, drop_tap=None, tap_shift=None, plane_shift=None, next_group=False, floor_len=False,
                pad=None):
    """(y, gw) of the strided / grouped layer in the kernels' phase form, a CPU stand-in: plane_p[ci][q] = xa[ci][s q + p], tap kk
    reads plane_p(kk)[q + dl(kk)] of the channels [grp cig, (grp + 1) cig) of its group.  xa = lrelu(x) and gym = gy, both already
    zero beyond the lengths.  Defects: drop_tap = kk (left out), tap_shift = (kk, n) (tap kk read n positions late), plane_shift =
    (p, n) (plane p read n positions late), next_group (group grp reads the input channels of group grp + 1, the last one those
    of group 0), floor_len (the output length taken as floor(n / s)), pad (the padding taken as this in place of (k - 1) / 2)."""
    B, cin, ld = xa.shape
    cout, cig, k = w.shape
    cog = cout // g
    assert cig * g == cin and cog * g == cout
    Q, H = out_ld(ld, s), 24  # the halo: k = 41 at stride 1 shifts by 20, and a defect by one more
    xp = F.pad(xa, (0, s * (Q + H) - ld))
    y = torch.zeros(B, cout, Q, dtype=xa.dtype)
    gw = torch.zeros_like(w)
    vo = torch.zeros(B, 1, Q, dtype=xa.dtype)
    for i, n in enumerate(lengths):
        vo[i, :, :(n // s if floor_len else cdiv(n, s))] = 1
    for kk, (p, dl) in enumerate(taps(k, s, pad)):
        if kk == drop_tap:
            continue
        if tap_shift is not None and tap_shift[0] == kk:
            dl += tap_shift[1]
        if plane_shift is not None and plane_shift[0] == p:
            dl += plane_shift[1]
        pl = F.pad(xp[:, :, p::s], (H, 0))  # column c = position c - H
        win = pl[:, :, H + dl:H + dl + Q]
        for grp in range(g):
            src = (grp + 1) % g if next_group else grp
            wi = win[:, src * cig:(src + 1) * cig]
            co = slice(grp * cog, (grp + 1) * cog)
            y[:, co] += torch.einsum("oi,biq->boq", w[co, :, kk], wi)
            gw[co, :, kk] = torch.einsum("boq,biq->oi", (gym * vo)[:, co], wi)
    return (y + b.view(1, -1, 1)) * vo, gw


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

    y, gx = _ragged(x, lengths, None if gy is None else gy.detach().to("cpu", dtype), x.shape[1], conv_op(1), block)
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
