"""The one-launch F(2,3) chains of the k = 3 ResBlocks (reschain32_f23_kernel, reschain16_f23_kernel; not a test module): a Python
restatement of F23ChainGeo (respair_f23.h), a numpy model of the chain in the kernels' fp32 arithmetic -- tile by tile, in the
kernels' buffer coordinates, with NaN wherever a kernel's LDS holds stale data -- next to a direct-order fp32 model and float64,
the data of tests/test_gpu_chain_f23.py, and that test's bars.  Shared by tests/test_chain_f23_model_cpu.py and
tests/test_gpu_chain_f23.py."""
from collections import namedtuple

import numpy as np
import torch

SLOPE = 0.1
DILS = (1, 3, 5)
K = 3
G23 = np.array([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]])

Geo = namedtuple("Geo", "C ncols span halo padl wout xw tiles_per_wave t0 nc1")


def round32_16(n):
    return (n - 16 + 31) // 32 * 32 + 16


def geo(C, halo=12):
    """F23ChainGeo: buffer coordinate p <-> time o0 - halo + p; conv_1's outputs p in [0, span) are computed in every pair, the
    owned ones are [halo, halo + wout); pair m's conv_d produces T on [t0[m], t0[m] + 2 nc1[m])"""
    wcols = {32: 32, 16: 64}[C]
    ncols = 4 * wcols
    span = 2 * ncols
    return Geo(C=C, ncols=ncols, span=span, halo=halo, padl=4, wout=span - 2 * halo, xw=round32_16(4 + span + 8),
               tiles_per_wave=wcols // (16 if C == 16 else 32), t0=(1, 3, 4), nc1=tuple(ncols // d * d for d in DILS))


def valid_ranges(g):
    """[(a, b)] for x_0 .. x_3: where each is valid in buffer coordinates, and whether every read stays inside the LDS row"""
    a, b = -g.padl, g.xw - g.padl
    out, in_row = [(a, b)], True
    for m, d in enumerate(DILS):
        lo, hi = g.t0[m], g.t0[m] + 2 * g.nc1[m]
        in_row = in_row and lo - d >= -g.padl and hi + d <= g.xw - g.padl and g.padl + g.span + 3 <= g.xw
        tlo, thi = max(lo, a + d), min(hi, b - d)          # T_m: its three samples are valid x_m
        a, b = max(tlo + 1, 0), min(thi - 1, g.span)       # x_m+1: its three samples are valid T_m, and it is written
        out.append((a, b))
    return out, in_row


def owners(L, g):
    """for each output t in [0, L): the tiles (first output o0) whose owned buffer coordinates [halo, halo + wout) hold it, found
    from the kernels' side: tile j of the ceil(L / wout) the launch enumerates has o0 = j wout, its coordinate p is time
    o0 - halo + p, and it stores the owned p whose time is below L"""
    own = [[] for _ in range(L)]
    for j in range(-(-L // g.wout)):
        o0 = j * g.wout
        for p in range(g.span):
            t = o0 - g.halo + p
            if g.halo <= p < g.halo + g.wout and 0 <= t < L:
                own[t].append(o0)
    return own


# ------------------------------------------------------------------------------------------------------------------------
# arithmetic
# ------------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in float64; one rounding to fp32 after the sum"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def lrelu(v, slope=SLOPE):
    return np.where(v > 0, v, v * v.dtype.type(slope))


def transform(w):
    """U[p][co][ci] = G w in double, rounded once (pair_host.hip's transform_taps)"""
    return np.einsum("pi,oci->poc", G23, w.astype(np.float64)).astype(np.float32)


def f23_columns(buf, U, first, step):
    """the kernels' tap loop: column j reads buf[:, first[j] + q step], q = 0 .. 3; one fused multiply-add per input channel in
    ascending order and point; A^T as the kernels' three additions.  Returns (even, odd) outputs [Co, columns] without bias"""
    Co = U.shape[1]
    acc = [np.zeros((Co, first.size), np.float32) for _ in range(4)]
    for ci in range(buf.shape[0]):
        x0, x1, x2, x3 = [buf[ci, first + q * step] for q in range(4)]
        b = [x0 - x2, x1 + x2, x2 - x1, x1 - x3]
        for p in range(4):
            acc[p] = fma32(U[p][:, ci][:, None], b[p][None, :], acc[p])
    return (acc[0] + acc[1]) + acc[2], (acc[1] - acc[2]) - acc[3]


def conv_f23(x, w, d):
    """x [C, L] fp32 (activated, zero outside), w [Co, Ci, 3] -> conv without bias in the F(2,3) arithmetic, units of 2 d outputs
    from t = 0 (tests/test_f23_c64_model.py's _conv_f23)"""
    L = x.shape[1]
    nu = -(-L // (2 * d))
    xp = np.zeros((x.shape[0], nu * 2 * d + 2 * d + 1), np.float32)
    xp[:, d:d + L] = x
    first = (2 * d * np.arange(nu)[:, None] + np.arange(d)[None, :]).ravel()
    ye, yo = f23_columns(xp, transform(w), first, d)
    out = np.zeros((w.shape[0], nu * 2 * d), np.float32)
    out[:, first], out[:, first + d] = ye, yo
    return out[:, :L]


def conv_direct(x, w, d, dtype):
    """the direct order: one fused multiply-add chain per output over (tap, channel); dtype float64 is the reference"""
    Co, Ci, k = w.shape
    L, P = x.shape[1], (k - 1) // 2 * d
    xp = np.zeros((Ci, L + 2 * P), dtype)
    xp[:, P:P + L] = x
    acc = np.zeros((Co, L), dtype)
    for tap in range(k):
        for ci in range(Ci):
            a, b = w[:, ci, tap].astype(dtype)[:, None], xp[ci, tap * d:tap * d + L][None, :]
            acc = fma32(a, b, acc) if dtype == np.float32 else acc + a * b
    return acc


def chain_plain(x, w6, b6, conv, slope=SLOPE):
    """the three pairs on one whole utterance x [C, L] with `conv(x, w, d)` as the conv: x = (conv_1(T) + b2) + x"""
    dt = x.dtype
    for m, d in enumerate(DILS):
        t = lrelu(conv(lrelu(x, slope), w6[2 * m], d) + b6[2 * m].astype(dt)[:, None], slope)
        x = (conv(t, w6[2 * m + 1], 1) + b6[2 * m + 1].astype(dt)[:, None]) + x
    return x


def chain_f64(x, w6, b6, slope=SLOPE):
    return chain_plain(x.astype(np.float64), [w.astype(np.float64) for w in w6], b6, lambda v, w, d: conv_direct(v, w, d, np.float64),
                       slope)


def chain_direct32(x, w6, b6, slope=SLOPE):
    return chain_plain(x, w6, b6, lambda v, w, d: conv_direct(v, w, d, np.float32), slope)


def chain_tiled(x, w6, b6, slope=SLOPE, defect=None):
    """reschain32/16_f23_kernel on one utterance x [C, L] fp32, tile by tile as the kernels index it.  What a kernel leaves stale in
    its LDS row is NaN here, so a column that must not feed a valid output poisons it.  defect: None, or a seeded bug --
    "x_not_zeroed" (lrelu(x_k+1) written as computed beyond the utterance), "halo11" (a halo of 11: the tiles own one output
    more on each side than the valid range holds), "res_activated" (the residual taken from the activated window)"""
    C, L = x.shape
    g = geo(C, halo=11) if defect == "halo11" else geo(C)
    U = [transform(w) for w in w6]
    out = np.full((C, L), np.nan, np.float32)
    for o0 in range(0, L, g.wout):
        t00 = o0 - g.halo
        tw = t00 - g.padl + np.arange(g.xw)                       # the staged window's times
        inw = (tw >= 0) & (tw < L)
        xs = np.where(inw, lrelu(x[:, np.clip(tw, 0, L - 1)], slope), np.float32(0))
        tp = t00 + np.arange(g.span)                               # conv_1's outputs
        inp = (tp >= 0) & (tp < L)
        raw = x[:, np.clip(tp, 0, L - 1)]
        res = np.where(inp, lrelu(raw, slope) if defect == "res_activated" else raw, np.float32(np.nan))
        for m, d in enumerate(DILS):
            c = np.arange(g.nc1[m])
            pe = g.t0[m] + 2 * d * (c // d) + c % d
            ve, vo = f23_columns(xs, U[2 * m], g.padl + pe - d, d)
            T = np.full((C, g.xw), np.nan, np.float32)
            for pos, v in ((pe, ve), (pe + d, vo)):
                tt = t00 + pos
                T[:, g.padl + 1 + pos] = np.where((tt >= 0) & (tt < L), lrelu(v + b6[2 * m][:, None], slope), np.float32(0))
            ye, yo = f23_columns(T, U[2 * m + 1], g.padl + 2 * np.arange(g.ncols), 1)
            new = np.empty_like(res)
            new[:, 0::2] = (ye + b6[2 * m + 1][:, None]) + res[:, 0::2]
            new[:, 1::2] = (yo + b6[2 * m + 1][:, None]) + res[:, 1::2]
            res = new
            xs = np.full((C, g.xw), np.nan, np.float32)
            act = lrelu(res, slope)
            xs[:, g.padl:g.padl + g.span] = act if defect == "x_not_zeroed" else np.where(inp, act, np.float32(0))
        own = np.arange(g.halo, g.halo + g.wout)
        own = own[(t00 + own < L) & (t00 + own >= 0)]
        out[:, t00 + own] = res[:, own]
    return out


# ------------------------------------------------------------------------------------------------------------------------
# the GPU test's data and bars
# ------------------------------------------------------------------------------------------------------------------------
LD = 2000


def lengths_for(C):
    """row 0 is the longest; then the shortest rows, the halo's edges, the tile's edges, two tiles, one wave's owned span"""
    g = geo(C)
    w, wave = g.wout, 2 * g.ncols // 4  # a wave computes span / 4 outputs: its owned span ends at halo + wave - halo = wave
    ls = [2000, 1, 2, 7, 11, 12, 13, 23, 24, 25, 63, 64, 65, w - 13, w - 12, w - 1, w, w + 1, w + 11, w + 12, w + 13,
          2 * w - 1, 2 * w + 1, wave - g.halo - 1, wave - g.halo, wave - g.halo + 1, 1999]
    return [n for n in ls if 0 < n <= LD]


def data(C, lengths, ld, seed):
    """pair_harness.data's draws for six convs: x [B, C, ld] uniform in (-1, 1) with NaN beyond every length, weights scaled
    0.9 / sqrt(C k), biases within 0.1.  CPU tensors"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(len(lengths), C, ld, generator=g) * 2 - 1
    for i, n in enumerate(lengths):
        x[i, :, n:] = float("nan")  # never read
    sc = 0.9 / (C * K) ** 0.5
    w6 = [((torch.rand(C, C, K, generator=g) * 2 - 1) * sc).contiguous() for _ in range(6)]
    b6 = [((torch.rand(C, generator=g) * 2 - 1) * 0.1).contiguous() for _ in range(6)]
    return x, w6, b6


def reference(x, w6, b6, lengths):
    """float64, one utterance at a time on its own samples (zero "same" padding at every layer).  x on any device"""
    import torch.nn.functional as F
    out = torch.zeros_like(x, dtype=torch.float64)
    for i, n in enumerate(lengths):
        if n == 0:
            continue
        v = x[i:i + 1, :, :n].double()
        for m, d in enumerate(DILS):
            t = F.conv1d(F.leaky_relu(v, SLOPE), w6[2 * m].double().to(x.device), b6[2 * m].double().to(x.device), padding=d, dilation=d)
            v = v + F.conv1d(F.leaky_relu(t, SLOPE), w6[2 * m + 1].double().to(x.device), b6[2 * m + 1].double().to(x.device), padding=1)
        out[i, :, :n] = v[0]
    return out


def errors(y, ref, lengths):
    """(max error over every utterance, rms error on row 0), the figures of pair_harness.check_pair"""
    worst = max(float((y[i, :, :n].double() - ref[i, :, :n]).abs().max()) for i, n in enumerate(lengths) if n)
    return worst, float(((y[0, :, :lengths[0]].double() - ref[0, :, :lengths[0]]) ** 2).mean().sqrt())


def within_bars(err, base):
    """the GPU test's accuracy bars: rms <= max(3 x the three-launch form's, 1e-6) and max <= 3 x the three-launch form's max"""
    return err[1] <= max(3.0 * base[1], 1e-6) and err[0] <= 3.0 * base[0]
