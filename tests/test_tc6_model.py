"""The six-point Toom-Cook form of the narrow residual pairs (respair32_tc6_kernel, respair_f23.hip), checked without a GPU:
the matrices of F(3,4) at the points 0, +-1, +-2, inf in exact rational arithmetic, and a numpy model of a whole pair in the
kernel's fp32 arithmetic (operands rounded to fp32, one rounding per fused multiply-add, the kernel's order of channels,
sub-filters and transform steps) against float64, next to a direct-order fp32 model of the same pair.

The host packing (pack_pair_reg: U = G w in double, rounded once) uploads to the device and has no host-only entry, so it is
covered by the GPU tests (tests/test_gpu_pairs_tc6.py); the model below forms U the same way."""
import functools
from fractions import Fraction as Fr

import numpy as np
import pytest

BT = [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]]
AT = [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 1]]
G = [[Fr(1, 4), 0, 0, 0], [Fr(-1, 6)] * 4, [Fr(-1, 6), Fr(1, 6), Fr(-1, 6), Fr(1, 6)],
     [Fr(1, 24), Fr(2, 24), Fr(4, 24), Fr(8, 24)], [Fr(1, 24), Fr(-2, 24), Fr(4, 24), Fr(-8, 24)], [0, 0, 0, 1]]
SLOPE = 0.1


def test_f34_matrices_satisfy_the_bilinear_identity_exactly():
    """y_m = sum_i g_i d_(m + i), m = 0..2, equals A^T [(G g) . (B^T d)] for every unit vector pair (g_i, d_n): the coefficient
    of g_i d_n in output m is sum_p A^T[m][p] G[p][i] B^T[p][n] = [n == m + i]"""
    for m in range(3):
        for i in range(4):
            for n in range(6):
                c = sum(Fr(AT[m][p]) * Fr(G[p][i]) * Fr(BT[p][n]) for p in range(6))
                assert c == (1 if n == m + i else 0), (m, i, n, c)


def test_kernel_transform_steps_are_the_matrices():
    """the shared sums the kernel uses for B^T (8 fused multiply-adds, 4 additions) and A^T, on exact integers"""
    rs = np.random.RandomState(0)
    x = rs.randint(-50, 50, size=(6, 100)).astype(np.float64)
    b = _bt(*x, fma=lambda a, b_, c: a * b_ + c)
    assert np.array_equal(np.stack(b), np.array(BT, np.float64) @ x)
    y = _at(*x, fma=lambda a, b_, c: a * b_ + c)
    assert np.array_equal(np.stack(y), np.array(AT, np.float64) @ x)


# ------------------------------------------------------------------------------------------------------------------------
# the fp32 model
# ------------------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in float64; one rounding to fp32 after the sum"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _bt(x0, x1, x2, x3, x4, x5, fma):
    one = x0.dtype.type
    pe, po, re, ro = fma(one(-4), x2, x4), fma(one(-4), x1, x3), x4 - x2, x3 - x1
    return [fma(one(4), x0, fma(one(-5), x2, x4)), pe + po, pe - po, fma(one(2), ro, re), fma(one(-2), ro, re),
            fma(one(4), x1, fma(one(-5), x3, x5))]


def _at(Y0, Y1, Y2, Y3, Y4, Y5, fma):
    one = Y0.dtype.type
    s12, d12, s34, d34 = Y1 + Y2, Y1 - Y2, Y3 + Y4, Y3 - Y4
    return [(Y0 + s12) + s34, fma(one(2), d34, d12), fma(one(4), s34, s12) + Y5]


def _conv_tc6(x, w, d):
    """x [C, L] fp32 (activated, zero outside), w [Co, Ci, k] fp32 -> conv without bias [Co, L] fp32, in the kernel's arithmetic"""
    Co, Ci, k = w.shape
    ns, L = (k + 3) // 4, x.shape[1]
    D, P = d * ns, (k - 1) // 2 * d
    nu = -(-L // (3 * D))
    xp = np.zeros((Ci, nu * 3 * D + (4 * ns - 1) * d + 1), np.float32)
    xp[:, P:P + L] = x  # x(t - P + tap d) = xp[t + tap d]
    first = (3 * D * np.arange(nu)[:, None] + np.arange(D)[None, :]).ravel()
    Gd = np.array([[float(v) for v in row] for row in G])
    wz = np.zeros((Co, Ci, 4 * ns))
    wz[:, :, :k] = w
    acc = [np.zeros((Co, first.size), np.float32) for _ in range(6)]
    for chunk in range(Ci // 16):
        for j in range(ns):
            U = np.einsum("pi,oci->poc", Gd, wz[:, :, j::ns]).astype(np.float32)  # [6][Co][Ci]
            for ci in range(16 * chunk, 16 * chunk + 16):
                b = _bt(*[xp[ci, first + j * d + q * D] for q in range(6)], fma=_fma32)
                for p in range(6):
                    acc[p] = _fma32(U[p][:, ci][:, None], b[p][None, :], acc[p])
    y = _at(*acc, fma=_fma32)
    out = np.zeros((Co, nu * 3 * D), np.float32)
    for m in range(3):
        out[:, first + m * D] = y[m]
    return out[:, :L]


def _conv_direct(x, w, d, dtype):
    """the direct order: one fused multiply-add chain per output over (tap, channel); dtype float64 is the reference"""
    Co, Ci, k = w.shape
    L, P = x.shape[1], (k - 1) // 2 * d
    xp = np.zeros((Ci, L + 2 * P), dtype)
    xp[:, P:P + L] = x
    acc = np.zeros((Co, L), dtype)
    for tap in range(k):
        for ci in range(Ci):
            a, b = w[:, ci, tap].astype(dtype)[:, None], xp[ci, tap * d:tap * d + L][None, :]
            acc = _fma32(a, b, acc) if dtype == np.float32 else acc + a * b
    return acc


def _lrelu(v):
    return np.where(v > 0, v, v * v.dtype.type(SLOPE))


def _pair(x, w1, b1, w2, b2, d, conv):
    t = _lrelu(conv(_lrelu(x), w1, d) + b1[:, None])
    return x + (conv(t, w2, 1) + b2[:, None])


def _rms_errors(x, w1, b1, w2, b2, d, conv):
    """rms error against float64 of the pair with `conv` as its conv model and with the direct-order fp32 one; the signal's rms"""
    ref = _pair(x.astype(np.float64), w1.astype(np.float64), b1.astype(np.float64), w2.astype(np.float64), b2.astype(np.float64), d,
                lambda v, w, dd: _conv_direct(v, w, dd, np.float64))
    y6 = _pair(x, w1, b1, w2, b2, d, conv)
    yd = _pair(x, w1, b1, w2, b2, d, lambda v, w, dd: _conv_direct(v, w, dd, np.float32))
    assert y6.dtype == np.float32 and yd.dtype == np.float32
    return float(np.sqrt(np.mean((y6 - ref) ** 2))), float(np.sqrt(np.mean((yd - ref) ** 2))), float(np.sqrt(np.mean(ref ** 2)))


@pytest.mark.parametrize("C", [32, 16])
@pytest.mark.parametrize("k", [7, 11])
@pytest.mark.parametrize("d", [1, 3, 5])
def test_six_point_pair_model_on_uniform_data(C, k, d):
    """data and weights as tests/test_gpu_pairs_f23.py::_data (uniform, weights scaled 0.9 / sqrt(C k)), L = 2000: the six-point
    pair's rms error against float64 stays within 3 x the direct-order model's"""
    rs = np.random.RandomState(100 * C + 10 * k + d)
    L, sc = 2000, 0.9 / (C * k) ** 0.5
    x = (rs.rand(C, L) * 2 - 1).astype(np.float32)
    w1, w2 = [((rs.rand(C, C, k) * 2 - 1) * sc).astype(np.float32) for _ in range(2)]
    b1, b2 = [((rs.rand(C) * 2 - 1) * 0.1).astype(np.float32) for _ in range(2)]
    e6, ed, _ = _rms_errors(x, w1, b1, w2, b2, d, _conv_tc6)
    print(f"C={C} k={k} d={d} uniform: six-point rms {e6:.2e}, direct order {ed:.2e}, ratio {e6 / ed:.2f}")
    assert e6 <= 3.0 * ed


@functools.lru_cache(maxsize=None)
def _trained_like():
    import torch
    from oracle import generator_ref as gr
    import synthdata as synth
    folded = gr.fold_state_dict(synth.synth_generator_state_dict(seed=0, kind="trained_like"))
    w64 = gr.to_double(folded)
    code, f0, spkr, _ = synth.synth_generator_inputs(1, 16, seed=199, kind="trained_like")
    x = gr.embed_concat(w64, torch.from_numpy(code), torch.from_numpy(f0), torch.from_numpy(spkr))
    conv_taps = {}
    gr.generator_forward(w64, synth.VCTK_CONFIG, x, taps={}, conv_taps=conv_taps)
    return folded, {key[:-2]: v[0].float().numpy() for key, v in conv_taps.items() if key.endswith(".x")}


@pytest.fixture(scope="module")
def trained_like():
    """the trained-like checkpoint (per-channel gains over decades, outlier channels, heavy tails) and the float64 oracle's
    inputs of every ResBlock conv on a trained-like utterance: built once per process, read-only"""
    return _trained_like()


@pytest.mark.parametrize("stage,C", [(3, 32), (4, 16)])
@pytest.mark.parametrize("k", [7, 11])
def test_six_point_pair_model_on_trained_like_draws(trained_like, stage, C, k):
    """the pairs of the 32- and 16-channel stages with their trained-like weights on the oracle's own inputs (2 000 columns):
    within 3 x the direct-order model's rms at every dilation"""
    folded, inp = trained_like
    j = (3, 7, 11).index(k)
    for m, d in enumerate((1, 3, 5)):
        p = f"resblocks.{3 * stage + j}"
        w1, b1 = folded[f"{p}.convs1.{m}.weight"].numpy(), folded[f"{p}.convs1.{m}.bias"].numpy()
        w2, b2 = folded[f"{p}.convs2.{m}.weight"].numpy(), folded[f"{p}.convs2.{m}.bias"].numpy()
        x = np.ascontiguousarray(inp[f"{p}.convs1.{m}"][:, 300:2300])
        assert x.shape == (C, 2000) and w1.shape == (C, C, k)
        e6, ed, sig = _rms_errors(x, w1, b1, w2, b2, d, _conv_tc6)
        print(f"C={C} k={k} d={d} trained-like: six-point rms {e6:.2e}, direct order {ed:.2e}, ratio {e6 / ed:.2f} (signal {sig:.3g})")
        assert e6 <= 3.0 * ed, (d, e6, ed)
