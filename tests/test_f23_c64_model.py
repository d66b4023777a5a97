"""The F(2,3) form of the 64-channel stage's k = 3 residual pairs (respair64_f23_kernel, respair_f23.hip), checked without a GPU:
the matrices at the points 0, 1, -1, inf in exact rational arithmetic, and a numpy model of a whole pair in the kernel's fp32
arithmetic (U = G w in double rounded once, B^T as one fp32 addition per operand, one fused multiply-add per input channel in
ascending order, A^T as the kernel's three additions) against float64, next to a direct-order fp32 model of the same pair.

The host packing uploads to the device and has no host-only entry: tests/test_gpu_pairs_c64.py covers it."""
from fractions import Fraction as Fr

import numpy as np
import pytest

from tc6_model import _conv_direct, _fma32, _rms_errors
from tc6_model import trained_like  # noqa: F401  (its fixture: the trained-like checkpoint and the oracle's conv inputs)

BT = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
AT = [[1, 1, 1, 0], [0, 1, -1, -1]]
G = [[1, 0, 0], [Fr(1, 2)] * 3, [Fr(1, 2), Fr(-1, 2), Fr(1, 2)], [0, 0, 1]]


def test_f23_matrices_satisfy_the_bilinear_identity_exactly():
    """y_m = sum_i g_i d_(m + i), m = 0..1, equals A^T [(G g) . (B^T d)]: the coefficient of g_i d_n in output m is [n == m + i]"""
    for m in range(2):
        for i in range(3):
            for n in range(4):
                c = sum(Fr(AT[m][p]) * Fr(G[p][i]) * Fr(BT[p][n]) for p in range(4))
                assert c == (1 if n == m + i else 0), (m, i, n, c)


def _conv_f23(x, w, d):
    """x [C, L] fp32 (activated, zero outside), w [Co, Ci, 3] fp32 -> conv without bias [Co, L] fp32, in the kernel's arithmetic:
    a column is the output pair (t, t + d) of a unit of 2 d outputs"""
    Co, Ci, k = w.shape
    assert k == 3
    L = x.shape[1]
    nu = -(-L // (2 * d))
    xp = np.zeros((Ci, nu * 2 * d + 2 * d + 1), np.float32)
    xp[:, d:d + L] = x  # x(t - d + tap d) = xp[t + tap d]
    first = (2 * d * np.arange(nu)[:, None] + np.arange(d)[None, :]).ravel()
    U = np.einsum("pi,oci->poc", np.array([[float(v) for v in row] for row in G]), w.astype(np.float64)).astype(np.float32)
    acc = [np.zeros((Co, first.size), np.float32) for _ in range(4)]
    for ci in range(Ci):
        x0, x1, x2, x3 = [xp[ci, first + q * d] for q in range(4)]
        b = [x0 - x2, x1 + x2, x2 - x1, x1 - x3]
        assert all(v.dtype == np.float32 for v in b)
        for p in range(4):
            acc[p] = _fma32(U[p][:, ci][:, None], b[p][None, :], acc[p])
    out = np.zeros((Co, nu * 2 * d), np.float32)
    out[:, first] = (acc[0] + acc[1]) + acc[2]
    out[:, first + d] = (acc[1] - acc[2]) - acc[3]
    return out[:, :L]


def test_model_is_exact_on_small_integers():
    """every product and sum is an integer below 2^24 (the halves of G on even weights): the F(2,3) model equals the direct conv"""
    rs = np.random.RandomState(1)
    x = rs.randint(-8, 9, size=(64, 301)).astype(np.float32)
    w = (2 * rs.randint(-4, 5, size=(64, 64, 3))).astype(np.float32)
    for d in (1, 3, 5):
        assert np.array_equal(_conv_f23(x, w, d), _conv_direct(x, w, d, np.float32)), d


@pytest.mark.parametrize("d", [1, 3, 5])
def test_f23_c64_pair_model_on_uniform_data(d):
    """data and weights as tests/test_gpu_pairs_f23.py::_data (uniform, weights scaled 0.9 / sqrt(C k)), L = 2000: the pair's rms
    error against float64 stays within 3 x the direct-order model's"""
    C, k = 64, 3
    rs = np.random.RandomState(100 * C + 10 * k + d)
    L, sc = 2000, 0.9 / (C * k) ** 0.5
    x = (rs.rand(C, L) * 2 - 1).astype(np.float32)
    w1, w2 = [((rs.rand(C, C, k) * 2 - 1) * sc).astype(np.float32) for _ in range(2)]
    b1, b2 = [((rs.rand(C) * 2 - 1) * 0.1).astype(np.float32) for _ in range(2)]
    ef, ed, _ = _rms_errors(x, w1, b1, w2, b2, d, _conv_f23)
    print(f"C={C} k={k} d={d} uniform: F(2,3) rms {ef:.2e}, direct order {ed:.2e}, ratio {ef / ed:.2f}")
    assert ef <= 3.0 * ed


def test_f23_c64_pair_model_on_trained_like_draws(trained_like):
    """the k = 3 pairs of the 64-channel stage with their trained-like weights on the oracle's own inputs: within 3 x the
    direct-order model's rms at every dilation"""
    folded, inp = trained_like
    stage, C, k = 2, 64, 3
    for m, d in enumerate((1, 3, 5)):
        p = f"resblocks.{3 * stage}"
        w1, b1 = folded[f"{p}.convs1.{m}.weight"].numpy(), folded[f"{p}.convs1.{m}.bias"].numpy()
        w2, b2 = folded[f"{p}.convs2.{m}.weight"].numpy(), folded[f"{p}.convs2.{m}.bias"].numpy()
        x = np.ascontiguousarray(inp[f"{p}.convs1.{m}"])
        assert x.shape[0] == C and x.shape[1] >= 1000 and w1.shape == (C, C, k)
        ef, ed, sig = _rms_errors(x, w1, b1, w2, b2, d, _conv_f23)
        print(f"C={C} k={k} d={d} trained-like: F(2,3) rms {ef:.2e}, direct order {ed:.2e}, ratio {ef / ed:.2f} (signal {sig:.3g})")
        assert ef <= 3.0 * ed, (d, ef, ed)
