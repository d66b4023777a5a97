"""The six-point Toom-Cook form of the narrow residual pairs (respair32_tc6_kernel, respair_f23.hip), checked without a GPU:
the matrices of F(3,4) at the points 0, +-1, +-2, inf in exact rational arithmetic, and a numpy model of a whole pair in the
kernel's fp32 arithmetic (operands rounded to fp32, one rounding per fused multiply-add, the kernel's order of channels,
sub-filters and transform steps; tests/tc6_model.py) against float64, next to a direct-order fp32 model of the same pair.

The host packing (pack_pair_reg: U = G w in double, rounded once) uploads to the device and has no host-only entry, so it is
covered by the GPU tests (tests/test_gpu_pairs_tc6.py); the model below forms U the same way."""
from fractions import Fraction as Fr

import numpy as np
import pytest

from tc6_model import AT, BT, G, _at, _bt, _conv_tc6, _rms_errors, trained_like  # noqa: F401  (trained_like: the module fixture)


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
