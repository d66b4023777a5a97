"""The six-point Toom-Cook form of the k = 7 / 11 residual pairs of the 64-channel stage (respair64_tc6_kernel, respair_f23.hip),
checked without a GPU: the numpy model of tests/tc6_model.py (the kernel's fp32 arithmetic: ascending 16-channel chunks, then
sub-filter, then channel; one rounding per fused multiply-add) at C = 64 against float64, next to the direct-order fp32 model of the
same pair.  The bar is the project's 3 x the direct-order model's rms error."""
import numpy as np
import pytest

from tc6_model import _conv_tc6, _rms_errors, trained_like  # noqa: F401  (its module fixture: the trained-like checkpoint)

C = 64


@pytest.mark.parametrize("k", [7, 11])
@pytest.mark.parametrize("d", [1, 3, 5])
def test_c64_six_point_pair_model_on_uniform_data(k, d):
    """data and weights as pair_harness.data (uniform, weights scaled 0.9 / sqrt(C k)), L = 1000"""
    rs = np.random.RandomState(100 * C + 10 * k + d)
    L, sc = 1000, 0.9 / (C * k) ** 0.5
    x = (rs.rand(C, L) * 2 - 1).astype(np.float32)
    w1, w2 = [((rs.rand(C, C, k) * 2 - 1) * sc).astype(np.float32) for _ in range(2)]
    b1, b2 = [((rs.rand(C) * 2 - 1) * 0.1).astype(np.float32) for _ in range(2)]
    e6, ed, _ = _rms_errors(x, w1, b1, w2, b2, d, _conv_tc6)
    print(f"C={C} k={k} d={d} uniform: six-point rms {e6:.2e}, direct order {ed:.2e}, ratio {e6 / ed:.2f}")
    assert e6 <= 3.0 * ed


@pytest.mark.parametrize("k", [7, 11])
def test_c64_six_point_pair_model_on_trained_like_draws(trained_like, k):  # noqa: F811
    """resblocks.7 (k = 7) / resblocks.8 (k = 11) with their trained-like weights on the oracle's own inputs (16 frames: 1 280
    columns): within 3 x the direct-order model's rms at every dilation"""
    folded, inp = trained_like
    p = f"resblocks.{6 + (3, 7, 11).index(k)}"
    for m, d in enumerate((1, 3, 5)):
        w1, b1 = folded[f"{p}.convs1.{m}.weight"].numpy(), folded[f"{p}.convs1.{m}.bias"].numpy()
        w2, b2 = folded[f"{p}.convs2.{m}.weight"].numpy(), folded[f"{p}.convs2.{m}.bias"].numpy()
        x = np.ascontiguousarray(inp[f"{p}.convs1.{m}"])
        assert x.shape == (C, 1280) and w1.shape == (C, C, k)
        e6, ed, sig = _rms_errors(x, w1, b1, w2, b2, d, _conv_tc6)
        print(f"C={C} k={k} d={d} trained-like: six-point rms {e6:.2e}, direct order {ed:.2e}, ratio {e6 / ed:.2f} (signal {sig:.3g})")
        assert e6 <= 3.0 * ed, (d, e6, ed)
