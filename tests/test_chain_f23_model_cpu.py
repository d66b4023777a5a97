"""The one-launch F(2,3) chains of the k = 3 ResBlocks (reschain32_f23_kernel, reschain16_f23_kernel), checked without a GPU: the
geometry restated in tests/chain_model.py against dissc_chain_info, ownership and the valid ranges; the numpy model of the kernels
(tile by tile, NaN where a kernel's LDS is stale) against float64 and a direct-order fp32 model on the data of
tests/test_gpu_chain_f23.py, inside that test's bars; and three seeded defects, which must miss them."""
import ctypes

import numpy as np
import pytest

import chain_model as cm


def _np(x, w6, b6, i, n):
    return x[i, :, :n].numpy(), [w.numpy() for w in w6], [b.numpy() for b in b6]


@pytest.mark.parametrize("C", [32, 16])
def test_geometry_is_what_the_library_reports(C):
    from dissc_amd import _lib
    g = cm.geo(C)
    info = _lib.DisscChainInfo()
    assert _lib.lib.dissc_chain_info(C, 3, (ctypes.c_int32 * 3)(*cm.DILS), ctypes.byref(info)) == 0
    assert (info.wout, info.span, info.halo, info.lds_bytes, info.tiles_per_wave) == (g.wout, g.span, g.halo, 4 * C * g.xw, g.tiles_per_wave)
    assert g.wout % 4 == 0 and g.span - g.wout == 2 * g.halo and g.halo == 2 + 4 + 6
    for shape in ((64, 3, (1, 3, 5)), (32, 7, (1, 3, 5)), (16, 3, (1, 3, 3)), (8, 3, (1, 3, 5))):
        assert _lib.lib.dissc_chain_info(shape[0], shape[1], (ctypes.c_int32 * 3)(*shape[2]), ctypes.byref(info)) != 0, shape


@pytest.mark.parametrize("C", [32, 16])
def test_every_output_has_one_owner_and_each_pair_covers_the_next(C):
    """for every L in 1 .. 3 WOUT + 13 each output is owned by exactly one tile; every read stays inside the LDS row; each pair's
    valid range covers what the next pair reads of it, down to the owned outputs; a halo of 11 would not"""
    g = cm.geo(C)
    for L in range(1, 3 * g.wout + 14):
        own = cm.owners(L, g)
        assert all(len(o) == 1 for o in own), L
    ranges, in_row = cm.valid_ranges(g)
    assert in_row
    for m, d in enumerate(cm.DILS):
        (a0, b0), (a1, b1) = ranges[m], ranges[m + 1]
        # x_m+1 at p reads T_m at p - 1 .. p + 1, which reads x_m at p - 1 - d .. p + 1 + d
        assert a1 - 1 - d >= a0 and b1 + d + 1 <= b0 and 0 <= a1 < b1 <= g.span, (m, ranges)
        # conv_d's columns cover the T positions the valid x_m+1 reads
        assert g.t0[m] <= a1 - 1 and b1 + 1 <= g.t0[m] + 2 * g.nc1[m], (m, ranges)
    assert ranges[3][0] <= g.halo and g.halo + g.wout <= ranges[3][1], ranges
    a11, b11 = cm.valid_ranges(cm.geo(C, halo=11))[0][3]
    assert not (a11 <= 11 and 11 + cm.geo(C, halo=11).wout <= b11)


@pytest.mark.parametrize("C", [32, 16])
def test_model_stays_inside_the_gpu_tests_bars_on_its_data(C):
    """the GPU test's rows whose tiles differ in kind (one tile, the tile's edges, two tiles and a bit, the wave's owned span, the
    shortest) in the kernels' arithmetic against float64, next to the direct-order fp32 model in the place of the three launches:
    the figures of the GPU test's two bars, per row; and the tiled model equals the untiled F(2,3) chain to rounding"""
    g = cm.geo(C)
    lengths = cm.lengths_for(C)
    x, w6, b6 = cm.data(C, lengths, cm.LD, seed=2300 + C)
    rows = [i for i, n in enumerate(lengths) if n in (1, 2, 13, 25, g.wout - 1, g.wout, g.wout + 1, g.wout + 13, 2 * g.wout + 1, 2 * g.ncols // 4 - g.halo)]
    rows = [0] + rows  # (row 0 = 2000 samples: the rms bar's row)
    worst = worst_d = rms = rms_d = 0.0
    for i in rows:
        xn, w, b = _np(x, w6, b6, i, lengths[i])
        ref = cm.chain_f64(xn, w, b)
        yt, yd = cm.chain_tiled(xn, w, b), cm.chain_direct32(xn, w, b)
        assert yt.dtype == np.float32 and np.isfinite(yt).all(), (i, lengths[i])
        err = (float(np.abs(yt - ref).max()), float(np.sqrt(np.mean((yt - ref) ** 2))))
        base = (float(np.abs(yd - ref).max()), float(np.sqrt(np.mean((yd - ref) ** 2))))
        print(f"C={C} L={lengths[i]}: chain model max {err[0]:.2e} rms {err[1]:.2e}; direct order {base[0]:.2e} / {base[1]:.2e}")
        worst, worst_d = max(worst, err[0]), max(worst_d, base[0])
        if i == 0:
            rms, rms_d = err[1], base[1]
        assert float(np.abs(yt - cm.chain_plain(xn, w, b, cm.conv_f23)).max()) <= 2e-6
    # the GPU test's bars as it takes them: the max over every row, the rms on row 0; the direct-order model stands for mode 0
    print(f"C={C}: max over the rows {worst:.2e} against {worst_d:.2e}, rms of row 0 {rms:.2e} against {rms_d:.2e}")
    assert cm.within_bars((worst, rms), (worst_d, rms_d))


@pytest.mark.parametrize("defect", ["x_not_zeroed", "halo11", "res_activated"])
@pytest.mark.parametrize("C", [32, 16])
def test_seeded_defects_miss_the_bars(C, defect):
    """an x_k not zeroed beyond the utterance, a halo of 11 instead of 12, a residual taken from the activated value: each leaves
    the bars (NaN counts as a miss: the GPU test feeds NaN beyond every length and asks for finite outputs)"""
    g = cm.geo(C)
    n = g.wout + 13
    lengths = cm.lengths_for(C)
    x, w6, b6 = cm.data(C, lengths, cm.LD, seed=2300 + C)
    xn, w, b = _np(x, w6, b6, lengths.index(n), n)
    ref = cm.chain_f64(xn, w, b)
    yd = cm.chain_direct32(xn, w, b)
    base = (float(np.abs(yd - ref).max()), float(np.sqrt(np.mean((yd - ref) ** 2))))
    good = cm.chain_tiled(xn, w, b)
    assert cm.within_bars((float(np.abs(good - ref).max()), float(np.sqrt(np.mean((good - ref) ** 2)))), base)
    bad = cm.chain_tiled(xn, w, b, defect=defect)
    err = (float(np.abs(bad - ref).max()), float(np.sqrt(np.mean((bad - ref) ** 2))))
    print(f"C={C} {defect}: max {err[0]:.2e} rms {err[1]:.2e} against the bars' base {base[0]:.2e} / {base[1]:.2e}")
    assert not (np.isfinite(bad).all() and cm.within_bars(err, base)), (defect, err, base)
