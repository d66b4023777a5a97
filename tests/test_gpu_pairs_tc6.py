"""The register-only six-point Toom-Cook residual pairs (respair32_tc6_kernel in respair_f23.hip: the points 0, +-1, +-2, inf used as
F(3,4); k = 7 and 11 at C = 32) through the C ABI (dissc_respair1d mode 3 under the shipped "pair_f23" / "pair_tc6"): the checks of
pair_harness.check_pair around each instance's own tile; the trained-like bars of tests/test_gpu_trained_like.py; and the whole
generator under the default plan against the direct pairs.  Run with -s for the measured figures."""
import ctypes

import pytest
import torch

import pair_harness as ph
import trained_like_cases as ttl
from generator_cases import _generator_with, _pair_cases
from trained_like_cases import tl  # noqa: F401  (its module fixture: trained-like checkpoint and the float64 oracle's layer taps)

pytestmark = pytest.mark.gpu
SIX = ph.Form("six-point", 3, {}, ph.TC6)
F23 = ph.Form("F(2,3)", 3, {"pair_tc6": 0}, ph.F23)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dissc_amd import _lib
    return _lib


def test_the_library_ships_the_masks_this_file_restores(lib):
    """pair_harness.options restores pair_harness.SHIPPED after every change: these are the library's own defaults"""
    for key, want in ph.shipped(lib).items():
        v = ctypes.c_int(-1)
        assert lib.lib.dissc_get_option(key.encode(), ctypes.byref(v)) == 0 and v.value == want, (key, v.value)


@pytest.mark.parametrize("C,k,d", [(32, k, d) for k in (7, 11) for d in (1, 3, 5)])
def test_six_point_pair_matches_float64_and_the_direct_pair(lib, C, k, d):
    """lengths 1, 7 and the instance's own tile edges (at k = 11 the odd waves' 90 outputs start 2 mod 4: the lengths 89 .. 93 and
    179 .. 183 end inside and beside the quads two waves share)"""
    lengths = [2000, 1, 7] + ph.edge_lengths(ph.form_tile(lib, SIX, C, k, d)) + [89, 90, 91, 92, 93, 179, 181, 183, 255, 1023, 1999, 12]
    y6 = ph.check_pair(lib, SIX, ph.DIRECT_PAIR, C, k, d, lengths, 1900 + d + k, alone=(3, 5, len(lengths) - 2))
    if k == 11:  # (the F(2,3) kernel of the same shape gives other bits)
        x, w1, b1, w2, b2 = ph.data(C, k, lengths, 2000, seed=1900 + d + k)
        assert not torch.equal(ph.run_form(lib, F23, x, w1, b1, w2, b2, lengths, k, d)[0], y6[0])


def test_pair_tc6_is_honoured_only_under_the_stage_bit_of_pair_f23(lib):
    """"pair_f23" = 0 still means no register-only transform-domain pair at all: mode 3 has no instance then"""
    ph.assert_no_instance(lib, 32, 7, dict(pair_f23=0, pair_tc6=15))


@pytest.mark.parametrize("k", [7, 11])
def test_trained_like_six_point_pairs(tl, k):
    """every (k, d) of the 32-channel stage with a six-point instance on its float64-oracle input, the adversarial rows (unit
    widths 3 NS and 3 NS d) and windows of the tap around the instance's tile: the six-point form is the shipped plan's, so all
    three bars (TD_RMS, TD_CH, LEAK) hold for it"""
    C, j, ns = 32, ttl.KS.index(k), (k + 3) // 4
    forms = [ph.TL_DIRECT, ph.TL_FUSED, ph.Form("TC6", 3, {}, ph.TC6)]
    bad = []
    for m, d in enumerate(ttl.DILS):
        t = ph.form_tile(tl["_lib"], forms[-1], C, k, d)
        bad += ph.trained_like_pair_layer(tl, C, k, d, f"resblocks.{9 + j}", m, forms, "TC6", [3 * ns, 3 * ns * d],
                                          7000 + 100 * j + m, ph.tile_windows(t))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------
# the whole generator
# ------------------------------------------------------------------------------------------------------------------------
def test_default_plan_agrees_with_the_direct_pairs(lib):
    """the default handle (its adopted shapes on respair32_tc6_kernel) against one built with "pair_f23" = 0 (the direct
    pairs): same waveform to fp32 rounding on the ragged cases and at B = 32 x T = 500 (the bars of
    test_f23_pairs_agree_with_the_direct_pairs); every adopted shape lowers the executed FLOPs and none changes the
    algorithmic count; batch-independent samples"""
    import synthdata as synth
    L = lib.lib
    g = _generator_with(L, synth)
    gd = _generator_with(L, synth, pair_f23=0)
    g0 = _generator_with(L, synth, pair_tc6=0)
    assert g.flops(1000) == gd.flops(1000) == g0.flops(1000)
    assert g0.flops_executed(1000) < gd.flops_executed(1000)
    fx = g0.flops_executed(1000)
    six = any(ph.pair_info(lib, 32, k, 1).form == ph.TC6 for k in (7, 11))  # (under the shipped options)
    for bit in (1, 2, 4, 8):
        if ph.SHIPPED["pair_tc6"] & bit:
            gb = _generator_with(L, synth, pair_tc6=bit)
            assert gb.flops(1000) == gd.flops(1000)
            # k = 7 leaves the direct pair's 7 products per output for 4, k = 11 the F(2,3) pair's 8 for 6
            print(f"pair_tc6={bit}: executed FLOPs per 1000 frames {gb.flops_executed(1000):.4g} (pair_tc6=0: {fx:.4g})")
            assert gb.flops_executed(1000) < fx, bit
    if six:
        assert g.flops_executed(1000) < fx
    for code, f0, spkr, lengths in _pair_cases(synth) + [synth.synth_generator_inputs(3, 1203, seed=5, ragged=True)]:
        kw = dict(code=torch.from_numpy(code), f0=torch.from_numpy(f0), spkr=torch.from_numpy(spkr),
                  lengths=torch.from_numpy(lengths))
        y, yd, y0 = g(**kw).cpu(), gd(**kw).cpu(), g0(**kw).cpu()
        assert torch.isfinite(y).all()
        if six:
            assert not torch.equal(y, y0)  # (the six-point kernels really ran)
        e = (y - yd).double()
        rms = float(e.pow(2).mean().sqrt())
        print(f"B={code.shape[0]} T={code.shape[1]}: default plan vs direct pairs: rms {rms:.2e}, max {float(e.abs().max()):.2e}")
        assert rms <= 2e-6 and float(e.abs().max()) <= 5e-5
        one = g(code=kw["code"][:1], f0=kw["f0"][:1], spkr=kw["spkr"][:1], lengths=kw["lengths"][:1]).cpu()[0]
        assert torch.equal(one, y[0])
