"""The one-launch register-only six-point residual pairs of the 64-channel stage (respair64_tc6_kernel in respair_f23.hip; k = 7 / 11,
d = 1 / 3 / 5; a column tile's two 32-row blocks on a wave pair) through the C ABI (dissc_respair1d mode 3 under "pair_tc6_c64"): the
checks of pair_harness.check_pair against the two direct launches (mode 0) around a wave's conv_1 range and each instance's own
tile, per row over all 64 rows, and other bits than the two transform-domain launches the pair replaces (mode 4); the trained-like
bars of tests/test_gpu_trained_like.py; and the whole generator with the option set against the option cleared.  Every test sets
the option itself and puts the library's value back (pair_harness.options restores only its own keys).  Run with -s for the
measured figures."""
import ctypes

import pytest
import torch

import pair_harness as ph
import trained_like_cases as ttl
from generator_cases import FP32_GUARD_RMS, _generator_with, _pair_cases, _rms
from trained_like_cases import tl  # noqa: F401  (its module fixture: trained-like checkpoint and the float64 oracle's layer taps)

pytestmark = pytest.mark.gpu
C = 64
SIX = ph.Form("six-point", 3, {"pair_tc6_c64": 3}, ph.TC6)
# the ends beside a wave's conv_1 range (96 outputs at k = 7, 90 at k = 11: the second column tile starts 2 mod 4 there)
WAVE_EDGES = [89, 90, 91, 92, 93, 95, 96, 97, 179, 180, 181, 182, 183, 191, 192, 193]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dissc_amd import _lib
    return _lib


@pytest.fixture(autouse=True)
def restore_pair_tc6_c64():
    from dissc_amd import _lib
    was = ctypes.c_int(-1)
    assert _lib.lib.dissc_get_option(b"pair_tc6_c64", ctypes.byref(was)) == 0
    yield
    assert _lib.lib.dissc_set_option(b"pair_tc6_c64", was.value) == 0


@pytest.mark.parametrize("k,d", [(k, d) for k in (7, 11) for d in (1, 3, 5)])
def test_c64_six_point_pair_matches_float64_and_the_direct_launches(lib, k, d):
    """lengths: 1, 7 and 12 samples, the ends beside a wave's conv_1 range, the instance's own tile edges, 255 / 1 023 / 1 999;
    rows alone against the same rows in the batch; EPI_RES and the three MRF epilogues; nothing beyond a length (check_pair).
    Then every one of the 64 rows against float64 on its own (both 32-row blocks: each belongs to another wave), and other
    bits than mode 4's"""
    lengths = [2000, 1, 7, 12] + WAVE_EDGES + ph.edge_lengths(ph.form_tile(lib, SIX, C, k, d)) + [255, 1023, 1999]
    seed = 6400 + 10 * k + d
    y6 = ph.check_pair(lib, SIX, ph.DIRECT_LAUNCHES, C, k, d, lengths, seed, alone=(1, 3, 5, 11, 21, len(lengths) - 2))
    x, w1, b1, w2, b2 = ph.data(C, k, lengths, 2000, seed=seed)
    ref = ph.reference(x, w1, b1, w2, b2, lengths, k, d)
    yd = ph.run_form(lib, ph.DIRECT_LAUNCHES, x, w1, b1, w2, b2, lengths, k, d)
    for i, n in enumerate(lengths):
        e = (y6[i, :, :n].double() - ref[i, :, :n]).abs().amax(1)
        assert e.shape == (C,) and float(e.max()) <= 1e-5, (i, n, int(e.argmax()), float(e.max()))
    row6 = (y6[0].double() - ref[0]).pow(2).mean(1).sqrt()
    rowd = (yd[0].double() - ref[0]).pow(2).mean(1).sqrt()
    print(f"C={C} k={k} d={d}: per-row rms six-point {float(row6.min()):.2e} .. {float(row6.max()):.2e}, "
          f"direct {float(rowd.min()):.2e} .. {float(rowd.max()):.2e}")
    assert (row6 <= torch.clamp(3.0 * rowd, min=1e-6)).all(), (row6 / rowd).tolist()
    y4 = ph.run_pair(lib, 4, x, w1, b1, w2, b2, lengths, k, d)  # the two transform-domain launches of the plan
    for i, n in enumerate(lengths):
        assert (y4[i, :, :n].double() - ref[i, :, :n]).abs().max().item() <= 1e-5, (i, n)
    assert not torch.equal(y6[0], y4[0])  # (the new kernel really ran)


@pytest.mark.parametrize("f23,mask", [(0, 3), (ph.SHIPPED["pair_f23"], 0)])
def test_either_switch_leaves_mode_3_without_an_instance(lib, f23, mask):
    for k in (7, 11):
        ph.assert_no_instance(lib, C, k, dict(pair_f23=f23, pair_tc6_c64=mask))


@pytest.mark.parametrize("k", [7, 11])
def test_trained_like_c64_six_point_pairs(tl, k):  # noqa: F811
    """the three pairs of resblocks.7 (k = 7) / resblocks.8 (k = 11) on their float64-oracle inputs, the adversarial rows (unit
    widths 3 NS and 3 NS d) and windows of the tap around the instance's tile: TD_RMS, TD_CH and LEAK hold for the form"""
    j, ns = ttl.KS.index(k), (k + 3) // 4
    six = ph.Form("TC6", 3, SIX.options, ph.TC6)
    bad = []
    for m, d in enumerate(ttl.DILS):
        t = ph.form_tile(tl["_lib"], six, C, k, d)
        bad += ph.trained_like_pair_layer(tl, C, k, d, f"resblocks.{6 + j}", m, [ph.TL_DIRECT, six], "TC6", [3 * ns, 3 * ns * d],
                                          6500 + 100 * j + m, ph.tile_windows(t))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------
# the whole generator
# ------------------------------------------------------------------------------------------------------------------------
def _td_macs(form, k):
    """products per output and C^2 of one transform-domain conv launch (conv_wino.hip, conv_wino8.hip)"""
    return {"F(4,3)": 6.0 * ((k + 2) // 3) / 4.0, "F(6,3)": 8.0 * ((k + 2) // 3) / 6.0, "F(5,4)": 8.0 * ((k + 3) // 4) / 5.0}[form]


def test_generator_with_c64_six_point_pairs_agrees_with_the_two_launch_plan(lib):
    """a handle with "pair_tc6_c64" = 3 (the k = 7 / 11 chains of the 64-channel stage as three one-launch pairs each) against
    one built with "pair_tc6_c64" = 0: same waveform to fp32 rounding, the algorithmic FLOPs equal, the executed ones differing
    by the plan's own count (2 C^2 ceil(k / 4) products per output and conv against the two launches' forms), batch-independent
    samples, and the fp32 parity guard against the float64 oracle"""
    import synthdata as synth
    from oracle import generator_ref as gr
    L = lib.lib
    g = _generator_with(L, synth, pair_tc6_c64=3)
    g0 = _generator_with(L, synth, pair_tc6_c64=0)
    assert g.flops(1000) == g0.flops(1000)
    mul = 5 * 4 * 4  # samples of the 64-channel stage per frame (VCTK upsample rates 5, 4, 4, 2, 2)
    assert synth.VCTK_CONFIG["upsample_rates"][:3] == [5, 4, 4]
    want = 0.0
    for k in (7, 11):
        for d in ttl.DILS:
            old = _td_macs(ttl._plan_conv_form(L, C, k, d), k) + _td_macs(ttl._plan_conv_form(L, C, k, 1), k)
            want += 2.0 * 1000 * mul * C * C * (2 * 2.0 * ((k + 3) // 4) - old)
    got = g.flops_executed(1000) - g0.flops_executed(1000)
    print(f"executed FLOPs per 1000 frames: {g.flops_executed(1000):.6g} against {g0.flops_executed(1000):.6g}")
    assert abs(got - want) <= 1e-9 * g.flops_executed(1000), (got, want)
    folded64 = gr.to_double(gr.fold_state_dict(synth.synth_generator_state_dict(seed=0)))
    code, f0, spkr, lengths = _pair_cases(synth)[0]
    for code, f0, spkr, lengths in [(code, f0, spkr, lengths), synth.synth_generator_inputs(3, 1203, seed=5, ragged=True)]:
        kw = dict(code=torch.from_numpy(code), f0=torch.from_numpy(f0), spkr=torch.from_numpy(spkr),
                  lengths=torch.from_numpy(lengths))
        y, y0 = g(**kw).cpu(), g0(**kw).cpu()
        assert torch.isfinite(y).all()
        assert not torch.equal(y, y0)  # (the new kernels really ran)
        e = (y - y0).double()
        rms = float(e.pow(2).mean().sqrt())
        print(f"B={code.shape[0]} T={code.shape[1]}: six-point c64 pairs vs two launches: rms {rms:.2e}, max {float(e.abs().max()):.2e}")
        assert rms <= 2e-6 and float(e.abs().max()) <= 5e-5
        one = g(code=kw["code"][:1], f0=kw["f0"][:1], spkr=kw["spkr"][:1], lengths=kw["lengths"][:1]).cpu()[0]
        assert torch.equal(one, y[0])
        # the parity guard of the generator tests, on the shortest rows (the float64 oracle runs on the CPU)
        for b in sorted(range(len(lengths)), key=lambda i: int(lengths[i]))[:2]:
            n = int(lengths[b])
            if n == 0:
                continue
            ref = gr.code_generator(folded64, synth.VCTK_CONFIG, code[b:b + 1, :n], f0[b:b + 1, :, :n], spkr[b:b + 1]).numpy()
            err = _rms(y[b:b + 1, :, :320 * n].numpy() - ref)
            print(f"  row {b} ({n} frames): rms against float64 {err:.2e}")
            assert err <= FP32_GUARD_RMS, (b, err)
