"""The one-launch register-only F(2,3) residual pairs of the 64-channel stage (respair64_f23_kernel in respair_f23.hip; k = 3,
d = 1 / 3 / 5) through the C ABI (dissc_respair1d mode 3 under the shipped "pair_f23" / "pair_f23_c64"): the checks of
pair_harness.check_pair against the two direct launches (mode 0), around a wave's 64 outputs and each instance's own tile, and
other bits than the two conv_wino launches it replaces (mode 2); the trained-like bars of tests/test_gpu_trained_like.py; and the
whole generator under the default plan against "pair_f23_c64" = 0.  Run with -s for the measured figures."""
import pytest
import torch

import pair_harness as ph
import trained_like_cases as ttl
from generator_cases import FP32_GUARD_RMS, _generator_with, _pair_cases, _rms
from trained_like_cases import tl  # noqa: F401  (its module fixture: trained-like checkpoint and the float64 oracle's layer taps)

pytestmark = pytest.mark.gpu
C, K = 64, 3
F23 = ph.Form("F(2,3)", 3, {}, ph.F23)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dissc_amd import _lib
    return _lib


@pytest.mark.parametrize("d", [1, 3, 5])
def test_c64_f23_pair_matches_float64_and_the_direct_launches(lib, d):
    """lengths: a 1-sample utterance, ends inside a quad (7, 63, 65, ...), a wave's 64-output boundary - 1 / 0 / + 1 and the
    next one, the instance's own tile edges"""
    lengths = [2000, 1, 7, 12, 63, 64, 65, 127, 128, 129] + ph.edge_lengths(ph.form_tile(lib, F23, C, K, d)) + [255, 1023, 1999]
    y3 = ph.check_pair(lib, F23, ph.DIRECT_LAUNCHES, C, K, d, lengths, 6400 + d, alone=(1, 3, 5, 11, len(lengths) - 2))
    x, w1, b1, w2, b2 = ph.data(C, K, lengths, 2000, seed=6400 + d)
    y2 = ph.run_pair(lib, 2, x, w1, b1, w2, b2, lengths, K, d)  # two conv_wino launches
    assert not torch.equal(y3[0], y2[0])  # (the new kernel really ran, not the two transform-domain launches)


@pytest.mark.parametrize("f23,c64v", [(0, 1), (ph.SHIPPED["pair_f23"], 0)])
def test_either_switch_leaves_mode_3_without_an_instance(lib, f23, c64v):
    """"pair_f23" = 0 (no register-only transform-domain pair anywhere) and "pair_f23_c64" = 0 each: mode 3 has no register-only
    form at C = 64 and nothing is written"""
    ph.assert_no_instance(lib, C, K, dict(pair_f23=f23, pair_f23_c64=c64v))


def test_trained_like_c64_pairs(tl):
    """the three k = 3 pairs of the 64-channel stage on their float64-oracle inputs, the adversarial rows (unit widths 2 and 2 d)
    and windows of the tap around the instance's tile; the form is the shipped plan's: all three bars hold for it"""
    forms = [ph.TL_DIRECT, F23]
    bad = []
    for m, d in enumerate(ttl.DILS):
        t = ph.form_tile(tl["_lib"], F23, C, K, d)
        bad += ph.trained_like_pair_layer(tl, C, K, d, "resblocks.6", m, forms, "F(2,3)", [2, 2 * d], 6400 + m, ph.tile_windows(t))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------
# the whole generator
# ------------------------------------------------------------------------------------------------------------------------
def test_generator_with_c64_pairs_agrees_with_the_two_launch_plan(lib):
    """a handle with "pair_f23_c64" = 1 (the k = 3 chain of the 64-channel stage as three one-launch pairs) against one built
    with "pair_f23_c64" = 0: same waveform to fp32 rounding (the bars of test_f23_pairs_agree_with_the_direct_pairs), the
    algorithmic FLOPs equal, the executed ones higher by 2 C^2 - 1.5 C^2 products per output and conv of the three pairs,
    batch-independent samples, and the fp32 parity guard against the float64 oracle"""
    import synthdata as synth
    from oracle import generator_ref as gr
    L = lib.lib
    g = _generator_with(L, synth, pair_f23_c64=1)
    g0 = _generator_with(L, synth, pair_f23_c64=0)
    assert g.flops(1000) == g0.flops(1000)
    mul = 5 * 4 * 4  # samples of the 64-channel stage per frame (VCTK upsample rates 5, 4, 4, 2, 2)
    assert synth.VCTK_CONFIG["upsample_rates"][:3] == [5, 4, 4]
    want = 2.0 * 1000 * mul * 3 * 2 * (2.0 - 1.5) * C * C
    got = g.flops_executed(1000) - g0.flops_executed(1000)
    print(f"executed FLOPs per 1000 frames: {g.flops_executed(1000):.6g} against {g0.flops_executed(1000):.6g}")
    assert abs(got - want) <= 1e-9 * g.flops_executed(1000), (got, want)
    if ph.SHIPPED["pair_f23_c64"]:
        gdef = _generator_with(L, synth)
        assert gdef.flops_executed(1000) == g.flops_executed(1000)
    folded64 = gr.to_double(gr.fold_state_dict(synth.synth_generator_state_dict(seed=0)))
    code, f0, spkr, lengths = _pair_cases(synth)[0]
    for code, f0, spkr, lengths in [(code, f0, spkr, lengths), synth.synth_generator_inputs(3, 1203, seed=5, ragged=True)]:
        kw = dict(code=torch.from_numpy(code), f0=torch.from_numpy(f0), spkr=torch.from_numpy(spkr),
                  lengths=torch.from_numpy(lengths))
        y, y0 = g(**kw).cpu(), g0(**kw).cpu()
        assert torch.isfinite(y).all()
        assert not torch.equal(y, y0)  # (the new kernel really ran)
        e = (y - y0).double()
        rms = float(e.pow(2).mean().sqrt())
        print(f"B={code.shape[0]} T={code.shape[1]}: c64 pairs vs two launches: rms {rms:.2e}, max {float(e.abs().max()):.2e}")
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
