"""The one-launch register-only F(2,3) residual pairs of the 64-channel stage (respair64_f23_kernel in respair_f23.hip; k = 3,
d = 1 / 3 / 5) through the C ABI (dissc_respair1d, mode 3 under "pair_f23" / "pair_f23_c64"): against a float64 torch evaluation,
the two direct launches (mode 0) and the two conv_wino launches it replaces (mode 2); ragged lengths around a wave's 64 outputs
and each instance's own tile, a sentinel beyond every utterance, batch independence, all epilogue modes; the trained-like bars
of tests/test_gpu_trained_like.py; and the whole generator under the default plan against "pair_f23_c64" = 0.
Run with -s for the measured figures."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import test_gpu_trained_like as ttl
from conftest import is_experimental_build
from test_gpu_generator import FP32_GUARD_RMS, _generator_with, _pair_cases, _rms
from test_gpu_pairs_f23 import DEV, F23_DEFAULT, _data, _pair, _reference
from test_gpu_trained_like import tl  # noqa: F401  (its module fixture: trained-like checkpoint and the float64 oracle's layer taps)

pytestmark = pytest.mark.gpu
C64_DEFAULT = 1  # the "pair_f23_c64" value the library ships with
TILE = {1: 252, 3: 248, 5: 248}  # outputs a workgroup owns (F23Geo64::WOUT), per dilation
C, K = 64, 3


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dissc_amd import _lib
    return _lib


def _set(lib, f23, c64):
    assert lib.lib.dissc_set_option(b"pair_f23", f23) == 0
    assert lib.lib.dissc_set_option(b"pair_f23_c64", c64) == 0


@pytest.fixture
def c64(lib):
    """mode 3 of dissc_respair1d builds respair64_f23_kernel at C = 64, k = 3; the shipped values are restored afterwards"""
    _set(lib, F23_DEFAULT, 1)
    yield
    _set(lib, F23_DEFAULT, C64_DEFAULT)


def test_the_library_ships_the_values_this_file_restores(lib):
    for key, want in ((b"pair_f23", F23_DEFAULT), (b"pair_f23_c64", C64_DEFAULT)):
        v = ctypes.c_int(-1)
        assert lib.lib.dissc_get_option(key, ctypes.byref(v)) == 0 and v.value == want, (key, v.value)


@pytest.mark.parametrize("d", [1, 3, 5])
def test_c64_f23_pair_matches_float64_and_the_direct_launches(lib, c64, d):
    """lengths: a 1-sample utterance, ends inside a quad (7, 63, 65, ...), a wave's 64-output boundary - 1 / 0 / + 1 and the
    next one, the instance's own tile - 1 / 0 / + 1 and 2 x tile +- 1.  The bars are those of
    tests/test_gpu_pairs_tc6.py::_check_pair: max error <= 1e-5, rms <= max(3 x the direct path's, 1e-6)"""
    t = TILE[d]
    lengths = [2000, 1, 7, 12, 63, 64, 65, 127, 128, 129, t - 1, t, t + 1, 2 * t - 1, 2 * t + 1, 255, 1023, 1999]
    ld = 2000
    x, w1, b1, w2, b2 = _data(C, K, lengths, ld, seed=6400 + d)
    ref = _reference(x, w1, b1, w2, b2, lengths, K, d)
    y3 = _pair(lib, 3, x, w1, b1, w2, b2, lengths, K, d)
    y0 = _pair(lib, 0, x, w1, b1, w2, b2, lengths, K, d)  # two direct launches
    y2 = _pair(lib, 2, x, w1, b1, w2, b2, lengths, K, d)  # two conv_wino launches
    worst3 = worst0 = 0.0
    for i, n in enumerate(lengths):
        assert torch.isfinite(y3[i, :, :n]).all(), (i, n)
        assert (y3[i, :, n:] == -7.0).all(), f"utterance {i}: wrote beyond its {n} samples"
        worst3 = max(worst3, (y3[i, :, :n].double() - ref[i, :, :n]).abs().max().item())
        worst0 = max(worst0, (y0[i, :, :n].double() - ref[i, :, :n]).abs().max().item())
    r3 = float(((y3[0, :, :2000].double() - ref[0]) ** 2).mean().sqrt())
    r0 = float(((y0[0, :, :2000].double() - ref[0]) ** 2).mean().sqrt())
    print(f"C={C} k={K} d={d}: F(2,3) pair max err {worst3:.2e} rms {r3:.2e}; direct launches {worst0:.2e} / {r0:.2e}")
    assert not torch.equal(y3[0], y2[0])  # (the new kernel really ran, not the two transform-domain launches)
    assert not torch.equal(y3[0], y0[0])
    assert worst3 <= 1e-5 and r3 <= max(3.0 * r0, 1e-6)
    for i in (1, 3, 5, 11, len(lengths) - 2):
        one = _pair(lib, 3, x[i:i + 1].clone(), w1, b1, w2, b2, lengths[i:i + 1], K, d)
        assert torch.equal(one[0, :, :lengths[i]], y3[i, :, :lengths[i]]), i
    acc0 = torch.rand(len(lengths), C, ld, device=DEV)
    for epi in (2, 3, 4):
        a = _pair(lib, 3, x, w1, b1, w2, b2, lengths, K, d, epi=epi, acc=acc0)
        for i, n in enumerate(lengths):
            want = y3[i, :, :n] if epi == 2 else acc0[i, :, :n] + y3[i, :, :n]
            if epi == 4:
                want = (want.cpu() / 3.0).to(DEV)
            assert torch.equal(a[i, :, :n], want), (epi, i)
            assert torch.equal(a[i, :, n:], acc0[i, :, n:])


@pytest.mark.parametrize("f23,c64v", [(0, 1), (F23_DEFAULT, 0)])
def test_either_switch_leaves_mode_3_without_an_instance(lib, f23, c64v):
    """"pair_f23" = 0 (no register-only transform-domain pair anywhere) and "pair_f23_c64" = 0 each: mode 3 has no register-only
    form at C = 64 and nothing is written"""
    lengths = [64]
    x, w1, b1, w2, b2 = _data(C, K, lengths, 64, seed=3)
    try:
        _set(lib, f23, c64v)
        y = torch.full_like(x, -7.0)
        ln = torch.as_tensor(lengths, dtype=torch.int32, device=DEV)
        rc = lib.lib.dissc_respair1d(x.data_ptr(), w1.contiguous().data_ptr(), b1.data_ptr(), w2.contiguous().data_ptr(),
                                     b2.data_ptr(), y.data_ptr(), None, ln.data_ptr(), 1, C, K, 1, 64, 64, ctypes.c_float(0.1),
                                     1, ctypes.c_float(3.0), 3, None)
        # (DISSC_EXPERIMENTAL=1 builds carry the F(4,3) pair kernel, which mode 3 then builds for this shape)
        assert (rc != 0) == (not is_experimental_build())
        assert rc == 0 or (y == -7.0).all()
    finally:
        _set(lib, F23_DEFAULT, C64_DEFAULT)


# ------------------------------------------------------------------------------------------------------------------------
# the trained-like bars (tests/test_gpu_trained_like.py: TD_RMS = 3 x the direct launches' e_rms, TD_CH, LEAK)
# ------------------------------------------------------------------------------------------------------------------------
def test_trained_like_c64_pairs(tl, c64):
    """the three k = 3 pairs of the 64-channel stage on their float64-oracle inputs and the adversarial rows (bursts after
    silence at every offset modulo the unit widths 2 and 2 d, spikes, ragged lengths around the tile)"""
    folded = tl["folded"]
    stage, j = 2, 0
    bad = []
    for m, d in enumerate(ttl.DILS):
        p = f"resblocks.{3 * stage + j}"
        w1, b1 = folded[f"{p}.convs1.{m}.weight"], folded[f"{p}.convs1.{m}.bias"]
        w2, b2 = folded[f"{p}.convs2.{m}.weight"], folded[f"{p}.convs2.{m}.bias"]
        forms = [("direct", 0), ("F(2,3)", 3)]
        tap = tl["inp"][f"{p}.convs1.{m}"]
        adv = ttl._adversarial_rows(tap, [2, 2 * d], seed=6400 + m)
        t = TILE[d]
        rows = [(tap, None)] + adv + [(tap[:, c0:c0 + ln].clone(), None) for c0, ln in ((0, t - 1), (5, t), (9, t + 1), (2, 2 * t + 1))]
        x, lens = ttl._batch(rows)
        pad = (K - 1) * d // 2 + (K - 1) // 2
        unit = F.leaky_relu(x, ttl.SLOPE).abs().amax((1, 2))
        s1 = float(w1.double().abs().sum((1, 2)).max())
        wsum = w2.double().abs().sum((1, 2)) * s1
        refs = [ttl._ref_pair(x[i, :, :n], w1, b1, w2, b2, K, d, torch.float64) for i, n in enumerate(lens)]
        cpu = [ttl._ref_pair(x[i, :, :n], w1, b1, w2, b2, K, d, torch.float32) for i, n in enumerate(lens)]
        res, outs = {}, {}
        for form, mode in [("cpu", -1)] + forms:
            acc_a, acc_b = ttl._Acc(C), ttl._Acc(C)
            if form == "cpu":
                y = cpu
            else:
                yb = ttl._pair(tl, mode, x, w1, b1, w2, b2, lens, K, d)
                outs[form] = yb
                for i, n in enumerate(lens):
                    assert (yb[i, :, n:] == -7.0).all(), (p, m, form, i, "wrote beyond the utterance")
                    assert torch.isfinite(yb[i, :, :n]).all(), (p, m, form, i)
                y = [yb[i, :, :n] for i, n in enumerate(lens)]
            for i, (r, loud) in enumerate(rows):
                if i == 0:
                    acc_a.add(y[i], refs[i])
                else:
                    acc_b.add(y[i], refs[i], loud, pad, float(unit[i]) * wsum * ttl.U)
            res[form] = (acc_a.metrics(), acc_b.metrics())
        # e_rms <= 3 x holds whether or not the form is the default: it is passed as the plan's form
        bad += ttl._check(f"{p}.pair{m}", [f[0] for f in forms], res, "F(2,3)")
        assert not torch.equal(outs["F(2,3)"], outs["direct"])
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
    if C64_DEFAULT:
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
