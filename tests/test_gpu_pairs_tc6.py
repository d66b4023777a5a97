"""The register-only six-point Toom-Cook residual pairs (respair32_tc6_kernel in respair_f23.hip: the points 0, +-1, +-2, inf used as
F(3,4); k = 7 and 11 at C = 32) through the C ABI (dissc_respair1d, mode 3 under "pair_f23" / "pair_tc6"): against a float64 torch
evaluation and the direct fused pair; ragged lengths around each instance's own tile, NaN beyond every utterance, all epilogue
modes; the trained-like bars of tests/test_gpu_trained_like.py; the F(2,3) kernels once more under "pair_tc6" = 0; and the whole
generator under the default plan against the direct pairs.  Run with -s for the measured figures."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import test_gpu_trained_like as ttl
from conftest import is_experimental_build
from test_gpu_generator import _generator_with, _pair_cases
from test_gpu_pairs_f23 import DEV, F23_DEFAULT, _data, _pair, _reference
from test_gpu_trained_like import tl  # noqa: F401  (its module fixture: trained-like checkpoint and the float64 oracle's layer taps)

pytestmark = pytest.mark.gpu
TC6_DEFAULT = 3  # the "pair_tc6" mask the library ships with (1: C = 32 k = 7, 2: C = 32 k = 11, 4 / 8: the same at C = 16)
TC6_BUILT = 3    # the shapes with an instance
# outputs a workgroup owns (Tc6Geo::WOUT), per (k, d)
TILE = {(7, 1): 376, (7, 3): 372, (7, 5): 352, (11, 1): 360, (11, 3): 360, (11, 5): 348}


def _tc6_bit(C, k):
    return (1 if C == 32 else 4) << (1 if k == 11 else 0)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dissc_amd import _lib
    return _lib


def _set(lib, f23, tc6):
    assert lib.lib.dissc_set_option(b"pair_f23", f23) == 0
    assert lib.lib.dissc_set_option(b"pair_tc6", tc6) == 0


@pytest.fixture
def tc6(lib):
    """mode 3 of dissc_respair1d builds the six-point form for every shape with an instance"""
    _set(lib, 3, 15)
    yield
    _set(lib, F23_DEFAULT, TC6_DEFAULT)


@pytest.fixture
def tc6_off(lib):
    """mode 3 of dissc_respair1d builds the F(2,3) forms"""
    _set(lib, 3, 0)
    yield
    _set(lib, F23_DEFAULT, TC6_DEFAULT)


def test_the_library_ships_the_masks_this_file_restores(lib):
    for key, want in ((b"pair_f23", F23_DEFAULT), (b"pair_tc6", TC6_DEFAULT)):
        v = ctypes.c_int(-1)
        assert lib.lib.dissc_get_option(key, ctypes.byref(v)) == 0 and v.value == want, (key, v.value)


def _check_pair(lib, C, k, d, lengths, seed, what):
    """ragged lengths, NaN beyond every utterance, against float64 and the direct pair (max <= 1e-5, rms <= max(3 x the direct
    pair's, 1e-6)); batch independence; the MRF modes.  Returns the mode-3 output."""
    ld = 2000
    x, w1, b1, w2, b2 = _data(C, k, lengths, ld, seed=seed)
    ref = _reference(x, w1, b1, w2, b2, lengths, k, d)
    y3 = _pair(lib, 3, x, w1, b1, w2, b2, lengths, k, d)
    y1 = _pair(lib, 1, x, w1, b1, w2, b2, lengths, k, d)  # the direct fused pair
    worst3 = worst1 = 0.0
    for i, n in enumerate(lengths):
        assert torch.isfinite(y3[i, :, :n]).all(), (i, n)
        assert (y3[i, :, n:] == -7.0).all(), f"utterance {i}: wrote beyond its {n} samples"
        worst3 = max(worst3, (y3[i, :, :n].double() - ref[i, :, :n]).abs().max().item())
        worst1 = max(worst1, (y1[i, :, :n].double() - ref[i, :, :n]).abs().max().item())
    r3 = float(((y3[0, :, :2000].double() - ref[0]) ** 2).mean().sqrt())
    r1 = float(((y1[0, :, :2000].double() - ref[0]) ** 2).mean().sqrt())
    print(f"C={C} k={k} d={d}: {what} pair max err {worst3:.2e} rms {r3:.2e}; direct pair {worst1:.2e} / {r1:.2e}")
    assert not torch.equal(y3[0], y1[0])  # (a transform-domain kernel really ran)
    assert worst3 <= 1e-5 and r3 <= max(3.0 * r1, 1e-6)
    for i in (3, 5, len(lengths) - 2):
        one = _pair(lib, 3, x[i:i + 1].clone(), w1, b1, w2, b2, lengths[i:i + 1], k, d)
        assert torch.equal(one[0, :, :lengths[i]], y3[i, :, :lengths[i]]), i
    acc0 = torch.rand(len(lengths), C, ld, device=DEV)
    for epi in (2, 3, 4):
        a = _pair(lib, 3, x, w1, b1, w2, b2, lengths, k, d, epi=epi, acc=acc0)
        for i, n in enumerate(lengths):
            want = y3[i, :, :n] if epi == 2 else acc0[i, :, :n] + y3[i, :, :n]
            if epi == 4:
                want = (want.cpu() / 3.0).to(DEV)
            assert torch.equal(a[i, :, :n], want), (epi, i)
            assert torch.equal(a[i, :, n:], acc0[i, :, n:])
    return y3


@pytest.mark.parametrize("C,k,d", [(32, k, d) for k in (7, 11) for d in (1, 3, 5)])
def test_six_point_pair_matches_float64_and_the_direct_pair(lib, tc6, C, k, d):
    """respair32_tc6_kernel: lengths 1, 7 and the instance's own tile - 1 / 0 / + 1 and 2 x tile +- 1 (at k = 11 the odd waves'
    90 outputs start 2 mod 4: the lengths 89 .. 93 and 179 .. 183 end inside and beside the quads two waves share)"""
    t = TILE[(k, d)]
    lengths = [2000, 1, 7, t - 1, t, t + 1, 2 * t - 1, 2 * t + 1, 89, 90, 91, 92, 93, 179, 181, 183, 255, 1023, 1999, 12]
    y6 = _check_pair(lib, C, k, d, lengths, 1900 + d + k, "six-point")
    if k == 11:  # (the F(2,3) kernel of the same shape gives other bits: the six-point one is what ran)
        _set(lib, 3, 0)
        x, w1, b1, w2, b2 = _data(C, k, lengths, 2000, seed=1900 + d + k)
        assert not torch.equal(_pair(lib, 3, x, w1, b1, w2, b2, lengths, k, d)[0], y6[0])


@pytest.mark.parametrize("C,d", [(32, 1), (32, 3), (32, 5), (16, 1), (16, 3), (16, 5)])
def test_f23_pairs_under_pair_tc6_0(lib, tc6_off, C, d):
    """respair32_f23_kernel / respair16_f23_kernel (k = 11: tiles of 500 / 492 / 468 outputs), reached through mode 3 when
    "pair_tc6" leaves the shape alone: the checks of tests/test_gpu_pairs_f23.py"""
    lengths = [2000, 1, 7, 255, 467, 468, 469, 491, 492, 493, 499, 500, 501, 507, 508, 509, 1023, 1999, 12]
    _check_pair(lib, C, 11, d, lengths, 900 + d + 11, "F(2,3)")


def test_pair_tc6_is_honoured_only_under_the_stage_bit_of_pair_f23(lib):
    """"pair_f23" = 0 still means no register-only transform-domain pair at all: mode 3 has no instance then"""
    lengths = [64]
    x, w1, b1, w2, b2 = _data(32, 7, lengths, 64, seed=3)
    try:
        _set(lib, 0, 15)
        y = torch.full_like(x, -7.0)
        ln = torch.as_tensor(lengths, dtype=torch.int32, device=DEV)
        rc = lib.lib.dissc_respair1d(x.data_ptr(), w1.contiguous().data_ptr(), b1.data_ptr(), w2.contiguous().data_ptr(),
                                     b2.data_ptr(), y.data_ptr(), None, ln.data_ptr(), 1, 32, 7, 1, 64, 64, ctypes.c_float(0.1),
                                     1, ctypes.c_float(3.0), 3, None)
        # (DISSC_EXPERIMENTAL=1 builds carry the F(4,3) pair kernel, which mode 3 then builds for this shape)
        assert (rc != 0) == (not is_experimental_build())
        assert rc == 0 or (y == -7.0).all()
    finally:
        _set(lib, F23_DEFAULT, TC6_DEFAULT)


# ------------------------------------------------------------------------------------------------------------------------
# the trained-like bars (tests/test_gpu_trained_like.py: TD_RMS = 3 x the direct kernel's e_rms, TD_CH, LEAK)
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [7, 11])
def test_trained_like_six_point_pairs(tl, tc6, k):
    """every (k, d) of the 32-channel stage with a six-point instance on its float64-oracle input and the adversarial rows
    (bursts after silence at every offset modulo the unit widths 3 d NS, spikes, ragged lengths): TD_CH and LEAK hold for every
    shape; TD_RMS for every shape of the default mask (a shape above it must not be in the mask)"""
    folded = tl["folded"]
    stage, C, j = 3, 32, ttl.KS.index(k)
    ns = (k + 3) // 4
    bad = []
    for m, d in enumerate(ttl.DILS):
        p = f"resblocks.{3 * stage + j}"
        w1, b1 = folded[f"{p}.convs1.{m}.weight"], folded[f"{p}.convs1.{m}.bias"]
        w2, b2 = folded[f"{p}.convs2.{m}.weight"], folded[f"{p}.convs2.{m}.bias"]
        forms = [("direct", 0), ("fused", 1), ("TC6", 3)]
        tap = tl["inp"][f"{p}.convs1.{m}"]
        adv = ttl._adversarial_rows(tap, [3 * ns, 3 * ns * d], seed=7000 + 100 * j + m)
        t = TILE[(k, d)]
        rows = [(tap, None)] + adv + [(tap[:, c0:c0 + ln].clone(), None) for c0, ln in ((0, t - 1), (5, t), (9, t + 1), (2, 2 * t + 1))]
        x, lens = ttl._batch(rows)
        pad = (k - 1) * d // 2 + (k - 1) // 2
        unit = F.leaky_relu(x, ttl.SLOPE).abs().amax((1, 2))
        s1 = float(w1.double().abs().sum((1, 2)).max())
        wsum = w2.double().abs().sum((1, 2)) * s1
        refs = [ttl._ref_pair(x[i, :, :n], w1, b1, w2, b2, k, d, torch.float64) for i, n in enumerate(lens)]
        cpu = [ttl._ref_pair(x[i, :, :n], w1, b1, w2, b2, k, d, torch.float32) for i, n in enumerate(lens)]
        res, outs = {}, {}
        for form, mode in [("cpu", -1)] + forms:
            acc_a, acc_b = ttl._Acc(C), ttl._Acc(C)
            if form == "cpu":
                y = cpu
            else:
                yb = ttl._pair(tl, mode, x, w1, b1, w2, b2, lens, k, d)
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
        in_mask = bool(TC6_DEFAULT & _tc6_bit(C, k))
        bad += ttl._check(f"{p}.pair{m}", [f[0] for f in forms], res, "TC6" if in_mask else None)
        assert not torch.equal(outs["TC6"], outs["direct"])
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
    for bit in (1, 2, 4, 8):
        if TC6_DEFAULT & bit:
            gb = _generator_with(L, synth, pair_tc6=bit)
            assert gb.flops(1000) == gd.flops(1000)
            # k = 7 leaves the direct pair's 7 products per output for 4, k = 11 the F(2,3) pair's 8 for 6
            print(f"pair_tc6={bit}: executed FLOPs per 1000 frames {gb.flops_executed(1000):.4g} (pair_tc6=0: {fx:.4g})")
            assert gb.flops_executed(1000) < fx, bit
    if TC6_DEFAULT & TC6_BUILT:
        assert g.flops_executed(1000) < fx
    for code, f0, spkr, lengths in _pair_cases(synth) + [synth.synth_generator_inputs(3, 1203, seed=5, ragged=True)]:
        kw = dict(code=torch.from_numpy(code), f0=torch.from_numpy(f0), spkr=torch.from_numpy(spkr),
                  lengths=torch.from_numpy(lengths))
        y, yd, y0 = g(**kw).cpu(), gd(**kw).cpu(), g0(**kw).cpu()
        assert torch.isfinite(y).all()
        if TC6_DEFAULT & TC6_BUILT:
            assert not torch.equal(y, y0)  # (the six-point kernels really ran)
        e = (y - yd).double()
        rms = float(e.pow(2).mean().sqrt())
        print(f"B={code.shape[0]} T={code.shape[1]}: default plan vs direct pairs: rms {rms:.2e}, max {float(e.abs().max()):.2e}")
        assert rms <= 2e-6 and float(e.abs().max()) <= 5e-5
        one = g(code=kw["code"][:1], f0=kw["f0"][:1], spkr=kw["spkr"][:1], lengths=kw["lengths"][:1]).cpu()[0]
        assert torch.equal(one, y[0])
