"""YAAPT F0 tracker, CPU side: the oracle restatement on known-F0 signals, and the host
stages of the product (dissc_amd/f0.py: spectral track, candidate merge, final DP -- vectorised numpy) against the
oracle's own versions of the same stages.  PARITY UNPINNED against amfm_decompy (absent offline): what is pinned
is ground truth (synthetic speech-like signals with a known F0) and mutual agreement."""
import os

import numpy as np
import pytest

from oracle import yaapt_ref as yr
from yaapt_cases import CASES, FS, _speech, check_track, pulse_train, speech_track_is_plausible, voiced


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_tracks_known_f0_within_2_percent(name):
    f0 = yr.get_yaapt_f0(voiced(CASES[name]))
    assert len(f0) == 300  # 1.5 s at a 5 ms hop: exactly 4 values per 20 ms unit
    check_track(f0, CASES[name])


def test_oracle_pulse_train_and_voicing_decisions():
    f0 = yr.get_yaapt_f0(pulse_train(140.0, 24000))
    check_track(f0, np.full(24000, 140.0))
    assert not yr.get_yaapt_f0(np.zeros(24000)).any()                         # silence
    assert [yr.get_yaapt_f0(voiced(np.full(n, 150.0))).tolist() for n in (1, 79)] == [[0.0], [0.0]]  # no time-domain frame
    noise = 0.1 * np.random.RandomState(0).standard_normal(24000)
    assert (yr.get_yaapt_f0(noise) > 0).mean() <= 0.1                        # white noise: (almost) all unvoiced
    x = np.concatenate([voiced(np.full(8000, 150.0)), 0.002 * np.random.RandomState(1).standard_normal(8000),
                        voiced(np.full(8000, 220.0))])
    f0 = yr.get_yaapt_f0(x)
    assert np.all(np.abs(f0[10:95] - 150) < 3) and not f0[108:195].any() and np.all(np.abs(f0[210:290] - 220) < 4.4)


def test_f0_per_unit_alignment():
    f = np.array([0, 100, 0, 110, 0, 0, 0, 0, 200, 200, 200, 200, 50], dtype=float)
    np.testing.assert_allclose(yr.f0_per_unit(f, 3), [105.0, 0.0, 200.0])
    from dissc_amd.f0 import f0_per_unit
    np.testing.assert_allclose(f0_per_unit(f, 3), [105.0, 0.0, 200.0])
    # more units than frames: the track is extended with its last value (textless pads with f0[-1], not zeros)
    np.testing.assert_allclose(f0_per_unit(f, 5), [105.0, 0.0, 200.0, 50.0, 50.0])
    np.testing.assert_allclose(f0_per_unit(f, 5), yr.f0_per_unit(f, 5))
    np.testing.assert_allclose(f0_per_unit(f[:12], 4), [105.0, 0.0, 200.0, 200.0])
    np.testing.assert_allclose(f0_per_unit(np.zeros(0), 2), [0.0, 0.0])


def test_product_host_stages_equal_the_oracle_stages():
    """dissc_amd.f0's vectorised host logic, fed the oracle's own intermediate results, reproduces the oracle's
    spectral track, candidate table and final track (float64, tie-free data -> exact up to rounding)."""
    from dissc_amd import f0 as prod
    p = yr.PARAMS
    x = np.concatenate([voiced(np.linspace(110, 180, 16000)), 0.002 * np.random.RandomState(3).standard_normal(4000),
                        voiced(np.full(12000, 240.0))])
    y = np.pad(x, (160, 160))
    filt, nl = yr.bandpass(y, FS), yr.bandpass(y * y, FS)
    energy, vuv = yr.nlfer(filt, FS)
    # SHC candidates per frame exactly as the oracle forms them
    nframe, njump, samples = yr.frame_geometry(len(nl), FS)
    F = len(samples)
    cand_p, cand_m = np.zeros((4, F)), np.ones((4, F))
    data = np.append(nl, np.zeros(2 * nframe + (F - 1) * njump - len(nl)))
    win = yr.kaiser(2 * nframe, 0.5)
    for f in np.nonzero(vuv)[0]:
        s = data[f * njump:f * njump + 2 * nframe] * win
        shc = yr.shc_of_magnitude(np.abs(np.fft.rfft(s - s.mean(), 8192)), FS)
        cand_p[:, f], cand_m[:, f] = yr.peaks(shc, FS / 8192.0, 4)
    spec_o, std_o, _ = yr.spec_track_from_candidates(cand_p, cand_m)
    spec_p, std_p = prod.spectral_track(cand_p, cand_m, prod.DEFAULTS)
    np.testing.assert_allclose(spec_p, spec_o, rtol=1e-12)
    assert abs(std_p - std_o) <= 1e-12 * std_o
    lo_o, hi_o = yr.lag_ranges(spec_o, std_o, FS)
    lo_p, hi_p = prod.lag_ranges(spec_o, std_o, FS, prod.DEFAULTS)
    np.testing.assert_array_equal(lo_o, lo_p)
    np.testing.assert_array_equal(hi_o, hi_p)
    # NCCF candidates (before the merit reshaping, which the product folds into merge_candidates)
    n, hop, nfr = yr.tda_geometry(len(filt), FS, F)
    raw = []
    for sig in (filt, nl):
        pit, mer = np.zeros((3, nfr)), np.zeros((3, nfr))
        for f in range(nfr):
            phi = yr.crs_corr(sig[f * hop:f * hop + n], int(lo_o[f]), int(hi_o[f]))
            pit[:, f], mer[:, f] = yr.cmp_rate(phi, FS, 3, int(lo_o[f]), int(hi_o[f]))
        raw.append((pit, mer))
    resh = [yr.reshape_merit(pit, mer, spec_o[:nfr], std_o) for pit, mer in raw]
    rp_o, rm_o = yr.refine(resh[0][0], resh[0][1], resh[1][0], resh[1][1], spec_o, energy, vuv)
    rp_p, rm_p = prod.merge_candidates(raw[0][0], raw[0][1], raw[1][0], raw[1][1], spec_o, std_o, energy, vuv,
                                       prod.DEFAULTS)
    np.testing.assert_allclose(rp_p, rp_o, rtol=1e-12)
    np.testing.assert_allclose(rm_p, rm_o, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(prod.final_track(rp_o, rm_o, energy, prod.DEFAULTS), yr.dynamic(rp_o, rm_o, energy),
                               rtol=1e-12)
    assert prod.DEFAULTS == {k: v for k, v in p.items() if k != "dec_factor"}


@pytest.mark.parametrize("name", ["s1_1", "s1_2"])
def test_oracle_on_the_reference_speech_fixtures(name):
    """the reference's own speech fixtures through the restatement: a plausible track, and the committed copy of it
    (tests/golden/yaapt_speech.npz, written by make_yaapt_tracks.py from this same oracle) shows drift"""
    f0 = yr.get_yaapt_f0(_speech(name))
    assert len(f0) == 400
    speech_track_is_plausible(f0, name)
    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "yaapt_speech.npz"))[name]
    assert ((f0 > 0) == (want > 0)).mean() >= 0.995
    both = (f0 > 0) & (want > 0)
    assert np.abs(f0[both] - want[both]).max() <= 1e-3 * want[both].max()
    per_unit = yr.f0_per_unit(f0, 99)
    assert np.isfinite(per_unit).all() and (per_unit > 0).mean() >= 0.5
