"""YAAPT F0 tracker on the GPU (dissc_amd/f0.py + csrc/yaapt.hip through the C ABI) against the CPU restatement
(oracle/yaapt_ref.py) stage by stage, against known-F0 signals, and through data/encode.py --f0 yaapt.
PARITY UNPINNED against amfm_decompy (absent offline)."""
import importlib.util
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from yaapt_cases import CASES, FS, _speech, check_track, pulse_train, speech_track_is_plausible, voiced

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def trk():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dissc_amd.f0 import YaaptTracker
    return YaaptTracker(device="cuda:0")


def _signals():
    rs = np.random.RandomState(5)
    a = np.concatenate([voiced(np.linspace(110, 180, 16000)), 0.002 * rs.standard_normal(4000), voiced(np.full(12000, 240.0))])
    b = voiced(180 + 15 * np.sin(2 * np.pi * 5 * np.arange(20000) / FS)) + 0.001 * rs.standard_normal(20000)
    return [a, b]


def test_front_end_stages_match_the_oracle(trk):
    """ragged batch of 2 (NaN in the padding): band-pass, NLFER energy, SHC, SHC candidates, NCCF, NCCF candidates"""
    from oracle import yaapt_ref as yr
    sigs = [np.pad(x, (160, 160)) for x in _signals()]
    lens = [len(s) for s in sigs]
    N = (max(lens) + 3) // 4 * 4
    wav = torch.full((2, N), float("nan"))
    for i, s in enumerate(sigs):
        wav[i, :lens[i]] = torch.from_numpy(s.astype(np.float32))
    out = trk.spectral(wav, torch.tensor(lens, dtype=torch.int32), want_shc=True)
    F = out["F"]
    for i, s in enumerate(sigs):
        s32 = s.astype(np.float32).astype(np.float64)
        filt, nl = yr.bandpass(s32, FS), yr.bandpass(s32 * s32, FS)
        n = lens[i]
        for got, want in ((out["filt"][i, :n].cpu().numpy(), filt), (out["nlfilt"][i, :n].cpu().numpy(), nl)):
            assert np.abs(got - want).max() <= 2e-5 * np.abs(want).max()
        nframe, njump, samples = yr.frame_geometry(n, FS)
        f = len(samples)
        assert trk.spectral.__self__ is trk and f <= F
        # raw NLFER band sums
        win = yr.hann(nframe + 2)[1:-1]
        spec = np.fft.rfft(yr.stride_matrix(filt, f, nframe, njump) * win, 8192)
        raw = np.abs(spec[:, 60:205]).sum(axis=1)
        got = out["energy"][i, :f].cpu().numpy()
        assert np.abs(got - raw).max() <= 1e-4 * raw.max()
        assert not out["energy"][i, f:].cpu().numpy().any()
        # SHC + candidates on a sample of voiced frames
        energy, vuv = yr.nlfer(filt, FS)
        data = np.append(nl, np.zeros(2 * nframe + (f - 1) * njump - n))
        kw = yr.kaiser(2 * nframe, 0.5)
        shc_g = out["shc"][i].cpu().numpy()
        cp, cm = out["cand_pitch"][i].cpu().numpy(), out["cand_merit"][i].cpu().numpy()
        same = tot = 0
        for fr in np.nonzero(vuv)[0][::7]:
            sl = data[fr * njump:fr * njump + 2 * nframe] * kw
            shc = yr.shc_of_magnitude(np.abs(np.fft.rfft(sl - sl.mean(), 8192)), FS)
            assert np.abs(shc_g[fr] - shc).max() <= 2e-3 * shc.max(), fr
            p, m = yr.peaks(shc, FS / 8192.0, 4)
            tot += 1
            same += int(np.allclose(cp[fr], p, rtol=1e-5, atol=1e-3) and np.allclose(cm[fr], m, rtol=2e-3, atol=2e-3))
        assert tot > 20 and same >= 0.97 * tot, (same, tot)
        # NCCF inside the oracle's lag ranges
        cand_p = np.where(vuv[None, :], cp[:f].T, 0.0)
        cand_m = np.where(vuv[None, :], cm[:f].T, 1.0)
        sp, std, _ = yr.spec_track_from_candidates(cand_p.astype(np.float64), cand_m.astype(np.float64))
        tda, hop, nfr = yr.tda_geometry(n, FS, f)
        lo, hi = yr.lag_ranges(sp[:nfr], std, FS)
        lmin, lmax = np.ones((2, F), np.int32), np.full((2, F), 2, np.int32)
        lmin[i, :nfr], lmax[i, :nfr] = lo, hi
        pit, mer, phi = trk.nccf(out["filt"], out["n_samples"], lmin, lmax, want_phi=True)
        pit, mer, phi = pit[i].cpu().numpy(), mer[i].cpu().numpy(), phi[i].cpu().numpy()
        same = 0
        for fr in range(0, nfr, 5):
            want = yr.crs_corr(filt[fr * hop:fr * hop + tda], int(lo[fr]), int(hi[fr]))
            assert np.abs(phi[fr] - want).max() <= 5e-4, fr
            p, m = yr.cmp_rate(want, FS, 3, int(lo[fr]), int(hi[fr]))
            same += int(np.allclose(pit[fr], p, rtol=1e-5) and np.allclose(mer[fr], m, atol=1e-3))
        assert same >= 0.97 * len(range(0, nfr, 5))
        assert np.all(pit[nfr:] == 0) and np.allclose(mer[nfr:], 0.001)


@pytest.mark.parametrize("name", sorted(CASES))
def test_tracker_on_known_f0(trk, name):
    f0 = trk([voiced(CASES[name])])[0]
    assert f0.dtype == np.float32 and len(f0) == 300
    check_track(f0.astype(np.float64), CASES[name])


def test_tracker_agrees_with_the_oracle_and_is_batch_independent(trk):
    from oracle import yaapt_ref as yr
    sigs = _signals() + [pulse_train(140.0, 24000), np.zeros(8000), 0.1 * np.random.RandomState(0).standard_normal(24000)]
    got = trk(sigs)
    for i, x in enumerate(sigs):
        want = yr.get_yaapt_f0(x.astype(np.float32))
        assert len(got[i]) == len(want)
        both = (got[i] > 0) & (want > 0)
        agree_v = ((got[i] > 0) == (want > 0)).mean()
        assert agree_v >= 0.97, (i, agree_v)
        if both.any():
            rel = np.abs(got[i][both] - want[both]) / want[both]
            assert (rel <= 5e-3).mean() >= 0.97, (i, np.percentile(rel, 97))
        alone = trk([x])[0]  # an utterance on its own == the same utterance in the batch
        np.testing.assert_array_equal(alone, got[i])
    assert not got[3].any() and (got[4] > 0).mean() <= 0.1


def test_tracker_on_the_reference_speech_fixtures(trk, tmp_path):
    """Real speech (the reference's own fixtures, tests/golden/s1_1.wav / s1_2.wav): the HIP tracker gives a plausible
    track, agrees with the CPU restatement (voicing on >= 97 % of the frames, F0 within 0.5 % on >= 99 % of the frames
    both call voiced) and with the committed copy of the restatement's track; the per-unit F0 and the speaker
    statistics data/prep_dataset.py derives from it are finite.  Parity with amfm_decompy stays UNPINNED."""
    from oracle import yaapt_ref as yr
    from dissc_amd import stats as S
    from dissc_amd.f0 import f0_per_unit
    names = ["s1_1", "s1_2"]
    sigs = [_speech(n) for n in names]
    got = trk(sigs)
    fixture = np.load(os.path.join(ROOT, "tests", "golden", "yaapt_speech.npz"))
    per_unit = []
    for n, x, f0 in zip(names, sigs, got):
        assert f0.dtype == np.float32 and len(f0) == 400
        speech_track_is_plausible(f0.astype(np.float64), n)
        for want, src in ((yr.get_yaapt_f0(x), "oracle"), (fixture[n].astype(np.float64), "fixture")):
            agree = ((f0 > 0) == (want > 0)).mean()
            both = (f0 > 0) & (want > 0)
            rel = np.abs(f0[both] - want[both]) / want[both]
            print(f"{n} vs {src}: voicing agreement {agree:.4f}, co-voiced frames {int(both.sum())}, "
                  f"within 0.5 %: {(rel <= 5e-3).mean():.4f}, max rel {rel.max():.2e}")
            assert agree >= 0.97, (n, src, agree)
            assert (rel <= 5e-3).mean() >= 0.99, (n, src, (rel <= 5e-3).mean())
        np.testing.assert_array_equal(trk([x])[0], f0)  # batch independence on speech too
        u = f0_per_unit(f0, 99)
        assert np.isfinite(u).all() and (u > 0).mean() >= 0.5
        per_unit.append(u)
    # encode -> prep_dataset statistics (mean / std of the voiced per-unit values per speaker), on the device
    st = S.pitch_stats({"s1": np.concatenate(per_unit)}, device="cuda:0", on_unvoiced="raise")["s1"]
    assert np.isfinite(st["mean"]) and np.isfinite(st["std"]) and 80 < float(st["mean"]) < 200 and 5 < float(st["std"]) < 60


def _long_batch():
    rs = np.random.RandomState(11)
    sigs = _signals() + [pulse_train(140.0, 24000), np.zeros(8000), 0.1 * rs.standard_normal(24000)]
    # a 10 s utterance with voiced / unvoiced alternation and a short one (3 frames)
    parts = []
    for k in range(10):
        parts.append(voiced(np.linspace(100 + 12 * k, 130 + 15 * k, 12000)))
        parts.append(0.003 * rs.standard_normal(4000))
    sigs.append(np.concatenate(parts))
    sigs.append(voiced(np.full(600, 200.0)))
    return sigs


def test_device_dp_stages_match_the_host_stages(trk):
    """spec_track (normalisation, median, 4-candidate Viterbi, pchip, lag ranges) and the final pass (merge, sort,
    8-candidate Viterbi) as one-workgroup-per-utterance kernels against the numpy functions of dissc_amd/f0.py, which
    are the restatement's (oracle/yaapt_ref.py) vectorised form: same tracks."""
    from dissc_amd import f0 as f0m
    sigs = _long_batch()
    pad = trk.flen // 2
    lens = [len(x) + 2 * pad for x in sigs]
    N = (max(lens) + 3) // 4 * 4
    wav = torch.zeros(len(sigs), N)
    for i, x in enumerate(sigs):
        wav[i, pad:pad + len(x)] = torch.from_numpy(np.asarray(x, dtype=np.float32))
    s = trk.spectral(wav, torch.tensor(lens, dtype=torch.int32))
    nfr = [f0m.lib.dissc_yaapt_frames(trk._h, n) for n in lens]
    ntd = [min(f0m.lib.dissc_yaapt_tda_frames(trk._h, n), f) for n, f in zip(lens, nfr)]
    st = trk.spec_track(s, nfr, ntd)
    energy = s["energy"].cpu().numpy().astype(np.float64)
    cp, cm = s["cand_pitch"].cpu().numpy(), s["cand_merit"].cpu().numpy()
    p = trk.p
    for b in range(len(sigs)):
        f, t = nfr[b], ntd[b]
        en = energy[b, :f] / energy[b, :f].mean() if energy[b, :f].mean() > 0 else energy[b, :f]
        vuv = en > p["nlfer_thresh1"]
        spec, std = f0m.spectral_track(np.where(vuv[None], cp[b, :f].T, 0.0), np.where(vuv[None], cm[b, :f].T, 1.0), p)
        np.testing.assert_allclose(st["en_norm"][b, :f].cpu().numpy(), en, rtol=1e-12)
        np.testing.assert_array_equal(st["vuv"][b, :f].cpu().numpy().astype(bool), vuv)
        np.testing.assert_allclose(st["spec"][b, :f].cpu().numpy(), spec, rtol=1e-9, err_msg=str(b))
        assert abs(float(st["spec_std"][b]) - std) <= 1e-9 * std
        lo, hi = f0m.lag_ranges(spec[:t], std, trk.fs, p)
        np.testing.assert_array_equal(st["lag_min"][b, :t].cpu().numpy(), lo)
        np.testing.assert_array_equal(st["lag_max"][b, :t].cpu().numpy(), hi)
        assert (st["lag_min"][b, t:].cpu().numpy() == 1).all() and (st["lag_max"][b, t:].cpu().numpy() == 2).all()
    dev = trk(sigs)
    host = trk(sigs, host_dp=True)
    for b in range(len(sigs)):
        assert len(dev[b]) == len(host[b]) == nfr[b]
        np.testing.assert_allclose(dev[b], host[b], rtol=1e-6, atol=0, err_msg=str(b))
    assert (dev[-2] > 0).mean() > 0.5 and not dev[3].any()


def test_encode_cli_writes_yaapt_f0_and_prep_dataset_accepts_it(trk, tmp_path):
    """data/encode.py (default --f0 yaapt) -> per-unit F0 in Hz -> data/prep_dataset.py statistics: the chain the
    ADVICE of round 1 found broken (all-zero f0 -> NaN statistics)."""
    import synthdata as synth
    td = str(tmp_path)
    os.makedirs(f"{td}/ckpt")
    os.makedirs(f"{td}/wav")
    torch.save({"model": synth.synth_hubert_state_dict(6)}, f"{td}/ckpt/hubert-base-ls960.pt")
    np.save(f"{td}/ckpt/kmeans_100.npy", synth.synth_kmeans_centers().numpy())
    f0s = {"spk1_001.wav": 120.0, "spk1_002.wav": 130.0, "spk2_001.wav": 210.0}
    for nm, f in f0s.items():
        x = voiced(np.full(24000, f))
        wavfile.write(f"{td}/wav/{nm}", FS, np.round(x / np.abs(x).max() * 20000).astype(np.int16))
    spec = importlib.util.spec_from_file_location("enc_cli_yaapt", os.path.join(ROOT, "data", "encode.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    cli.main(["--base_dir", f"{td}/wav", "--out_file", f"{td}/enc/train.txt", "--checkpoint_dir", f"{td}/ckpt"])
    lines = [json.loads(x) for x in open(f"{td}/enc/train.txt").read().strip().split("\n")]
    assert sorted(d["audio"] for d in lines) == sorted(f0s)
    for d in lines:
        f0 = np.array(d["f0"])
        assert len(f0) == len(d["units"]) == 74  # (24000 - 400) // 320 + 1
        v = f0[3:-3]
        assert (v > 0).all() and np.abs(v - f0s[d["audio"]]).max() <= 0.02 * f0s[d["audio"]]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "data", "prep_dataset.py"), "--encoded_path",
                        f"{td}/enc/train.txt", "--stats_path", f"{td}/enc/f0_stats.pkl"],
                       capture_output=True, text=True, timeout=600, cwd=td)
    assert r.returncode == 0, r.stderr
    stats = pickle.load(open(f"{td}/enc/f0_stats.pkl", "rb"))
    assert abs(stats["spk1"]["mean"] - 125.0) < 2.5 and abs(stats["spk2"]["mean"] - 210.0) < 4.2
