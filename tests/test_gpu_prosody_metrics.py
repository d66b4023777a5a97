"""The prosody-metric kernels (csrc/prosody_metrics.hip through dissc_amd.metrics) and eval.py on the MI355X.

Yardsticks: scipy.stats.wasserstein_distance for the EMD, tests/eval_ref.py (pinned to the reference's own functions by
tests/test_eval_ref_cpu.py) for everything else.

EMD bar, derived and not measured: every term |cdf_a - cdf_b| * delta of the sum is non-negative, so a double sum of n
terms in ANY order is within n * 2^-53 of the exact sum, relative; scipy's pairwise sum likewise; the terms themselves
carry a few roundings each.  Allowed: 4 * (len_a + len_b) * 2^-53 relative (1.1e-11 at 24 000 values).  Two all-zero
tracks give exactly 0.0.  The FFE is a count divided by a length in double: compared bit for bit.
"""
import os
import pickle

import numpy as np
import pytest
import torch
from scipy.io import wavfile
from scipy.stats import wasserstein_distance

import eval_ref as er
from yaapt_cases import CASES, FS, _speech, voiced

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def metrics():
    from dissc_amd import metrics
    return metrics


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "eval_prosody.npz"))


def same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


# ---------------------------------------------------------------------------------------------------------
# EMD
# ---------------------------------------------------------------------------------------------------------
def emd_cases():
    rng = np.random.RandomState(11)
    levels = np.array([0.0, 0.0, 97.5, 110.0, 110.0, 182.25], np.float32)
    rows = [er.synth_track(rng, 700), er.synth_track(rng, 700), er.synth_track(rng, 811), np.zeros(900, np.float32),
            rng.choice(levels, 3000).astype(np.float32), rng.choice(levels, 2999).astype(np.float32),
            er.synth_track(rng, 12000), er.synth_track(rng, 12000), np.array([143.5], np.float32),
            np.array([88.0], np.float32)]
    F = max(len(r) for r in rows)
    tracks = np.stack([np.pad(r, (0, F - len(r))) for r in rows])
    n = [len(r) for r in rows]
    # (row_a, n_a, len_a, row_b, n_b, len_b)
    pairs = [(0, 700, 700, 1, 700, 700),        # equal sizes, ~40 % zeros each
             (0, 700, 700, 2, 811, 811),        # unequal sizes
             (2, 811, 811, 0, 700, 811),        # the reference's zero extension
             (1, 500, 700, 0, 650, 651),        # both cut and extended, unequal
             (8, 1, 1, 9, 1, 1),                # length 1 against length 1
             (8, 1, 1, 0, 700, 700),            # length 1 against a track
             (3, 900, 900, 3, 640, 640),        # both all-zero
             (3, 0, 500, 3, 0, 77),             # nothing read at all: zeros only
             (3, 900, 900, 1, 700, 700),        # all-zero against a track
             (4, 3000, 3000, 5, 2999, 2999),    # six distinct values, heavy ties
             (4, 3000, 3000, 4, 3000, 3000),    # a track against itself
             (6, 12000, 12000, 7, 12000, 12000),  # 60 s + 60 s
             (6, 12000, 12000, 0, 700, 700)]
    assert all(na <= n[ra] and nb <= n[rb] for ra, na, _, rb, nb, _ in pairs)
    return tracks, pairs


def emd_want(tracks, pair):
    ra, na, la, rb, nb, lb = pair
    a = np.pad(tracks[ra, :na].astype(np.float64), (0, la - na))
    b = np.pad(tracks[rb, :nb].astype(np.float64), (0, lb - nb))
    return wasserstein_distance(a, b)


def test_track_emd_against_scipy_and_batch_independent(metrics):
    tracks, pairs = emd_cases()
    dev = torch.from_numpy(tracks).to(DEV)
    got = metrics.track_emd(dev, pairs).cpu().numpy()
    for k, pair in enumerate(pairs):
        want = emd_want(tracks, pair)
        bar = 4 * (pair[2] + pair[5]) * 2.0 ** -53
        print(f"emd pair {pair}: got {got[k]!r} want {want!r} rel {abs(got[k] - want) / want if want else 0.0:.2e} bar {bar:.2e}")
        assert abs(got[k] - want) <= bar * abs(want), (pair, got[k], want)
    assert got[6] == 0.0 and got[7] == 0.0 and got[10] == 0.0  # exactly
    assert got[11] > 1.0 and got[1] > 0.1                       # not vacuous
    for k, pair in enumerate(pairs):                            # alone = inside the batch, to the bit
        alone = metrics.track_emd(dev, [pair]).cpu().numpy()
        assert alone[0] == got[k], (pair, alone[0], got[k])
    rev = metrics.track_emd(dev, pairs[::-1]).cpu().numpy()
    assert np.array_equal(rev[::-1], got)


def test_track_emd_refuses_what_it_cannot_hold(metrics):
    from dissc_amd import DisscError
    dev = torch.zeros(2, 64, device=DEV)
    with pytest.raises(DisscError, match="does not fit the LDS"):
        metrics.track_emd(dev, [(0, 64, 30000, 1, 64, 10001)])
    # entries that break the table's rules come back as NaN, the others are computed
    got = metrics.track_emd(dev, [(0, 64, 64, 1, 64, 64), (2, 64, 64, 1, 64, 64), (0, 65, 65, 1, 64, 64),
                                  (0, 10, 5, 1, 64, 64), (0, 0, 0, 1, 64, 64), (-1, 1, 1, 0, 1, 1)]).cpu().numpy()
    assert got[0] == 0.0 and np.isnan(got[1:]).all()
    assert metrics.track_emd(dev, np.zeros((0, 6), np.int32)).shape == (0,)


# ---------------------------------------------------------------------------------------------------------
# FFE
# ---------------------------------------------------------------------------------------------------------
def ffe_want(tracks, n_frames, rows, times):
    """eval_ref on one interval at a time -> (table [S, 6], ffe [S], status [S])"""
    table, ffe, status = [], [], []
    for (rr, rs), t in zip(rows, times):
        ref, syn = tracks[rr, :n_frames[rr]].astype(np.float64), tracks[rs, :n_frames[rs]].astype(np.float64)
        table.append((rr, *er.slice_bounds(t[0], t[1], len(ref)), rs, *er.slice_bounds(t[2], t[3], len(syn))))
        try:
            ffe.append(er.aligned_ffe([er.Interval(t[0], t[1], "x")], [er.Interval(t[2], t[3], "x")], ref, syn))
            status.append(0)
        except ValueError:
            ffe.append(np.nan)
            status.append(1)
    return np.array(table, np.int32), np.array(ffe), np.array(status, np.int32)


def test_track_ffe_on_the_reference_goldens(metrics, gold):
    table, ffe, status = ffe_want(gold["iv_tracks"], gold["iv_n_frames"], gold["iv_rows"], gold["iv_times"])
    assert same(ffe, gold["iv_ffe"]) and np.array_equal(status, gold["iv_status"])  # eval_ref = the reference, here too
    got, st = metrics.track_ffe(torch.from_numpy(gold["iv_tracks"]).to(DEV), table)
    assert np.array_equal(st.cpu().numpy(), gold["iv_status"])
    assert same(got.cpu().numpy(), gold["iv_ffe"])


def random_batch():
    rng = np.random.RandomState(77)
    tracks, n_frames, rows, times = [], [], [], []
    for _ in range(300):
        n_ref, n_syn = (int(v) for v in rng.randint(300, 901, 2))
        ref, syn = er.synth_pair(rng, n_ref, n_syn)
        tracks += [ref, syn]
        n_frames += [n_ref, n_syn]
        rows += [(len(tracks) - 2, len(tracks) - 1)] * 8
        times += list(er.synth_cuts(rng, n_ref, n_syn, 8))
    at = lambda i: (i - 2 + 0.5) / 200.0  # a time whose frame index is i  # noqa: E731
    for k in range(12):  # length-1 generated slices by hand
        rows.append((2 * k, 2 * k + 1))
        times.append((at(20 + k), at(60 + 3 * k), at(100 + 7 * k), at(101 + 7 * k)))
    F = max(n_frames)
    return np.stack([np.pad(t, (0, F - len(t))) for t in tracks]), n_frames, rows, times


def test_track_ffe_on_a_random_batch_bit_equal_and_batch_independent(metrics):
    tracks, n_frames, rows, times = random_batch()
    table, ffe, status = ffe_want(tracks, n_frames, rows, times)
    S = len(ffe)
    ok = status == 0
    share = {"between": np.mean(ok & (ffe > 0) & (ffe < 1)), "nan": np.mean(ok & np.isnan(ffe)), "raise": np.mean(status == 1),
             "len1": np.mean((table[:, 5] - table[:, 4] == 1) & (table[:, 2] - table[:, 1] > 1))}
    print(f"random batch: {S} intervals, {share}")
    assert S >= 2000 and share["between"] >= 0.5, share  # not vacuous
    assert min(share["nan"], share["raise"], share["len1"]) > 0 and share["nan"] + share["raise"] + share["len1"] < 0.05, share
    dev = torch.from_numpy(tracks).to(DEV)
    got, st = metrics.track_ffe(dev, table)
    got, st = got.cpu().numpy(), st.cpu().numpy()
    assert np.array_equal(st, status)
    assert same(got, ffe), np.flatnonzero(~((got == ffe) | (np.isnan(got) & np.isnan(ffe))))[:10]
    for k in list(range(0, S, 61)) + list(np.flatnonzero(status == 1)[:3]) + list(np.flatnonzero(ok & np.isnan(ffe))[:3]):
        g1, s1 = metrics.track_ffe(dev, table[k:k + 1])
        assert same(g1.cpu().numpy(), got[k:k + 1]) and int(s1[0]) == st[k], k
    g2, s2 = metrics.track_ffe(dev, table[::-1].copy())
    assert same(g2.cpu().numpy()[::-1], got) and np.array_equal(s2.cpu().numpy()[::-1], st)


def test_track_ffe_every_length_pair_through_the_kernel(metrics):
    """(cur_len, target_len) in 1..200 x 0..200: the nearest map with its ties, the length-1 product, equal lengths"""
    rng = np.random.RandomState(5)
    levels = np.array([0.0, 100.0, 130.0, 170.0], np.float32)  # neighbours differ by more than 20 %: a wrong index shows
    tracks = rng.choice(levels, (2, 200)).astype(np.float32)
    tracks[1, 0] = 0.5  # the length-1 product: 0.5 * target_len crosses the levels
    table = np.array([(0, 0, tgt, 1, 0, cur) for cur in range(1, 201) for tgt in range(0, 201)], np.int32)
    want = np.array([er.slice_ffe(tracks[0, :tgt], tracks[1, :cur]) for _, _, tgt, _, _, cur in table])
    got, st = metrics.track_ffe(torch.from_numpy(tracks).to(DEV), table)
    assert not st.cpu().numpy().any()
    got = got.cpu().numpy()
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
    assert len(bad) == 0, [tuple(table[b]) for b in bad[:10]]
    assert np.isnan(want).sum() == 200 and np.mean((want > 0) & (want < 1)) > 0.9


def test_track_ffe_marks_bad_entries(metrics):
    dev = torch.full((2, 32), 100.0, device=DEV)
    got, st = metrics.track_ffe(dev, [(0, 0, 8, 1, 0, 8), (2, 0, 8, 1, 0, 8), (0, 0, 33, 1, 0, 8), (0, 5, 4, 1, 0, 8),
                                      (0, 0, 8, 1, -1, 8), (0, 0, 8, 1, 8, 8)])
    assert st.cpu().tolist() == [0, 2, 2, 2, 2, 1]
    got = got.cpu().numpy()
    assert got[0] == 0.0 and np.isnan(got[1:]).all()


# ---------------------------------------------------------------------------------------------------------
# tracker keyword, evaluator, eval.py
# ---------------------------------------------------------------------------------------------------------
def test_tracker_on_device_returns_the_same_values():
    from dissc_amd.f0 import YaaptTracker
    trk = YaaptTracker(device=DEV)
    waves = [_speech("s1_1"), voiced(CASES["vibrato"])[:9000].astype(np.float32), _speech("s1_2")]
    host = trk(waves)
    f0, counts = trk(waves, on_device=True)
    assert f0.is_cuda and f0.dtype == torch.float32 and f0.shape[0] == 3 and f0.shape[1] >= max(counts)
    assert counts == [len(h) for h in host]
    f0 = f0.cpu().numpy()
    for b, h in enumerate(host):
        assert np.array_equal(f0[b, :counts[b]], h) and not f0[b, counts[b]:].any()  # zero beyond a row's frames
    assert trk([], on_device=True)[1] == []
    with pytest.raises(ValueError):
        trk(waves, host_dp=True, on_device=True)


def build_results_tree(root):
    """orig/ + sr/p231/ from the speech fixtures and known-F0 signals, with TextGrids over each file's duration"""
    rng = np.random.RandomState(9)
    waves = {"orig/p231_001": _speech("s1_1"), "orig/p231_002": voiced(CASES["glide100-250"]),
             "sr/p231/p225_001": _speech("s1_2"),                       # aligned, same interval counts
             "sr/p231/p226_001": voiced(CASES["vibrato"])[:20000],      # MFA failed: no grid
             "sr/p231/p227_002": voiced(CASES["flat120"])[:21000],      # another phone count
             "sr/p231/p228_002": voiced(CASES["flat200"]),              # same length as its reference
             "sr/p231/p231_001": _speech("s1_1"),                       # reconstruction: skipped
             "sr/p231/p229_007": _speech("s1_2")}                       # no reference: skipped
    phones = {"sr/p231/p227_002": 3}
    for name, x in waves.items():
        folder = os.path.join(root, os.path.dirname(name))
        os.makedirs(os.path.join(folder, "txtgrid"), exist_ok=True)
        x = np.asarray(x, np.float64)
        wavfile.write(os.path.join(root, name + ".wav"), FS, np.round(x / np.abs(x).max() * 20000).astype(np.int16))
        if name.endswith("p226_001"):
            continue
        dur, n_words, ppw = round(len(x) / FS, 4), 6, phones.get(name, 2)
        w = np.concatenate([[0.0], (np.arange(1, n_words) + rng.uniform(-0.3, 0.3, n_words - 1)) * dur / n_words, [dur]]).round(4)
        wm = ["", "a", "b", "c", "d", ""]
        p, pm = [0.0], []
        for i in range(n_words):
            k = ppw if wm[i] else 1
            p += list(np.linspace(w[i], w[i + 1], k + 1)[1:].round(4))
            pm += [f"{wm[i]}{j}" if wm[i] else "" for j in range(k)]
        er.write_textgrid(os.path.join(folder, "txtgrid", os.path.basename(name) + ".TextGrid"), dur,
                          [("words", w, wm), ("phones", p, pm)])
    return ["p225_001", "p226_001", "p227_002", "p228_002"]


def test_eval_cli_end_to_end_on_the_trackers_own_tracks(metrics, tmp_path, monkeypatch, capsys):
    """pickle and printed block of eval.py = eval_ref on the tracks the tracker gives for the same files: this isolates
    the new stage (the tracker's parity with YAAPT is the business of test_gpu_yaapt.py)"""
    import glob
    import eval as dissc_eval
    from dissc_amd.f0 import YaaptTracker
    from dissc_amd.textgrid import TextGrid
    root = str(tmp_path)
    names = build_results_tree(root)
    real = glob.glob
    monkeypatch.setattr(dissc_eval.glob, "glob", lambda pat: sorted(real(pat)))
    # --batch_seconds 3: the four files fall into several batches, the reference of 002 is carried from one to the next
    dissc_eval.main(["--base_path", root, "--method", "sr", "--device", DEV, "--target_speakers", "p231",
                     "--batch_seconds", "3"])
    said = capsys.readouterr().out.splitlines()
    with open(os.path.join(root, "sr_results.pkl"), "rb") as f:
        errs = pickle.load(f)

    trk = YaaptTracker(device=DEV)
    want = {k: [] for k in ("len", "emd", "p_len", "p_ffe", "w_len", "w_ffe")}
    bars = []
    for name in names:
        ref_name = "p231_" + name.split("_")[1]
        ref_w, syn_w = (metrics.load_wav(os.path.join(root, p + ".wav"))[0] for p in ("orig/" + ref_name, "sr/p231/" + name))
        ref_f0, syn_f0 = trk([metrics.peak_normalize(ref_w), metrics.peak_normalize(syn_w)])
        bars.append(4 * 2 * max(len(ref_f0), len(syn_f0)) * 2.0 ** -53)  # both samples are at most the longer track
        grid = os.path.join(root, "sr/p231/txtgrid", name + ".TextGrid")
        row = er.score_file(ref_f0, syn_f0, len(ref_w), len(syn_w),
                            TextGrid.fromFile(os.path.join(root, "orig/txtgrid", ref_name + ".TextGrid")),
                            TextGrid.fromFile(grid) if os.path.isfile(grid) else None)
        for k in want:
            if k in row:
                want[k].append(row[k])
    print("eval.py:", {k: errs[k] for k in want}, "\neval_ref:", want)
    assert [len(want[k]) for k in ("len", "emd", "p_len", "p_ffe", "w_len", "w_ffe")] == [4, 4, 3, 3, 4, 4]
    assert set(errs) == {"wer_s", "wer_d", "cer_s", "cer_d", "len", "emd", "w_ffe", "w_len", "p_ffe", "p_len"}
    for k in ("len", "p_len", "p_ffe", "w_len", "w_ffe"):
        assert same(errs[k], want[k]), (k, errs[k], want[k])
    assert sum(0 < v < 1 for v in want["w_ffe"]) >= 2 and min(want["emd"]) > 0  # real numbers, not only 0 / 1 / NaN
    assert len(errs["emd"]) == 4 and all(abs(g - w) <= b * w for g, w, b in zip(errs["emd"], want["emd"], bars)), \
        (errs["emd"], want["emd"])
    bar = max(bars)
    assert said[0] == "--- speaker p231 -----" and "No reference recording:  p231_007.wav" in said
    block = said[-8:]
    assert block[:2] == ["WER:  n/a", "CER:  n/a"] and block[2].startswith("EMD:  ")
    assert abs(float(block[2][6:]) - np.mean(want["emd"])) <= bar * np.mean(want["emd"])
    assert block[3:] == [f"Len Error:  {np.mean(want['len']) / 16000}", f"Word Len Error:  {np.mean(want['w_len'])}",
                         f"Char Len Error:  {np.mean(want['p_len'])}", f"Word FFE:  {np.mean(want['w_ffe'])}",
                         f"Character FFE:  {np.mean(want['p_ffe'])}"]
