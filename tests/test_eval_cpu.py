"""eval.py without a GPU: the discovery / skip / seq rules, the pickle and the printed block on the results tree of
tests/golden/eval_prosody.npz, with the tracks injected through a stand-in evaluator built on tests/eval_ref.py and the
grids read from real TextGrid files by dissc_amd.textgrid.  The lists must equal what the reference's calc_errors gave
on the same tree (the fixture), exactly.  Also: the host bookkeeping of dissc_amd.metrics (frame bounds, EMD sizes,
pseudo-intervals) equals eval_ref's."""
import argparse
import glob
import json
import os
import pickle

import numpy as np
import pytest

import eval_ref as er


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "eval_prosody.npz"))


def build_tree(root, gold):
    """the fixture's tree on disk (empty WAVs: the stand-in evaluator never opens them) -> {wav path: track index}"""
    tree = json.loads(str(gold["file_tree"]))
    index = {}

    def put(folder, name, entry):
        os.makedirs(os.path.join(root, folder, "txtgrid"), exist_ok=True)
        wav = os.path.join(root, folder, name + ".wav")
        open(wav, "wb").close()
        index[os.path.normpath(wav)] = entry["track"]
        g = entry["grid"]
        if g:
            er.write_textgrid(os.path.join(root, folder, "txtgrid", name + ".TextGrid"), g["maxTime"],
                              [("words", g["w"][0], g["w"][1]), ("phones", g["p"][0], g["p"][1])])

    for name, entry in tree["orig"].items():
        put("orig", name, entry)
    for trg, files in tree["gen"].items():
        for name, entry in files.items():
            put(os.path.join("sr", trg), name, entry)
    return index


class InjectedEvaluator:
    def __init__(self, gold, index):
        self.gold, self.index, self.jobs = gold, index, None

    def evaluate(self, jobs):
        from dissc_amd.textgrid import TextGrid
        g = self.gold
        self.jobs = list(jobs)
        out = []
        for ref_wav, syn_wav, ref_grid, syn_grid in self.jobs:
            r, s = self.index[os.path.normpath(ref_wav)], self.index[os.path.normpath(syn_wav)]
            out.append(er.score_file(g["file_tracks"][r, :g["file_n_frames"][r]], g["file_tracks"][s, :g["file_n_frames"][s]],
                                     int(g["file_samples"][r]), int(g["file_samples"][s]), TextGrid.fromFile(ref_grid),
                                     TextGrid.fromFile(syn_grid) if syn_grid else None))
        return out


def same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def test_tree_discovery_pickle_and_printed_block(gold, tmp_path, monkeypatch, capsys):
    import eval as dissc_eval
    index = build_tree(str(tmp_path), gold)
    real = glob.glob
    monkeypatch.setattr(dissc_eval.glob, "glob", lambda pat: sorted(real(pat)))  # the fixture's (sorted) file order
    args = dissc_eval.build_parser().parse_args(["--base_path", str(tmp_path), "--target_speakers", "p231", "p270"])
    assert (args.method, args.device, args.batch_seconds) == ("sr", "cuda:0", 640.0)
    ev = InjectedEvaluator(gold, index)
    errs = dissc_eval.calc_errors(ev, args)
    names = [os.path.basename(j[1]) for j in ev.jobs]
    assert names == ["p225_001.wav", "p226_001.wav", "p227_001.wav", "p229_002.wav", "p230_002.wav", "p232_001.wav",
                     "p225_003.wav"]
    assert [j[3] is None for j in ev.jobs] == [False, True, False, False, False, False, False]
    assert os.path.basename(ev.jobs[3][0]) == "p231_002.wav" and ev.jobs[3][2].endswith("txtgrid/p231_002.TextGrid")
    said = capsys.readouterr().out
    assert "--- speaker p231 -----" in said and "No reference recording:  p231_009.wav" in said
    assert "p270_024 is a problematic sample" in said
    assert set(errs) == {"wer_s", "wer_d", "cer_s", "cer_d", "len", "emd", "w_ffe", "w_len", "p_ffe", "p_len"}
    for key in ("len", "emd", "p_len", "p_ffe", "w_len", "w_ffe"):
        assert same(errs[key], gold["res_" + key]), key
    dissc_eval.log_results(errs, args)
    lines = capsys.readouterr().out.splitlines()
    assert lines[:2] == ["WER:  n/a", "CER:  n/a"]
    assert lines[2:] == [f"EMD:  {np.mean(errs['emd'])}", f"Len Error:  {np.mean(errs['len']) / 16000}",
                         f"Word Len Error:  {np.mean(errs['w_len'])}", f"Char Len Error:  {np.mean(errs['p_len'])}",
                         f"Word FFE:  {np.mean(errs['w_ffe'])}", f"Character FFE:  {np.mean(errs['p_ffe'])}"]
    with open(tmp_path / "sr_results.pkl", "rb") as f:
        saved = pickle.load(f)
    assert list(saved) == list(errs) and saved["wer_d"] == 0 and same(saved["emd"], errs["emd"])


def test_reference_defaults_of_the_parser():
    import eval as dissc_eval
    args = dissc_eval.build_parser().parse_args([])
    assert vars(args) == {"base_path": "../results/vctk/", "method": "sr", "device": "cuda:0",
                          "target_speakers": ["p231", "p239", "p245", "p270"], "batch_seconds": 640.0}


def test_host_bookkeeping_of_the_binding_equals_eval_ref(gold):
    from dissc_amd import metrics
    rng = np.random.RandomState(3)
    for t in np.concatenate([gold["iv_times"].ravel(), rng.uniform(0, 60, 2000), [0.0, 0.005, 1e-9, 59.9975]]):
        assert metrics.frame_index(t) == er.frame_index(t)
    for a, b, n in zip(rng.uniform(-1, 5, 500), rng.uniform(-1, 5, 500), rng.randint(0, 900, 500)):
        assert metrics.slice_bounds(a, b, n) == er.slice_bounds(a, b, n)
        lo, hi = metrics.slice_bounds(a, b, n)
        assert 0 <= lo <= hi <= n and hi - lo == len(np.arange(n)[er.frame_index(a):er.frame_index(b)])
    for fr, fs, sr_, ss in rng.randint(1, 50, (500, 4)):
        assert metrics.emd_lengths(fr, fs, sr_, ss) == er.emd_lengths(fr, fs, sr_, ss)
    tier = [er.Interval(0, 0.5, ""), er.Interval(0.5, 1.1, "a"), er.Interval(1.1, 1.2, ""), er.Interval(1.2, 2.0, "b")]
    for syn in (None, tier[1:]):
        got, want = metrics.tier_intervals(tier, syn, 2.0), er.tier_intervals(tier, syn, 2.0)
        assert [[(i.minTime, i.maxTime, i.mark) for i in side] for side in got] == \
               [[(i.minTime, i.maxTime, i.mark) for i in side] for side in want]
    w = rng.standard_normal(1000).astype(np.float32)
    assert np.array_equal(metrics.peak_normalize(w), (w / np.abs(w).max()) * np.float32(0.95))
    assert not metrics.peak_normalize(np.zeros(8)).any()


def test_evaluator_and_kernels_refuse_the_cpu():
    from dissc_amd import DisscError, metrics
    import torch
    with pytest.raises(DisscError):
        metrics.ProsodyEvaluator("cpu")
    with pytest.raises(DisscError):
        metrics.track_emd(torch.zeros(2, 8), [(0, 8, 8, 1, 8, 8)])
    L = metrics.lib
    assert L.dissc_track_emd(None, 1, 8, None, 1, 16, None, None, 0, None) == -1 and b"bad argument" in L.dissc_last_error()
    assert L.dissc_track_ffe(None, 1, 8, None, 1, None, None, None, 0, None) == -1
    assert L.dissc_track_emd(1, 1, 8, 1, 1, metrics.EMD_MAX_PAIR_FRAMES + 1, 1, None, 0, None) == -1
    assert b"does not fit the LDS" in L.dissc_last_error()
    assert L.dissc_track_emd(None, 0, 0, None, 0, 0, None, None, 0, None) == 0
    assert L.dissc_track_emd_workspace_bytes(4, 100) == 0 and L.dissc_track_ffe_workspace_bytes(4) == 0
