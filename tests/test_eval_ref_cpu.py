"""tests/eval_ref.py (the CPU yardstick of the prosody metrics) against the reference's own results stored in
tests/golden/eval_prosody.npz (tests/golden/make_eval_golden.py) and against scipy: exact, no tolerance -- an FFE is a
ratio of two integers computed in double."""
import json
import os

import numpy as np
import pytest
from scipy.interpolate import interp1d

import eval_ref as er


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "eval_prosody.npz"))


def same(a, b):
    """equal bit patterns up to NaN payload: NaN only where NaN"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def test_interval_ffe_equals_the_reference(gold):
    tracks, n = gold["iv_tracks"], gold["iv_n_frames"]
    seen = {"nan": 0, "raise": 0, "len1": 0}
    for (rr, rs), t, want, status in zip(gold["iv_rows"], gold["iv_times"], gold["iv_ffe"], gold["iv_status"]):
        ref, syn = tracks[rr, :n[rr]].astype(np.float64), tracks[rs, :n[rs]].astype(np.float64)
        lo, hi = er.slice_bounds(t[2], t[3], len(syn))
        seen["len1"] += hi - lo == 1
        args = ([er.Interval(t[0], t[1], "x")], [er.Interval(t[2], t[3], "x")], ref, syn)
        if status == 1:
            seen["raise"] += 1
            with pytest.raises(ValueError):
                er.aligned_ffe(*args)
        else:
            got = er.aligned_ffe(*args)
            seen["nan"] += bool(np.isnan(want))
            assert same(got, want), (t, got, want)
    assert min(seen.values()) >= 2, seen  # the three quirk cases are in the fixture


def test_recorded_interp_quirks(gold):
    assert np.array_equal(gold["interp_len1"], [400.0]) and np.array_equal(er.interp(np.array([100.0]), 4), [400.0])
    assert int(gold["interp_empty_raises"]) == 1
    with pytest.raises(ValueError):
        er.interp(np.zeros(0), 3)
    assert er.interp(np.zeros(0), 0).shape == (0,)


def test_nearest_map_equals_scipy_everywhere():
    """every (cur_len, target_len) in 1..200 x 0..200 through the expression reference utils.interp evaluates"""
    ties = 0
    for cur in range(1, 201):
        vals = np.arange(cur, dtype=np.float64) + 1.0
        x = np.linspace(0.0, 1.0, cur)
        for tgt in range(0, 201):
            got = er.interp(vals, tgt)
            if cur == 1:
                want = np.array(tgt * vals)
            elif tgt == cur:
                want = vals
            else:
                want = interp1d(x, vals, bounds_error=False, kind="nearest", fill_value=0)(np.linspace(0.0, 1.0, tgt))
                if tgt > 1:
                    mid = x[:-1] / 2.0 + x[1:] / 2.0
                    ties += int(np.isin(np.linspace(0.0, 1.0, tgt), mid).any())
            assert np.array_equal(got, want), (cur, tgt)
    assert ties > 4000  # grid points exactly on a midpoint are common: the tie rule is exercised


def file_results(gold):
    """eval_ref.score_file over the golden tree in the reference's (sorted) order with its skip rules applied by hand"""
    tree = json.loads(str(gold["file_tree"]))
    tracks, n, samples = gold["file_tracks"], gold["file_n_frames"], gold["file_samples"]

    class Grid:
        def __init__(self, g):
            self.maxTime = g["maxTime"]
            self.tiers = [[er.Interval(a, b, m) for a, b, m in zip(g[k][0][:-1], g[k][0][1:], g[k][1])] for k in "wp"]

        def __len__(self):
            return 2

        def __getitem__(self, i):
            return self.tiers[i]

    rows = []
    for trg in ("p231", "p270"):
        for name in sorted(tree["gen"][trg]):
            src, seq = name.split("_")
            if src == trg or f"{trg}_{seq}" not in tree["orig"] or (src == "p270" and seq == "024"):
                continue
            o, g = tree["orig"][f"{trg}_{seq}"], tree["gen"][trg][name]
            rows.append(er.score_file(tracks[o["track"], :n[o["track"]]], tracks[g["track"], :n[g["track"]]],
                                      int(samples[o["track"]]), int(samples[g["track"]]), Grid(o["grid"]),
                                      Grid(g["grid"]) if g["grid"] else None))
    return rows


def test_file_results_equal_the_reference(gold):
    rows = file_results(gold)
    assert len(rows) == len(gold["res_len"]) == 7
    for key in ("len", "emd", "p_len", "p_ffe", "w_len", "w_ffe"):
        got = [r[key] for r in rows if key in r]
        assert same(got, gold["res_" + key]), (key, got, gold["res_" + key])
    # the cases the tree was built for: a tier dropped for its interval count, an FFE dropped after its length error
    assert len(gold["res_p_len"]) == 6 and len(gold["res_p_ffe"]) == 5 and len(gold["res_w_ffe"]) == 7
