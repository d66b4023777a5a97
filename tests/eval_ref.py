"""CPU restatement (numpy + scipy) of the stage of reference eval.py between "two F0 tracks" and "the numbers": the
yardstick of tests/test_eval_ref_cpu.py, tests/test_eval_cpu.py and tests/test_gpu_prosody_metrics.py.

Restated from reference eval.py:50-57 (aligned_ffe), :96-102 (EMD with zero extension), :110-129 (the two tiers) and
utils.py:39-45 (interp), quirks included:
  * interp on a length-1 ndarray is ``target_len * vals``: a product of shape (1,), which broadcasts;
  * interp on an empty slice with a non-empty target raises ValueError (from scipy): the file drops out of the tier's FFE
    list AFTER its length error was appended;
  * an empty reference slice gives mean([]) = NaN, which goes into the mean over intervals;
  * the zero extension made for the EMD stays in place: the FFE slices are cut from the extended tracks.
tests/golden/make_eval_golden.py runs the reference's own functions on the same inputs; the test compares exactly.

Tracks are handled as float64 here (pYAAPT's samp_values are float64; the device's float32 values are widened)."""
import contextlib
import warnings

import numpy as np
from scipy.stats import wasserstein_distance


class Interval:
    """what the reference reads of a textgrid.Interval"""

    def __init__(self, minTime, maxTime, mark):
        self.minTime, self.maxTime, self.mark = minTime, maxTime, mark

    def duration(self):
        return self.maxTime - self.minTime


def nearest_map(cur_len, target_len):
    """index into a length-cur_len array (cur_len >= 2) for every point of linspace(0, 1, target_len), as
    scipy.interpolate.interp1d(kind='nearest') picks it: 'left' on a tie, i.e. the lower index wins"""
    x = np.arange(cur_len) * (1.0 / (cur_len - 1))
    x[-1] = 1.0
    mid = x[:-1] / 2.0 + x[1:] / 2.0
    if target_len > 1:
        x_new = np.arange(target_len) * (1.0 / (target_len - 1))
        x_new[-1] = 1.0
    else:
        x_new = np.zeros(target_len)
    return np.clip(np.searchsorted(mid, x_new, side="left"), 0, cur_len - 1).astype(np.intp)


def interp(vals, target_len):
    vals = np.asarray(vals, dtype=np.float64)
    cur_len = len(vals)
    if cur_len == 1:
        return target_len * vals  # shape (1,)
    if target_len == cur_len:
        return vals.copy()
    if cur_len == 0:
        raise ValueError("empty slice cannot be resampled")  # interp1d refuses empty x / y
    return vals[nearest_map(cur_len, target_len)]


def frame_index(t, sr=16000):
    """time of a TextGrid boundary -> index into the 5 ms track, in the reference's order of operations"""
    return int(t * sr * 0.005 * 2.5 + 2)


def slice_bounds(t_min, t_max, n, sr=16000):
    """the bounds numpy uses for track[frame_index(t_min):frame_index(t_max)] on a track of n frames: 0 <= lo <= hi <= n"""
    lo, hi, _ = slice(frame_index(t_min, sr), frame_index(t_max, sr)).indices(n)
    return lo, max(lo, hi)


def slice_ffe(ref, syn):
    """one interval: share of frames whose F0 differs by more than 20 %; ValueError / NaN as described above"""
    ref = np.asarray(ref, dtype=np.float64)
    syn = interp(syn, ref.shape[0])
    with np.errstate(invalid="ignore", divide="ignore"), _quiet():
        return (np.abs(((ref + 0.0001) / (syn + 0.0001)) - 1) > 0.2).mean()


@contextlib.contextmanager
def _quiet():
    """numpy's "mean of empty slice" warnings: the reference lets those NaNs through"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


def aligned_ffe(int_ref, int_syn, pitch_ref, pitch_syn, sr=16000):
    ffe = []
    for i in range(len(int_ref)):
        lo, hi = slice_bounds(int_ref[i].minTime, int_ref[i].maxTime, len(pitch_ref), sr)
        ref = pitch_ref[lo:hi]
        lo, hi = slice_bounds(int_syn[i].minTime, int_syn[i].maxTime, len(pitch_syn), sr)
        ffe.append(slice_ffe(ref, pitch_syn[lo:hi]))
    with _quiet():
        return np.mean(ffe)


def emd_lengths(n_ref_frames, n_syn_frames, n_ref_samples, n_syn_samples):
    """sizes (ref, syn) of the two samples after the reference's zero extension; its second branch tests the WAVEFORM
    lengths"""
    if n_ref_frames > n_syn_frames:
        return n_ref_frames, n_ref_frames
    if n_ref_samples < n_syn_samples:
        return n_syn_frames, n_syn_frames
    return n_ref_frames, n_syn_frames


def zero_extend(pitch_ref, pitch_syn, n_ref_samples, n_syn_samples):
    """the two tracks as the reference carries them on after eval.py:98-101 -- the FFE slices are cut from these
    zero-extended tracks too, not from the tracker's"""
    pitch_ref, pitch_syn = np.asarray(pitch_ref, np.float64), np.asarray(pitch_syn, np.float64)
    lr, ls = emd_lengths(len(pitch_ref), len(pitch_syn), n_ref_samples, n_syn_samples)
    return np.pad(pitch_ref, (0, lr - len(pitch_ref))), np.pad(pitch_syn, (0, ls - len(pitch_syn)))


def emd(pitch_ref, pitch_syn, n_ref_samples, n_syn_samples):
    ref, syn = zero_extend(pitch_ref, pitch_syn, n_ref_samples, n_syn_samples)
    return wasserstein_distance(syn, ref)


def tier_intervals(ref_tier, syn_tier, ref_max_time):
    """non-empty intervals of one tier of both grids; without a generated grid, uniform pseudo-intervals over the
    reference's maxTime (one slot per interval of the tier, empty ones included, plus one)"""
    ref_iv = [f for f in ref_tier if f.mark]
    if syn_tier is not None:
        syn_iv = [f for f in syn_tier if f.mark]
    else:
        n = len(ref_tier) + 1
        syn_iv = [Interval(ref_max_time / n * i, ref_max_time / n * (i + 1), inv.mark)
                  for i, inv in enumerate(ref_tier) if inv.mark]
    return ref_iv, syn_iv


def tier_len_error(ref_iv, syn_iv):
    """mean |duration difference|; ValueError when the counts differ (numpy cannot broadcast them)"""
    with _quiet():
        return np.abs(np.array([i.duration() for i in ref_iv]) - np.array([i.duration() for i in syn_iv])).mean()


def score_file(pitch_ref, pitch_syn, n_ref_samples, n_syn_samples, ref_grid, syn_grid, sr=16000):
    """one generated file -> dict with 'len', 'emd' and those of 'p_len', 'p_ffe', 'w_len', 'w_ffe' the reference
    would have appended.  ref_grid / syn_grid: objects with .maxTime and [tier] -> list of intervals (syn_grid may be
    None)."""
    out = {"len": abs(n_ref_samples - n_syn_samples), "emd": emd(pitch_ref, pitch_syn, n_ref_samples, n_syn_samples)}
    pitch_ref, pitch_syn = zero_extend(pitch_ref, pitch_syn, n_ref_samples, n_syn_samples)
    for key, tier in (("p", 1), ("w", 0)):
        try:
            ref_iv, syn_iv = tier_intervals(ref_grid[tier], syn_grid[tier] if syn_grid else None, ref_grid.maxTime)
            out[key + "_len"] = tier_len_error(ref_iv, syn_iv)
            out[key + "_ffe"] = aligned_ffe(ref_iv, syn_iv, pitch_ref, pitch_syn, sr)
        except ValueError:
            pass
    return out


# ---------------------------------------------------------------------------------------------------------
# synthetic inputs shared by tests/golden/make_eval_golden.py and the tests
# ---------------------------------------------------------------------------------------------------------
def synth_track(rng, n):
    """F0-like track of n frames: a slow sinusoid around 120 Hz plus 6 Hz noise, voiced in 25-frame runs with
    probability 0.6, exact zeros elsewhere (float32 like the tracker's output)"""
    t = np.arange(n)
    f0 = 120.0 + 25.0 * np.sin(2 * np.pi * t / 260.0 + rng.uniform(0, 6.28)) + 6.0 * rng.standard_normal(n)
    voiced = np.repeat(rng.random_sample(n // 25 + 1) < 0.6, 25)[:n]
    return np.where(voiced, f0, 0.0).astype(np.float32)


def synth_pair(rng, n_ref, n_syn):
    """a reference track and a 'generated' one: the same contour on another time axis, scaled by 1, 1.1 or 1.25, with
    its own noise"""
    ref = synth_track(rng, n_ref)
    idx = np.minimum((np.arange(n_syn) * (n_ref / n_syn)).astype(np.intp), n_ref - 1)
    syn = ref[idx].astype(np.float64) * rng.choice([1.0, 1.1, 1.25])
    syn = np.where(syn > 0, syn + 6.0 * rng.standard_normal(n_syn), 0.0).astype(np.float32)
    return ref, syn


def synth_cuts(rng, n_ref, n_syn, n_intervals):
    """interval times (seconds) [n_intervals, 4] = (ref min, ref max, syn min, syn max): consecutive pieces between
    sorted uniform cut times over each track's duration (a little beyond its end, so that some slices come out empty)"""
    out = np.empty((n_intervals, 4))
    for col, n in ((0, n_ref), (2, n_syn)):
        cuts = np.sort(rng.uniform(0.0, (n + 2) / 200.0, n_intervals + 1))
        out[:, col], out[:, col + 1] = cuts[:-1], cuts[1:]
    return out


def write_textgrid(path, max_time, tiers):
    """Praat long text format; tiers = [(name, boundaries [n + 1], marks [n])], times written with repr()"""
    lines = ['File type = "ooTextFile"', 'Object class = "TextGrid"', "", "xmin = 0", f"xmax = {max_time!r}",
             "tiers? <exists>", f"size = {len(tiers)}", "item []:"]
    for k, (name, times, marks) in enumerate(tiers):
        lines += [f"    item [{k + 1}]:", '        class = "IntervalTier"', f'        name = "{name}"', "        xmin = 0",
                  f"        xmax = {max_time!r}", f"        intervals: size = {len(marks)}"]
        for i, mark in enumerate(marks):
            lines += [f"        intervals [{i + 1}]:", f"            xmin = {float(times[i])!r}",
                      f"            xmax = {float(times[i + 1])!r}", '            text = "%s"' % mark.replace('"', '""')]
    with open(path, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
