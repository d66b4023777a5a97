"""Golden vectors of the prosody metrics, from the REFERENCE's own eval.py / utils.py (this container only).

    python tests/golden/make_eval_golden.py      # writes tests/golden/eval_prosody.npz

The reference's eval.py is imported unmodified with stub modules in place of the libraries that are not installed
(whisper, torchaudio, amfm_decompy, librosa, textgrid, editdistance, tensorflow); what it computes with numpy and scipy
runs for real.  Two parts:
  * intervals: ``aligned_ffe`` on one interval at a time over synthetic tracks (tests/eval_ref.py's recipe), with the
    three quirk cases added by hand: per interval the value (NaN included) or the ValueError;
  * files: ``calc_errors`` on a results tree of empty WAVs whose "audio" carries an index into the stored tracks
    (torchaudio.load, get_yaapt and TextGrid.fromFile are the stubs that hand the injected data over), with a
    generated file without a grid, one with another phone count, the skip rules and both EMD padding branches.
Nothing of the reference's source is stored: inputs, the tree's description and the reference's results only.
"""
import argparse
import glob as _glob
import json
import os
import sys
import tempfile
import types
import warnings

import numpy as np

warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
OUT = os.environ.get("DISSC_GOLDEN_OUT", HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import eval_ref as er  # noqa: E402  (the shared synthetic-input recipe and the Interval stand-in)


class _Grid:
    """stand-in for textgrid.TextGrid: maxTime and tiers of intervals"""

    def __init__(self, max_time, tiers):
        self.maxTime, self.tiers = max_time, tiers

    def __len__(self):
        return len(self.tiers)

    def __getitem__(self, i):
        return self.tiers[i]


def import_reference():
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    stub("whisper")
    stub("editdistance", eval=lambda a, b: 0)
    stub("torchaudio")
    stub("tensorflow", summary=None)
    stub("amfm_decompy")
    stub("amfm_decompy.pYAAPT")
    stub("amfm_decompy.basic_tools")
    stub("librosa")
    stub("librosa.util", normalize=lambda x: x)
    stub("textgrid", Interval=er.Interval, TextGrid=types.SimpleNamespace())
    sys.path.insert(0, REF)
    import eval as ref_eval  # reference eval.py
    import utils as ref_utils  # reference utils.py
    return ref_eval, ref_utils


def tier(times, marks):
    return [er.Interval(float(a), float(b), m) for a, b, m in zip(times[:-1], times[1:], marks)]


def grid_arrays(rng, duration, n_words, phones_per_word=3, silent=(0,)):
    """boundaries and marks of a words tier and a phones tier over [0, duration]; the intervals named in `silent`
    (word indices) get an empty mark, like MFA's silences"""
    w = np.concatenate([[0.0], (np.arange(1, n_words) + rng.uniform(-0.3, 0.3, n_words - 1)) * duration / n_words,
                        [duration]]).round(4)
    wm = ["" if i in silent else f"w{i}" for i in range(n_words)]
    p, pm = [0.0], []
    for i in range(n_words):
        k = np.arange(1, phones_per_word) + rng.uniform(-0.3, 0.3, phones_per_word - 1)
        inner = w[i] + (w[i + 1] - w[i]) * k / phones_per_word if wm[i] else np.zeros(0)
        p += list(inner.round(4)) + [w[i + 1]]
        pm += [f"p{i}{j}" if wm[i] else "" for j in range(len(inner) + 1)]
    return w, wm, np.array(p), pm


def make_intervals(ref_eval, rng):
    tracks, n_frames, rows, times = [], [], [], []
    for _ in range(40):
        n_ref, n_syn = (int(v) for v in rng.randint(300, 901, 2))
        ref, syn = er.synth_pair(rng, n_ref, n_syn)
        cuts = er.synth_cuts(rng, n_ref, n_syn, 8)
        tracks += [ref, syn]
        n_frames += [n_ref, n_syn]
        rows += [(len(tracks) - 2, len(tracks) - 1)] * len(cuts)
        times += list(cuts)
    # by hand, on the first pair: length-1 generated slices (voiced / unvoiced frame), an empty generated slice, an empty
    # reference slice, both empty, equal lengths, a generated slice of 2 frames against a long reference
    v = int(np.flatnonzero(tracks[1] > 0)[0])
    u = int(np.flatnonzero(tracks[1] == 0)[0])
    f = lambda i: (i - 2 + 0.5) / 200.0  # a time whose frame index is i  # noqa: E731
    for a, b, c, d in ((10, 40, v, v + 1), (10, 40, u, u + 1), (50, 51, v, v + 1), (10, 30, 60, 60), (30, 30, 10, 50),
                       (30, 30, 40, 40), (100, 160, 120, 180), (20, 140, 33, 35), (0, n_frames[0] + 50, 0, n_frames[1] + 50)):
        rows.append((0, 1))
        times.append((f(a), f(b), f(c), f(d)))
    ffe, status = [], []
    for (rr, rs), t in zip(rows, times):
        one_r, one_s = [er.Interval(t[0], t[1], "x")], [er.Interval(t[2], t[3], "x")]
        try:
            ffe.append(ref_eval.aligned_ffe(one_r, one_s, tracks[rr].astype(np.float64), tracks[rs].astype(np.float64)))
            status.append(0)
        except ValueError:
            ffe.append(np.nan)
            status.append(1)
    F = max(n_frames)
    return {"iv_tracks": np.stack([np.pad(t, (0, F - len(t))) for t in tracks]).astype(np.float32),
            "iv_n_frames": np.array(n_frames, np.int32), "iv_rows": np.array(rows, np.int32),
            "iv_times": np.array(times, np.float64), "iv_ffe": np.array(ffe, np.float64),
            "iv_status": np.array(status, np.int32)}


def make_files(ref_eval, rng):
    """-> arrays + a JSON description of the tree; runs the reference's calc_errors over it"""
    import torch
    tracks, samples = [], []

    def wave(n_frames_, n_samples):
        tracks.append(er.synth_track(rng, n_frames_))
        samples.append(n_samples)
        return len(tracks) - 1

    def grid(duration, n_words, silent=(0,), phones_per_word=3):
        w, wm, p, pm = grid_arrays(rng, duration, n_words, phones_per_word, silent)
        return {"maxTime": float(duration), "w": [list(map(float, w)), wm], "p": [list(map(float, p)), pm]}

    orig = {"p231_001": (wave(400, 63700), grid(2.0, 6)), "p231_002": (wave(380, 60500), grid(1.9, 5, silent=(0, 4))),
            "p231_024": (wave(300, 47700), grid(1.5, 4)), "p270_003": (wave(350, 55700), grid(1.75, 5))}
    g1 = orig["p231_001"][1]
    other_phones = grid(2.1, 6, phones_per_word=2)
    other_phones["w"] = [[round(t * 1.05, 4) for t in g1["w"][0]], g1["w"][1]]  # same words, other phone count
    late = grid(1.9, 5, silent=(0, 4))
    late["p"][0] = [round(t + 5.0, 4) for t in late["p"][0]]  # phones beyond the generated track: empty generated slices
    gen = {
        "p231": {"p225_001": (wave(380, 60500), grid(1.9, 6)),        # shorter than the reference: first EMD branch
                 "p226_001": (wave(430, 68500), None),                # no grid: pseudo-intervals; second EMD branch
                 "p227_001": (wave(420, 66900), other_phones),        # another phone count: phones dropped, words kept
                 "p231_001": (wave(400, 63700), grid(2.0, 6)),        # reconstruction: skipped
                 "p228_009": (wave(300, 47700), grid(1.5, 4)),        # no reference recording: skipped
                 "p270_024": (wave(300, 47700), grid(1.5, 4)),        # the file the reference excludes by name
                 "p232_001": (wave(410, 63000), grid(2.05, 6)),       # more frames, shorter waveform: no padding at all
                 "p229_002": (wave(380, 61000), late),                # equal frames, longer waveform; ValueError in p_ffe
                 "p230_002": (wave(200, 31700), grid(1.0, 5, silent=(0, 4)))},  # much shorter: NaN / length-1 territory
        "p270": {"p225_003": (wave(350, 55700), grid(1.75, 5)),
                 "p270_003": (wave(350, 55700), grid(1.75, 5))},      # reconstruction: skipped
    }

    def to_grid(g):
        return _Grid(g["maxTime"], [tier(np.array(g["w"][0]), g["w"][1]), tier(np.array(g["p"][0]), g["p"][1])])

    with tempfile.TemporaryDirectory() as tmp:
        by_path = {}

        def put(folder, name, idx, g):
            os.makedirs(os.path.join(tmp, folder, "txtgrid"), exist_ok=True)
            wav = os.path.join(tmp, folder, name + ".wav")
            open(wav, "wb").close()
            with open(os.path.join(tmp, folder, name + ".txt"), "w") as f:
                f.write("text\n")
            by_path[os.path.normpath(wav)] = idx
            if g is not None:
                tg = os.path.join(tmp, folder, "txtgrid", name + ".TextGrid")
                open(tg, "w").close()
                by_path[os.path.normpath(tg)] = g

        for name, (idx, g) in orig.items():
            put("orig", name, idx, g)
        for trg, files in gen.items():
            for name, (idx, g) in files.items():
                put(os.path.join("sr", trg), name, idx, g)

        def load(path):  # "audio" = zeros with the track's index in sample 0
            idx = by_path[os.path.normpath(str(path))]
            x = torch.zeros(1, samples[idx])
            x[0, 0] = idx
            return x, 16000

        ref_eval.torchaudio.load = load
        ref_eval.get_yaapt = lambda audio: tracks[int(audio[0])].astype(np.float64)
        ref_eval.textgrid.TextGrid.fromFile = lambda path: to_grid(by_path[os.path.normpath(str(path))])
        real_glob = _glob.glob
        ref_eval.glob = types.SimpleNamespace(glob=lambda pat: sorted(real_glob(pat)))  # a fixed file order
        asr = types.SimpleNamespace(transcribe=lambda f: {"text": "text"})
        args = argparse.Namespace(base_path=tmp, method="sr", target_speakers=["p231", "p270"])
        err = ref_eval.calc_errors(asr, args)
    F = max(len(t) for t in tracks)
    tree = {"orig": {k: {"track": v[0], "grid": v[1]} for k, v in orig.items()},
            "gen": {trg: {k: {"track": v[0], "grid": v[1]} for k, v in files.items()} for trg, files in gen.items()}}
    out = {"file_tracks": np.stack([np.pad(t, (0, F - len(t))) for t in tracks]).astype(np.float32),
           "file_n_frames": np.array([len(t) for t in tracks], np.int32), "file_samples": np.array(samples, np.int64),
           "file_tree": np.array(json.dumps(tree))}
    for k in ("len", "emd", "p_len", "p_ffe", "w_len", "w_ffe"):
        out["res_" + k] = np.array(err[k], np.float64)
    return out


def main():
    ref_eval, ref_utils = import_reference()
    rng = np.random.RandomState(20240)
    out = make_intervals(ref_eval, rng)
    out.update(make_files(ref_eval, rng))
    # utils.interp itself on the quirk inputs, as recorded facts
    out["interp_len1"] = np.asarray(ref_utils.interp(np.array([100.0]), 4), np.float64)
    try:
        ref_utils.interp(np.zeros(0), 3)
        out["interp_empty_raises"] = np.array(0)
    except ValueError:
        out["interp_empty_raises"] = np.array(1)
    np.savez_compressed(os.path.join(OUT, "eval_prosody.npz"), **out)
    n = len(out["iv_ffe"])
    f = out["iv_ffe"]
    print(f"intervals {n}: 0<ffe<1 {np.mean((f > 0) & (f < 1)):.2f}, nan {np.mean(np.isnan(f) & (out['iv_status'] == 0)):.3f}, "
          f"ValueError {np.mean(out['iv_status'] == 1):.3f}")
    for k in ("len", "emd", "p_len", "p_ffe", "w_len", "w_ffe"):
        print(k, out["res_" + k])


if __name__ == "__main__":
    main()
