"""Stage times of eval.py's scoring on a synthetic results tree of the VCTK sweep's shape (cfg5: 4 target speakers x
108 source speakers x 24 utterances = 10 368 generated files of about 3.5 s, 96 originals, TextGrids with ~11 words /
~33 phones each):

    python tools/eval_bench.py [--files 10368] [--cpu_files 1024] [--batch_seconds 640]

prints the wall seconds of the file reads (WAVs and TextGrids), the F0 tracking, the metric stage (the two launches and
their D2H copies) and the host's bookkeeping (interval tables, means) of dissc_amd.metrics.ProsodyEvaluator, and for
comparison the same metrics through tests/eval_ref.py (numpy + scipy, one file at a time) on tracks copied back to the
host, measured on --cpu_files files and scaled to the whole tree.  One JSON line at the end.  The numbers of record are in profiles/eval_prosody.md.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
from scipy.io import wavfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

FS = 16000


def utterance(rng, seconds):
    """speech-like enough for the tracker: 12 harmonics of a wandering F0, voiced in stretches, a little noise"""
    n = int(seconds * FS)
    t = np.arange(n) / FS
    f0 = rng.uniform(90, 220) * (1 + 0.15 * np.sin(2 * np.pi * rng.uniform(0.3, 1.0) * t + rng.uniform(0, 6.28)))
    ph = 2 * np.pi * np.cumsum(f0) / FS
    x = sum(np.sin(k * ph + 0.3 * k) / k for k in range(1, 13))
    gate = np.repeat(rng.random_sample(n // 2000 + 1) < 0.65, 2000)[:n]
    gate = np.convolve(gate.astype(np.float64), np.ones(160) / 160, mode="same")
    return (0.3 * x * gate + 0.002 * rng.standard_normal(n)).astype(np.float32)


def grid_tiers(rng, dur, n_words=11, ppw=3):
    w = np.concatenate([[0.0], (np.arange(1, n_words + 2) + rng.uniform(-0.3, 0.3, n_words + 1)) * dur / (n_words + 3),
                        [dur]]).round(4)
    wm = [""] + [f"w{i}" for i in range(n_words)] + [""]
    p, pm = [0.0], []
    for i, m in enumerate(wm):
        k = ppw if m else 1
        p += list(np.linspace(w[i], w[i + 1], k + 1)[1:].round(4))
        pm += [f"{m}{j}" if m else "" for j in range(k)]
    return [("words", w, wm), ("phones", p, pm)]


def build_tree(root, n_files, rng):
    import eval_ref as er
    targets, n_seq = ["p231", "p239", "p245", "p270"], 24
    pool = [utterance(rng, rng.uniform(2.5, 4.5)) for _ in range(64)]

    def put(folder, name, x):
        os.makedirs(os.path.join(root, folder, "txtgrid"), exist_ok=True)
        wavfile.write(os.path.join(root, folder, name + ".wav"), FS, np.round(x * 20000).astype(np.int16))
        er.write_textgrid(os.path.join(root, folder, "txtgrid", name + ".TextGrid"), round(len(x) / FS, 4),
                          grid_tiers(rng, round(len(x) / FS, 4)))

    for trg in targets:
        for s in range(1, n_seq + 1):
            put("orig", f"{trg}_{s:03d}", pool[rng.randint(len(pool))])
    made, src = 0, 0
    while made < n_files:
        for trg in targets:
            for s in range(1, n_seq + 1):
                if made < n_files:
                    put(os.path.join("sr", trg), f"s{300 + src}_{s:03d}", pool[rng.randint(len(pool))])
                    made += 1
        src += 1
    return targets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=10368)
    ap.add_argument("--cpu_files", type=int, default=1024)
    ap.add_argument("--batch_seconds", type=float, default=640.0)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    import torch
    import eval as dissc_eval
    import eval_ref as er
    from dissc_amd import metrics
    from dissc_amd.textgrid import TextGrid

    rng = np.random.RandomState(0)
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        targets = build_tree(root, a.files, rng)
        print(f"tree of {a.files} generated files written in {time.perf_counter() - t0:.1f} s", flush=True)
        args = argparse.Namespace(base_path=root, method="sr", target_speakers=targets)
        ev = metrics.ProsodyEvaluator(a.device, batch_seconds=a.batch_seconds)
        warm = dissc_eval.find_jobs(args)[:8]
        ev.evaluate(warm)  # library load, first launches, page-locked staging
        ev.timings = {}
        t0 = time.perf_counter()
        jobs = dissc_eval.find_jobs(args)
        rows = ev.evaluate(jobs)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        gpu = dict(ev.timings)

        # the same numbers on the host: tracks copied back, numpy + scipy per file
        ev.timings = None
        sub = jobs[:a.cpu_files]
        waves = {p: metrics.load_wav(p)[0] for j in sub for p in j[:2]}
        names = list(waves)
        f0 = dict(zip(names, ev.tracker([metrics.peak_normalize(waves[p]) for p in names])))
        grids = {p: TextGrid.fromFile(p) for j in sub for p in j[2:] if p}
        t0 = time.perf_counter()
        cpu_rows = [er.score_file(f0[r], f0[s], len(waves[r]), len(waves[s]), grids[rg], grids[sg] if sg else None)
                    for r, s, rg, sg in sub]
        cpu = time.perf_counter() - t0
    agree = all(np.array_equal(np.asarray(g.get(k, np.nan)), np.asarray(c.get(k, np.nan)), equal_nan=True)
                for g, c in zip(rows, cpu_rows) for k in ("len", "p_len", "p_ffe", "w_len", "w_ffe"))
    emd_rel = max(abs(g["emd"] - c["emd"]) / c["emd"] for g, c in zip(rows, cpu_rows) if c["emd"] > 0)
    audio = sum(len(w) for w in waves.values()) / FS / max(len(waves), 1)
    res = {"files": len(jobs), "total_s": round(total, 3), "read_s": round(gpu.get("read", 0.0), 3),
           "track_s": round(gpu.get("track", 0.0), 3), "metrics_s": round(gpu.get("metrics", 0.0), 3),
           "host_tables_s": round(total - sum(gpu.values()), 3),
           "metrics_over_track": round(gpu.get("metrics", 0.0) / gpu.get("track", 1.0), 3),
           "cpu_files": len(sub), "cpu_eval_ref_s": round(cpu, 3),
           "cpu_eval_ref_scaled_s": round(cpu / max(len(sub), 1) * len(jobs), 2), "mean_file_s": round(audio, 2),
           "ffe_len_equal_on_cpu_files": bool(agree), "emd_max_rel_diff": float(emd_rel),
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
