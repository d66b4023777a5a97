#!/usr/bin/env python
"""HuBERT unit-encode timing: B x seconds of synthetic audio through dissc_amd.hubert.HubertEncoder.
    python tools/encode_bench.py [--utts 32 --seconds 10 --iters 10] [--precision split_bf16] [--ragged] [--alternate 3]
Prints one JSON line per run (ms per batch, x real time, algorithmic TFLOP/s, the units' checksum).
--ragged: the B = 32 ragged 2 .. 10 s batch of tests/test_gpu_hubert_trained_like.py (lengths only; iid audio and checkpoint).
--alternate N: fp32 and split_bf16 by turns, N runs each in ONE process (the spread between the repeats is the noise a
difference between the modes has to exceed)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dissc_amd.hubert import HubertEncoder  # noqa: E402
import synthdata as synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--utts", type=int, default=32)
ap.add_argument("--seconds", type=float, default=10.0)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--precision", default=None, choices=["fp32", "split_bf16"])
ap.add_argument("--ragged", action="store_true")
ap.add_argument("--alternate", type=int, default=0)
a = ap.parse_args()
n = int(a.seconds * 16000)
if a.ragged:
    rs = np.random.RandomState(12)
    ns = [160000] + [int(v) for v in rs.randint(32000, 160001, size=30)] + [32000]
    n, a.utts = max(ns), len(ns)
    wav = torch.zeros(a.utts, n)
    for i, k in enumerate(ns):
        wav[i, :k] = torch.from_numpy(synth.synth_waveform(k, seed=i))
    wav, n_samples, audio_s = wav.cuda(), torch.tensor(ns), sum(ns) / 16000.0
else:
    wav = torch.stack([torch.from_numpy(synth.synth_waveform(n, seed=i)) for i in range(a.utts)]).cuda()
    n_samples, audio_s = None, a.utts * a.seconds
sd, centers = synth.synth_hubert_state_dict(6), synth.synth_kmeans_centers()


def run(enc, precision):
    for _ in range(3):
        out = enc(wav, n_samples=n_samples, want_dense=False)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        out = enc(wav, n_samples=n_samples, want_dense=False)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.iters
    # algorithmic FLOPs per utterance (conv feature extractor 49.1 + encoder 52.1 GFLOP per 10 s)
    gflop = 101.2 * audio_s / 10.0
    res = {"utts": a.utts, "seconds": a.seconds, "ms_per_batch": round(ms, 3),
           "x_realtime": round(audio_s / ms * 1e3, 1), "tflops": round(gflop / ms, 1),
           "units_checksum": int(out["units"].sum())}
    if precision is not None or a.ragged:
        res.update(precision=precision or "default", ragged=a.ragged)
    print(json.dumps(res), flush=True)


if a.alternate > 0:
    encs = {p: HubertEncoder(sd, centers, 6, precision=p).to("cuda:0") for p in ("fp32", "split_bf16")}
    for _ in range(a.alternate):
        for p, enc in encs.items():
            run(enc, p)
else:
    run(HubertEncoder(sd, centers, 6, precision=a.precision).to("cuda:0"), a.precision)
