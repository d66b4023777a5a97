#!/usr/bin/env python
"""One sha256 per case over the whole output buffer of every path that goes through the host launch interface (run_conv, the pair
and ResBlock launchers), for comparing two builds of the library bit for bit: run once per build in separate processes,
DISSC_HIP_LIB naming the other build, and diff the two outputs (tools/pair_digest.py does the same for dissc_respair1d alone).
  the generator at test size (tests/test_gpu_generator.py: synth_generator_inputs(6, 41, seed=21, ragged=True)) under the default
    options, multistream = 0, wino = 0, pair_max_c = 0 with pair_dma = 1 / 0, precision = 1, and one B = 1, T = 100 forward;
  a ragged three-utterance HuBERT encode in fp32 and split-bf16; one forward of each predictor kind; nn.conv1d forward and
  backward; one YAAPT track.  Seconds per run."""
import ctypes
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dissc_amd  # noqa: E402
import synthdata as synth  # noqa: E402
from dissc_amd._lib import lib  # noqa: E402

DEV = "cuda:0"


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update((t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)).tobytes())
    return h.hexdigest()


def generator(precision=None, B=6, T=41, **options):
    """a handle created under `options` (the native handle takes its snapshot and its plan when it is created, which CodeGenerator
    does inside its first forward: hence inside this try block), the defaults restored afterwards"""
    saved = {}
    try:
        for k, v in options.items():
            cur = ctypes.c_int(0)
            assert lib.dissc_get_option(k.encode(), ctypes.byref(cur)) == 0, k
            saved[k] = cur.value
            assert lib.dissc_set_option(k.encode(), v) == 0, k
        g = dissc_amd.CodeGenerator(synth.VCTK_CONFIG, precision=precision).to(DEV)
        g.load_state_dict(synth.synth_generator_state_dict(seed=0))
        g.eval().remove_weight_norm()
        if B == 1:
            code, f0, spkr, _ = synth.synth_generator_inputs(1, T, seed=21)
            y = g(code=torch.from_numpy(code), f0=torch.from_numpy(f0), spkr=torch.from_numpy(spkr))
        else:
            code, f0, spkr, lengths = synth.synth_generator_inputs(B, T, seed=21, ragged=True)
            y = g(code=torch.from_numpy(code), f0=torch.from_numpy(f0), spkr=torch.from_numpy(spkr), lengths=torch.from_numpy(lengths))
        torch.cuda.synchronize()
        return sha(y)
    finally:
        for k, v in saved.items():
            lib.dissc_set_option(k.encode(), v)


def hubert(precision):
    from dissc_amd.hubert import HubertEncoder
    enc = HubertEncoder(synth.synth_hubert_state_dict(6), synth.synth_kmeans_centers(), n_layers=6, precision=precision).to(DEV)
    ns = [16000, 4000, 719]
    wav = torch.full((len(ns), max(ns)), float("nan"))
    for i, n in enumerate(ns):
        wav[i, :n] = torch.from_numpy(synth.synth_waveform(n, seed=n))
    out = enc(wav, n_samples=torch.tensor(ns))
    return sha(out["dense"], out["units"], out["frames"])


def predictors():
    from dissc_amd import predictors as P
    rs = np.random.RandomState(3)
    lens = torch.tensor([57, 23, 1], dtype=torch.int32)
    seq = torch.from_numpy(rs.randint(0, 100, (3, 57)).astype(np.int64))
    spk = torch.from_numpy(rs.randint(0, 108, (3, 1)).astype(np.int64))
    lm = P.LenPredictor(n_tokens=100, n_speakers=108).to(DEV)
    lm.load_state_dict(synth.synth_len_state_dict(100, 108))
    lm.eval()
    lm.norm_mean, lm.norm_std = synth.synth_len_norm_stats()
    yield "len", sha(lm(seq, spk, lengths=lens))
    g = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "pred.npz"))
    id2m, id2s = torch.from_numpy(g["id2pitch_mean"]), torch.from_numpy(g["id2pitch_std"])
    for kind, cls in (("new", P.PitchPredictor), ("base", P.PitchPredictorBase)):
        pm = cls(100, 108, id2pitch_mean=id2m, id2pitch_std=id2s).to(DEV)
        pm.load_state_dict(synth.synth_pitch_state_dict(kind, 100, 108))
        pm.eval()
        yield f"pitch-{kind}", sha(pm.infer_freq(seq, spk, True, lengths=lens))


def nn_conv1d():
    from dissc_amd import nn
    rs = np.random.RandomState(11)
    cin, cout, k, d, B, ld = 48, 80, 7, 3, 3, 300
    x = torch.from_numpy(rs.randn(B, cin, ld).astype(np.float32)).to(DEV).requires_grad_(True)
    w = torch.from_numpy((rs.uniform(-1, 1, (cout, cin, k)) / np.sqrt(cin * k)).astype(np.float32)).to(DEV).requires_grad_(True)
    b = torch.from_numpy(rs.uniform(-1, 1, cout).astype(np.float32)).to(DEV).requires_grad_(True)
    add = torch.from_numpy(rs.randn(B, cout, ld).astype(np.float32)).to(DEV).requires_grad_(True)
    ln = torch.tensor([300, 133, 1], dtype=torch.int32, device=DEV)
    y = nn.conv1d(x, w, b, lengths=ln, dilation=d, in_slope=0.1, add=add)
    y.backward(torch.from_numpy(rs.randn(B, cout, ld).astype(np.float32)).to(DEV))
    torch.cuda.synchronize()
    return sha(y, x.grad, w.grad, b.grad, add.grad)


def yaapt():
    from dissc_amd.f0 import YaaptTracker
    t = np.arange(24000) / 16000.0
    f = 140 + 30 * np.sin(2 * np.pi * 2 * t)
    sig = sum(np.sin(2 * np.pi * h * np.cumsum(f) / 16000.0) / h for h in (1, 2, 3)) * 0.2
    return sha(*YaaptTracker(device=DEV)([sig, sig[:9000]]))


def main():
    cases = [("generator default", lambda: generator()),
             ("generator multistream=0", lambda: generator(multistream=0)),
             ("generator wino=0", lambda: generator(wino=0)),
             ("generator pair_max_c=0 pair_dma=1", lambda: generator(pair_max_c=0, pair_dma=1)),
             ("generator pair_max_c=0 pair_dma=0", lambda: generator(pair_max_c=0, pair_dma=0)),
             ("generator precision=1", lambda: generator(precision="split_bf16")),
             ("generator B=1 T=100", lambda: generator(B=1, T=100)),
             ("hubert fp32", lambda: hubert("fp32")),
             ("hubert split_bf16", lambda: hubert("split_bf16")),
             ("nn.conv1d forward+backward", nn_conv1d),
             ("yaapt", yaapt)]
    for name, fn in cases:
        print(f"{name} {fn()}", flush=True)
    for name, d in predictors():
        print(f"predictor {name} {d}", flush=True)


if __name__ == "__main__":
    main()
