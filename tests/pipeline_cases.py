"""Shared by tests/test_gpu_pipeline.py and tests/test_gpu_multigpu.py (not a test module): the synthetic models on the GPU, the
model / wav trees the CLIs read, the sweep's jobs, a free port and a checked subprocess run."""
import json
import os
import shutil
import socket
import subprocess

import numpy as np
import pytest
import torch
from scipy.io import wavfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture(scope="module")
def models():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import synthdata as synth
    import dissc_amd
    from dissc_amd import predictors as P
    from dissc_amd.hubert import HubertEncoder
    m = {"hsd": synth.synth_hubert_state_dict(6), "centers": synth.synth_kmeans_centers(),
         "lsd": synth.synth_len_state_dict(100, 108), "lstats": synth.synth_len_norm_stats(),
         "psd": synth.synth_pitch_state_dict("new", 100, 108), "gsd": synth.synth_generator_state_dict(seed=0)}
    m["enc"] = HubertEncoder(m["hsd"], m["centers"], 6).to(DEV)
    lm = P.LenPredictor(100, 108).to(DEV)
    lm.load_state_dict(m["lsd"])
    lm.norm_mean, lm.norm_std = m["lstats"]
    pm = P.PitchPredictor(100, 108).to(DEV)
    pm.load_state_dict(m["psd"])
    g = dissc_amd.CodeGenerator(synth.VCTK_CONFIG).to(DEV)
    g.load_state_dict(m["gsd"])
    g.eval().remove_weight_norm()
    m.update(lm=lm, pm=pm, g=g)
    return m


def _sweep_jobs(n_utts, targets, seed=3):
    import synthdata as synth
    rs = np.random.RandomState(seed)
    jobs = []
    for u in range(n_utts):
        T = int(rs.randint(100, 251))
        code, f0, _, _ = synth.synth_generator_inputs(1, T, seed=5000 + u)
        for t in targets:
            jobs.append(dict(code=code[0], f0=f0[0, 0], spkr=t))
    return jobs


def _write_models(td, models, golden_dir, f0_normalize=False):
    import pickle
    import synthdata as synth
    for d in ("hub", "len", "pitch", "ckpt", "meta"):
        os.makedirs(f"{td}/{d}")
    torch.save({"model": models["hsd"]}, f"{td}/hub/hubert-base-ls960.pt")
    np.save(f"{td}/hub/kmeans_100.npy", models["centers"].numpy())
    torch.save(models["lsd"], f"{td}/len/best_model.pth")
    torch.save(models["lstats"], f"{td}/len/len_norm_stats.pth")
    torch.save(models["psd"], f"{td}/pitch/best_model.pth")
    shutil.copy(os.path.join(golden_dir, "vctk_id_to_spkr.pkl"), f"{td}/meta/id_to_spkr.pkl")
    cfg = dict(synth.VCTK_CONFIG, input_training_file=f"{td}/meta/train.txt", f0_normalize=False, f0_stats=None)
    if f0_normalize:
        # the shipped configs' mode (reference sr/configs/VCTK/hubert100_lut.json: f0_normalize + f0_stats): per
        # SOURCE speaker statistics, a global fallback for speakers the pickle does not know, median fill
        st = {"src0": {"mean": np.float64(0.21), "std": np.float64(1.7)},
              "src1": {"mean": np.float64(-0.4), "std": np.float64(0.6)},
              "f0_mean": np.float64(0.05), "f0_std": np.float64(1.3)}
        pickle.dump(st, open(f"{td}/meta/f0_stats_src.pkl", "wb"))
        cfg.update(f0_normalize=True, f0_stats=f"{td}/meta/f0_stats_src.pkl", f0_median=True)
    json.dump(cfg, open(f"{td}/ckpt/config.json", "w"))
    torch.save({"generator": models["gsd"]}, f"{td}/ckpt/g_00000001")


def _write_wavs(wav_dir, n, seed=7, lo=1.0, hi=4.0):
    import synthdata as synth
    os.makedirs(wav_dir)
    rs = np.random.RandomState(seed)
    names = []
    for i in range(n):
        ns = int(rs.uniform(lo, hi) * 16000)
        x = synth.synth_waveform(ns, seed=300 + i)
        nm = f"src{i % 5}_{i:03d}.wav"
        wavfile.write(os.path.join(wav_dir, nm), 16000, np.round(x * 32767).astype(np.int16))
        names.append(nm)
    return names


def _run(cmd, env, cwd, timeout=1500):
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout, cwd=cwd)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r
