"""BASELINE.json configs[1], [3], [4] on the GPU, checked against the ORACLE chain (not against this
repo's own CLIs): the full encode -> predict -> resynthesise pipeline on 8 x 10 s utterances, a
256-utterance ragged many-to-many sweep through the resynthesis harness, and the rank-sharded
pipeline (2 ranks sharing this box's GPU over gloo) against the 1-rank run and the file-based chain.
"""
import importlib.util
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from pipeline_cases import DEV, ROOT, _free_port, _run, _sweep_jobs, _write_models, _write_wavs, models  # noqa: F401  (models: the module fixture)

pytestmark = pytest.mark.gpu


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, rel))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_cfg2_full_pipeline_8x10s_against_oracle_chain(models):
    """configs[1]: 8 x 10 s utterances, encode -> (--pred_len --pred_pitch, target p231) -> resynth on
    one GPU.  Stage by stage against oracle.hubert_ref.encode -> predictors_ref.infer_sample ->
    generator_ref.code_generator on 2 utterances (each stage of the oracle is fed the HIP output of
    the stage before, so that a legitimate k-means near-tie cannot hide a later difference); size-
    independent properties and bitwise batch-independence on all 8."""
    import synthdata as synth
    from oracle import generator_ref as gr, hubert_ref as hr, predictors_ref as pr
    from dissc_amd import predictors as P
    from dissc_amd.pipeline import Converter
    m = models
    N, tgt = 160000, 6  # p231
    waves = [synth.synth_waveform(N, seed=100 + i) for i in range(8)]
    conv = Converter(m["enc"], m["lm"], m["pm"], m["g"])
    raw = Converter(m["enc"], m["lm"], m["pm"], m["g"], postprocess=False)(waves, [tgt])
    out = conv(waves, [tgt])
    assert sorted(out) == [(i, tgt) for i in range(8)] == sorted(raw)

    # stage outputs of the HIP path, utterance by utterance (the reference's B=1 mode)
    enc = m["enc"](torch.from_numpy(np.stack(waves)), want_dense=True)
    units_hip = enc["units"].cpu()
    assert units_hip.shape == (8, 499)
    gw = gr.fold_state_dict(m["gsd"])
    for i in (0, 5):
        # (1) units: every frame where HIP and the oracle disagree is a k-means near-tie of the oracle
        u_ref, dense_ref = hr.encode(m["hsd"], m["centers"], torch.from_numpy(waves[i])[None])
        rel = float((enc["dense"][i].cpu() - dense_ref).norm() / dense_ref.norm())
        assert rel <= hr.FEAT_EPS_L2_REL, rel  # regression guard (<= 10x measured), see oracle/hubert_ref.py
        hr.check_units(units_hip[i].numpy(), u_ref.numpy(), dense_ref, m["centers"], x_dev=enc["dense"][i].cpu(),
                       tag=f"utt {i} (dense rel {rel:.2e})")
        # (2) rhythm + pitch on the HIP units: units/durations exact, F0 within fp32 noise
        ou, of0 = pr.infer_sample(units_hip[i].numpy(), tgt, m["lsd"], m["lstats"], m["psd"], "new", True)
        hu, hf0, _ = P.infer_samples([units_hip[i]], [tgt], m["lm"], m["pm"], norm_pitch=True, device=DEV)[0]
        assert hu == ou
        of0, hf0 = np.asarray(of0, np.float32), np.asarray(hf0, np.float32)
        flips = (of0 == 0) != (hf0 == 0)
        assert flips.sum() <= 1 and np.abs(of0[~flips] - hf0[~flips]).max() <= 2e-5
        # (3) generator on the HIP units/F0: waveform within the north-star tolerance (1e-4 RMS)
        code = torch.tensor(hu)[None]
        ref = gr.code_generator(gw, synth.VCTK_CONFIG, code, torch.from_numpy(hf0)[None, None], torch.tensor([[tgt]]))
        got = raw[(i, tgt)]
        assert got.shape == (320 * len(hu),)
        err = got.astype(np.float64) - ref[0, 0].numpy()
        rms, ref_rms = np.sqrt(np.mean(err ** 2)), float(ref.double().pow(2).mean().sqrt())
        assert rms <= 1e-4 and rms <= 1e-3 * ref_rms, (rms, ref_rms)
    # properties on all 8
    for i in range(8):
        r, o = raw[(i, tgt)], out[(i, tgt)]
        assert r.shape == o.shape and r.size % 320 == 0 and r.size > 0 and np.isfinite(r).all()
        # the post-processing of the pipeline == the oracle's int16-truncate + peak-normalise of the raw wave
        np.testing.assert_array_equal(o, gr.wav_postprocess(r))
        assert np.abs(o).max() == 1.0
        # batch independence: the utterance converted on its own (B=1 through every stage) is bit-identical
        alone = conv([waves[i]], [tgt])[(0, tgt)]
        np.testing.assert_array_equal(alone, o)


def test_cfg4_ragged_sweep_256_utterances_one_gpu(models):
    """configs[3]/[4]-shaped: 256 ragged utterances (T 100-250 frames) x 2 targets through
    harness.run_resynthesis: the oracle on a sample, batch-independence on ALL jobs (a different
    batching and, on a sample, B=1 must reproduce every waveform bit for bit)."""
    import synthdata as synth
    from oracle import generator_ref as gr
    from dissc_amd import harness
    jobs = _sweep_jobs(256, [6, 57])
    g = models["g"]
    waves = harness.run_resynthesis(g, jobs, device=DEV)
    assert sorted(waves) == list(range(512))
    other = harness.run_resynthesis(g, jobs, device=DEV, max_batch=7, max_frames=7 * 251)
    for j in range(512):
        assert waves[j].shape == (320 * len(jobs[j]["code"]),)
        np.testing.assert_array_equal(waves[j], other[j])
    rs = np.random.RandomState(0)
    gw = gr.fold_state_dict(models["gsd"])
    for j in rs.choice(512, 16, replace=False):
        j = int(j)
        one = harness.run_resynthesis(g, [jobs[j]], device=DEV)[0]
        np.testing.assert_array_equal(one, waves[j])
    for j in rs.choice(512, 4, replace=False):
        j = int(j)
        job = jobs[j]
        ref = gr.code_generator(gw, synth.VCTK_CONFIG, torch.from_numpy(job["code"])[None],
                                torch.from_numpy(job["f0"])[None, None], torch.tensor([[job["spkr"]]]))
        err = waves[j].astype(np.float64) - ref[0, 0].numpy()
        assert np.sqrt(np.mean(err ** 2)) <= 1e-4


@pytest.mark.parametrize("n_utts,f0_normalize", [(40, True), (8, False)])
def test_sharded_full_pipeline_two_ranks_equal_one_rank_and_file_chain(models, golden_dir, tmp_path, n_utts,
                                                                       f0_normalize):
    """convert.py (the rank-sharded encode -> predict -> resynthesise entry): 2 ranks (sharing this
    GPU, gloo instead of RCCL) must write byte-identical WAVs to the 1-rank run on 40 utterances x 2
    targets; and the 1-rank files equal the reference-style three-script chain through JSONL files --
    also with the vocoder config's f0_normalize / f0_stats / f0_median step switched on (the shipped
    configs' mode), which the chain applies in sr/inference.py and convert.py applies on the device."""
    td = str(tmp_path)
    _write_models(td, models, golden_dir, f0_normalize)
    names = _write_wavs(f"{td}/wav", n_utts)
    common = ["--base_dir", f"{td}/wav", "--hubert_dir", f"{td}/hub", "--len_model", f"{td}/len/", "--f0_model",
              f"{td}/pitch/", "--checkpoint_file", f"{td}/ckpt/", "--id_to_spkr", f"{td}/meta/id_to_spkr.pkl",
              "--target_speakers", "p231", "p225"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "convert.py")] + common + ["--output_dir", f"{td}/out1"],
                       env=env, capture_output=True, text=True, timeout=900, cwd=td)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    env2 = dict(env, DISSC_DIST_BACKEND="gloo")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                        os.path.join(ROOT, "convert.py")] + common + ["--output_dir", f"{td}/out2"],
                       env=env2, capture_output=True, text=True, timeout=900, cwd=td)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    files = sorted(os.listdir(f"{td}/out1"))
    assert len(files) == 2 * n_utts and sorted(os.listdir(f"{td}/out2")) == files
    for fn in files:
        assert open(f"{td}/out1/{fn}", "rb").read() == open(f"{td}/out2/{fn}", "rb").read(), fn
    # the same conversion through the three file-based entry points
    os.makedirs(f"{td}/enc")
    shutil.copy(f"{td}/meta/id_to_spkr.pkl", f"{td}/enc/id_to_spkr.pkl")
    _load("enc_cli_p", "data/encode.py").main(["--base_dir", f"{td}/wav", "--out_file", f"{td}/enc/val.txt",
                                               "--checkpoint_dir", f"{td}/hub", "--f0", "zeros"])
    _load("infer_cli_p", "infer.py").main(["--input_path", f"{td}/enc/val.txt", "--out_path", f"{td}/pred",
                                           "--pred_len", "--pred_pitch", "--len_model", f"{td}/len/", "--f0_model",
                                           f"{td}/pitch/", "--wild_sample", "--id_to_spkr", f"{td}/meta/id_to_spkr.pkl",
                                           "--f0_path", os.path.join(golden_dir, "vctk_f0_stats.pkl"), "--vc",
                                           "--target_speakers", "p231", "p225"])
    sr_cli = _load("sr_cli_p", "sr/inference.py")
    for t in ("p231", "p225"):
        sr_cli.main(["--input_code_file", f"{td}/pred/{t}_val.txt", "--data_path", f"{td}/wav", "--output_dir",
                     f"{td}/out3", "--checkpoint_file", f"{td}/ckpt/", "--vc", "--target-speakers", t,
                     "--unseen_speaker", "--id_to_spkr", f"{td}/meta/id_to_spkr.pkl", "-n", "-1"])
    got3 = sorted(f for f in os.listdir(f"{td}/out3") if f.endswith("_gen.wav"))
    assert got3 == files
    for fn in files:
        _, a = wavfile.read(f"{td}/out1/{fn}")
        _, b = wavfile.read(f"{td}/out3/{fn}")
        np.testing.assert_array_equal(a, b)


def test_sr_inference_256_utterances_two_ranks(models, golden_dir, tmp_path):
    """The resynthesis-only entry on a configs[3]-sized manifest: 256 ragged utterances x 2 targets,
    2 gloo ranks on this GPU == 1 rank, file for file."""
    td = str(tmp_path)
    _write_models(td, models, golden_dir)
    jobs = _sweep_jobs(256, [0])
    with open(f"{td}/man.txt", "w") as f:
        for u, j in enumerate(jobs):
            f.write(json.dumps({"units": j["code"].tolist(), "f0": [float(v) for v in j["f0"]],
                                "audio": f"p{225 + u % 7}_{u:03d}.wav"}) + "\n")
    args = ["--input_code_file", f"{td}/man.txt", "--data_path", f"{td}/nowav", "--checkpoint_file", f"{td}/ckpt/",
            "--vc", "--target-speakers", "p231", "p225", "--unseen_speaker", "--id_to_spkr",
            f"{td}/meta/id_to_spkr.pkl", "-n", "-1"]
    _load("sr_cli_256", "sr/inference.py").main(args + ["--output_dir", f"{td}/o1"])
    env = dict({k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")},
               DISSC_DIST_BACKEND="gloo")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                        os.path.join(ROOT, "sr", "inference.py")] + args + ["--output_dir", f"{td}/o2"],
                       env=env, capture_output=True, text=True, timeout=900, cwd=td)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    files = sorted(os.listdir(f"{td}/o1"))
    assert len(files) == 512 and sorted(os.listdir(f"{td}/o2")) == files
    for fn in files:
        assert open(f"{td}/o1/{fn}", "rb").read() == open(f"{td}/o2/{fn}", "rb").read(), fn
    # (o2: every rank wrote the files of the jobs it decoded, the N > 1 default.)  One writer instead -- rank 0 receives
    # every waveform of every round -- must produce the same bytes
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                        os.path.join(ROOT, "sr", "inference.py")] + args + ["--output_dir", f"{td}/o3"],
                       env=dict(env, DISSC_WRITERS="rank0"), capture_output=True, text=True, timeout=900, cwd=td)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted(os.listdir(f"{td}/o3")) == files
    for fn in files:
        assert open(f"{td}/o1/{fn}", "rb").read() == open(f"{td}/o3/{fn}", "rb").read(), fn


def test_cfg3_full_pipeline_256_esd_shaped_utterances(models, golden_dir, tmp_path):
    """BASELINE configs[3] at its stated size: the FULL pipeline (encode -> predict -> resynthesise) on 256
    ESD-shaped utterances (2-5 s) x 2 targets through convert.py: (a) one process, no process group; (b) two ranks
    sharing this GPU over gloo; (c) one rank with the collectives forced onto RCCL (DISSC_FORCE_DIST=1) AND the run cut
    into several gather-write-free rounds -- all three must write the same 512 files byte for byte."""
    td = str(tmp_path)
    _write_models(td, models, golden_dir, f0_normalize=True)
    _write_wavs(f"{td}/wav", 256, seed=11, lo=2.0, hi=5.0)
    common = ["--base_dir", f"{td}/wav", "--hubert_dir", f"{td}/hub", "--len_model", f"{td}/len/", "--f0_model",
              f"{td}/pitch/", "--checkpoint_file", f"{td}/ckpt/", "--id_to_spkr", f"{td}/meta/id_to_spkr.pkl",
              "--target_speakers", "p231", "p225"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "DISSC_FORCE_DIST")}
    conv = os.path.join(ROOT, "convert.py")
    _run([sys.executable, conv] + common + ["--output_dir", f"{td}/a"], env, td)
    _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
          "127.0.0.1", "--master-port", str(_free_port()), conv] + common + ["--output_dir", f"{td}/b"],
         dict(env, DISSC_DIST_BACKEND="gloo"), td)
    r = _run([sys.executable, conv] + common + ["--output_dir", f"{td}/c", "--round_seconds", "400"],
             dict(env, DISSC_FORCE_DIST="1", MASTER_PORT=str(_free_port()), NCCL_DEBUG="VERSION"), td)
    assert "512 waveforms written" in r.stdout
    files = sorted(os.listdir(f"{td}/a"))
    assert len(files) == 512 and sorted(os.listdir(f"{td}/b")) == files and sorted(os.listdir(f"{td}/c")) == files
    total = 0
    for fn in files:
        ref = open(f"{td}/a/{fn}", "rb").read()
        assert ref == open(f"{td}/b/{fn}", "rb").read(), fn
        assert ref == open(f"{td}/c/{fn}", "rb").read(), fn
        total += len(ref)
    assert total > 512 * 2000 * 4  # real conversions, not stubs (the synthetic rhythm model shortens the utterances)


def test_cfg5_full_vctk_sweep_10368_jobs(models):
    """BASELINE configs[4] at its stated size: 108 speakers x 24 utterances x 4 targets = 10 368
    generator jobs (2-5 s each, ~36 000 s of audio) through harness.run_resynthesis in bounded rounds.  Every job's
    waveform must be bitwise independent of the batching (two different batch plans, compared by digest on ALL jobs),
    B=1 reproduces a sample bit for bit, the oracle agrees on 4 jobs to 1e-4 RMS, and the exchange moves <= 1.1x
    the payload."""
    import hashlib
    import time
    import synthdata as synth
    from oracle import generator_ref as gr
    from dissc_amd import harness
    from dissc_amd.generator import wav_postprocess_
    rs = np.random.RandomState(9)
    targets = [6, 57, 3, 101]
    jobs = []
    for u in range(108 * 24):
        T = int(rs.randint(100, 251))
        code, f0, _, _ = synth.synth_generator_inputs(1, T, seed=20000 + u)
        for t in targets:
            jobs.append(dict(code=code[0], f0=f0[0, 0], spkr=t))
    assert len(jobs) == 10368
    keep_ids = set(int(j) for j in rs.choice(len(jobs), 12, replace=False))
    g = models["g"]

    def sweep(**kw):
        digests, kept, stats = {}, {}, {}

        def sink(waves):
            for j, w in waves.items():
                digests[j] = hashlib.blake2b(w.tobytes(), digest_size=12).digest()
                if j in keep_ids:
                    kept[j] = w.copy()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = harness.run_resynthesis(g, jobs, device=DEV, sink=sink, stats=stats, **kw)
        return n, digests, kept, stats, time.perf_counter() - t0

    n, dig, kept, stats, wall = sweep(round_floats=1 << 27)
    audio_sec = sum(len(j["code"]) for j in jobs) * 0.02
    print(f"cfg5 sweep: {audio_sec:.0f} s of audio in {wall:.2f} s wall = {audio_sec / wall:.0f}x real time incl. host "
          f"batching, D2H and hashing; {stats['rounds']} rounds, compute {stats['compute_s']:.2f} s")
    assert n == 10368 and sorted(dig) == list(range(10368)) and stats["rounds"] >= 4
    assert stats["sent_floats"] <= 1.1 * stats["payload_floats"]
    n2, dig2, _, _, _ = sweep(max_batch=13, max_frames=13 * 251, round_floats=None)
    assert n2 == 10368 and dig2 == dig
    gw = gr.fold_state_dict(models["gsd"])
    ids = sorted(keep_ids)
    for j in ids:
        assert kept[j].shape == (320 * len(jobs[j]["code"]),)
        one = harness.run_resynthesis(g, [jobs[j]], device=DEV)[0]
        np.testing.assert_array_equal(one, kept[j])
    for j in ids[:4]:  # the sweep ran without post-processing: raw generator output vs the oracle
        job = jobs[j]
        ref = gr.code_generator(gw, synth.VCTK_CONFIG, torch.from_numpy(job["code"])[None],
                                torch.from_numpy(job["f0"])[None, None], torch.tensor([[job["spkr"]]]))
        err = kept[j].astype(np.float64) - ref[0, 0].numpy()
        assert np.sqrt(np.mean(err ** 2)) <= 1e-4
        post = torch.from_numpy(kept[j].copy())[None, None].to(DEV)
        wav_postprocess_(post, torch.tensor([post.shape[-1]], dtype=torch.int32, device=DEV))
        ref_post = gr.wav_postprocess(kept[j])
        np.testing.assert_array_equal(post[0, 0].cpu().numpy(), ref_post)
