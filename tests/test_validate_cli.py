"""sr/validate.py: its host logic with a stub scorer (no GPU), and the whole command on the MI355X.

On the GPU the per-file errors of mel_spec_error.json must equal the float64 oracle (tests/mel_ref.py) applied to the
ground truth and to the waveform an in-process CodeGenerator produces for the same inputs, within the fused-L1 bar of
tests/test_gpu_mel.py: the mean over cells of the two signals' per-cell log tolerances.
"""
import importlib.util
import json
import os
import shutil

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import synthdata as synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP = 320  # code_hop_size of the shipped configs


@pytest.fixture(scope="module")
def cli():
    spec = importlib.util.spec_from_file_location("dissc_sr_validate_cli", os.path.join(ROOT, "sr", "validate.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


MEL_CFG = dict(n_fft=1024, num_mels=80, hop_size=256, win_size=1024, fmin=0, fmax=8000, fmax_for_loss=None, sampling_rate=16000,
               code_hop_size=HOP)


def setup_tree(td, golden_dir, extra_lengths=(10560 + 77,), checkpoints=(("g_00000001", 0),)):
    """checkpoint dir, wav dir and a manifest: the two golden recordings and synthetic wavs whose lengths are no hop multiple"""
    for d in ("ckpt", "wav", "meta", "out"):
        os.makedirs(f"{td}/{d}")
    cfg = dict(synth.VCTK_CONFIG, **MEL_CFG, input_training_file=f"{td}/meta/train.txt", input_validation_file=f"{td}/meta/val.txt",
               val_base_path=f"{td}/wav", f0_normalize=False, f0_stats=None)
    json.dump(cfg, open(f"{td}/ckpt/config.json", "w"))
    for name, seed in checkpoints:
        torch.save({"generator": synth.synth_generator_state_dict(seed=seed)}, f"{td}/ckpt/{name}")
    shutil.copy(os.path.join(golden_dir, "vctk_id_to_spkr.pkl"), f"{td}/meta/id_to_spkr.pkl")
    names = ["p225_001.wav", "p231_002.wav"]
    for i, nm in enumerate(names):
        shutil.copy(os.path.join(golden_dir, f"s1_{i + 1}.wav"), f"{td}/wav/{nm}")
    for j, n in enumerate(extra_lengths):
        names.append(f"p226_{j:03d}.wav")
        wavfile.write(f"{td}/wav/{names[-1]}", 16000, np.round(synth.synth_waveform(n, seed=40 + j, kind="speech_like") * 32767).astype(np.int16))
    rs = np.random.RandomState(3)
    with open(f"{td}/meta/val.txt", "w") as f:
        for nm in names:
            n = wavfile.read(f"{td}/wav/{nm}")[1].shape[0]
            T = n // HOP + 3  # a few units more than the audio has: cut to the audio like the trainer's data set does
            f0 = np.where(rs.rand(T) < 0.4, 0.0, 100.0 + 80.0 * rs.rand(T))
            f.write(json.dumps({"audio": f"/somewhere/else/{nm}", "units": rs.randint(0, 100, T).tolist(), "f0": f0.tolist()}) + "\n")
    return cfg, names


# ---------------------------------------------------------------------------------------------------------
# host logic, no GPU
# ---------------------------------------------------------------------------------------------------------
def test_items_means_report_and_ordering_with_a_stub_scorer(cli, golden_dir, tmp_path, capsys):
    td = str(tmp_path)
    cfg, names = setup_tree(td, golden_dir, extra_lengths=(10560 + 77, 300), checkpoints=(("g_00000001", 0), ("g_00000002", 0)))
    seen = []

    def make_scorer(cp):
        scale = 2.0 if cp.endswith("g_00000001") else 1.0  # the later checkpoint is the better one

        def scorer(batch):
            seen.append((os.path.basename(cp), [it["name"] for it in batch]))
            for it in batch:  # prepared like the trainer's validation items
                n = wavfile.read(f"{td}/wav/{it['name']}")[1].shape[0]
                T = n // HOP
                assert len(it["code"]) == len(it["f0"]) == T and it["gt"].shape == (T * HOP,) and it["gt"].dtype == np.float32
                assert 0.1 < np.abs(it["gt"]).max() <= 0.95 + 1e-6  # peak-scaled before the cut
                assert it["spkr"] == pickle_index(golden_dir, it["name"].split("_")[0])
            frames = np.array([len(it["gt"]) // 256 for it in batch])
            return frames, scale * np.array([0.5 + 0.001 * len(it["code"]) for it in batch])
        return scorer

    res = cli.main(["--checkpoint_file", f"{td}/ckpt/", "--all", "--output_dir", f"{td}/out"], make_scorer=make_scorer)
    out = capsys.readouterr().out
    assert "skipped p226_001.wav" in out  # 300 samples: no unit survives the cut / too short to mirror
    assert [r["checkpoint"] for r in res] == ["g_00000002", "g_00000001"]  # best first
    lines = [ln for ln in out.splitlines() if "validation/mel_spec_error:" in ln]
    assert len(lines) == 2 and lines[0].startswith("g_00000002") and lines[1].startswith("g_00000001")
    doc = json.load(open(f"{td}/out/mel_spec_error.json"))
    assert [c["checkpoint"] for c in doc["checkpoints"]] == ["g_00000002", "g_00000001"]
    for c in doc["checkpoints"]:
        assert [r["name"] for r in c["rows"]] == names[:3]  # manifest order, whatever the batches were
        assert all(set(r) == {"name", "frames", "error"} for r in c["rows"])
        err, fr = np.array([r["error"] for r in c["rows"]]), np.array([r["frames"] for r in c["rows"]], np.float64)
        assert c["mel_spec_error"] == pytest.approx(err.mean(), rel=1e-15)
        assert c["frame_weighted"] == pytest.approx((err * fr).sum() / fr.sum(), rel=1e-15)
        assert c["files"] == 3 and c["frames"] == int(fr.sum()) and c["precision"] == "fp32"
        assert f"{c['mel_spec_error']:.6f}" in out
    # batches are the harness's: longest first
    assert seen[0][1][0] == max(names[:3], key=lambda nm: wavfile.read(f"{td}/wav/{nm}")[1].shape[0])
    # without --all: the latest checkpoint only, into the checkpoint directory by default
    res = cli.main(["--checkpoint_file", f"{td}/ckpt/"], make_scorer=make_scorer)
    assert [r["checkpoint"] for r in res] == ["g_00000002"] and os.path.exists(f"{td}/ckpt/mel_spec_error.json")
    assert capsys.readouterr().out.count("validation/mel_spec_error:") == 1


def pickle_index(golden_dir, speaker):
    import pickle
    return list(pickle.load(open(os.path.join(golden_dir, "vctk_id_to_spkr.pkl"), "rb"))).index(speaker)


def test_f0_is_normalised_by_the_source_speakers_statistics(cli, golden_dir, tmp_path):
    td = str(tmp_path)
    cfg, names = setup_tree(td, golden_dir)
    stats = {"p225": {"mean": 120.0, "std": 20.0}, "f0_mean": 150.0, "f0_std": 30.0}
    from dissc_amd import AttrDict, formats
    samples = formats.read_manifest(f"{td}/meta/val.txt")
    ids = formats.load_pickle(f"{td}/meta/id_to_spkr.pkl")
    raw, _ = cli.prepare_items(AttrDict(cfg), samples, ids, None, f"{td}/wav")
    items, skipped = cli.prepare_items(AttrDict(dict(cfg, f0_normalize=True)), samples, ids, stats, f"{td}/wav")
    assert not skipped and [it["name"] for it in items] == names
    for it, r, (mean, std) in zip(items, raw, ((120.0, 20.0), (150.0, 30.0), (150.0, 30.0))):
        v = r["f0"] != 0
        np.testing.assert_allclose(it["f0"][v], (r["f0"][v] - mean) / std, rtol=1e-6)
        assert np.array_equal(it["f0"][~v], r["f0"][~v]) and np.array_equal(it["code"], r["code"])
    assert cli.summarise([])["files"] == 0


# ---------------------------------------------------------------------------------------------------------
# the whole command on the GPU
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_validate_cli_equals_the_float64_oracle(cli, golden_dir, tmp_path, capsys):
    import mel_ref
    from mel_cases import SHIPPED, Ref
    from dissc_amd import AttrDict, CodeGenerator, formats
    td = str(tmp_path)
    cfg, names = setup_tree(td, golden_dir, checkpoints=(("g_00000001", 0), ("g_00000002", 1)))
    res = cli.main(["--checkpoint_file", f"{td}/ckpt/", "--all", "--output_dir", f"{td}/out"])
    out = capsys.readouterr().out
    doc = json.load(open(f"{td}/out/mel_spec_error.json"))
    assert sorted(c["checkpoint"] for c in doc["checkpoints"]) == ["g_00000001", "g_00000002"]
    assert out.count("validation/mel_spec_error:") == 2 and "g_00000001" in out and "g_00000002" in out
    h = AttrDict(cfg)
    items, _ = cli.prepare_items(h, formats.read_manifest(f"{td}/meta/val.txt"), formats.load_pickle(f"{td}/meta/id_to_spkr.pkl"),
                                 None, f"{td}/wav")
    assert [it["name"] for it in items] == names
    for c in doc["checkpoints"]:
        g = CodeGenerator(h).to("cuda:0")
        g.load_state_dict(torch.load(f"{td}/ckpt/{c['checkpoint']}", map_location="cpu")["generator"])
        g.eval()
        g.remove_weight_norm()
        rows = {r["name"]: r for r in c["rows"]}
        for it in items:  # one utterance at a time: the figure does not depend on how the command batched
            T = len(it["code"])
            y = g(code=torch.from_numpy(it["code"]).view(1, T), f0=torch.from_numpy(it["f0"]).view(1, 1, T),
                  spkr=torch.tensor([[it["spkr"]]]), lengths=torch.tensor([T], dtype=torch.int32)).cpu().numpy().reshape(-1)
            assert y.shape == it["gt"].shape
            a, b = Ref([it["gt"]], SHIPPED), Ref([y], SHIPPED)
            want, bar = float(np.abs(a.log[0] - b.log[0]).mean()), float((a.tol[0] + b.tol[0]).mean())
            r = rows[it["name"]]
            print(f"validate {c['checkpoint']} {it['name']}: {r['error']:.9f} oracle {want:.9f} bar {bar:.3e}")
            assert r["frames"] == len(y) // 256 == mel_ref.frames(len(y), 256)
            assert abs(r["error"] - want) <= bar, (c["checkpoint"], it["name"], r["error"], want, bar)
        assert c["mel_spec_error"] == pytest.approx(np.mean([r["error"] for r in c["rows"]]), rel=1e-15)
        assert f"validation/mel_spec_error: {c['mel_spec_error']:.6f}" in out
