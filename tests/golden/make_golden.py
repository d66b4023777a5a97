"""Generate golden vectors by running the REFERENCE itself (this container only).

    python tests/golden/make_golden.py            # writes tests/golden/*.npz (every target, one
                                                  # interpreter each: the reference's root and sr/
                                                  # trees both define modules named utils/models/dataset)
    python tests/golden/make_golden.py hubert     # one target

Imports the reference modules unmodified from /root/reference (which does not
exist on the GPU box -- only the .npz outputs travel).  Weights/inputs come
from synthdata.py (numpy RandomState, reproducible anywhere), are loaded
into the reference modules with strict ``load_state_dict`` (which also pins our
checkpoint key/shape layout against the reference's), and the reference's
outputs are stored.  Nothing of the reference's source is stored.
"""
import json
import os
import sys
import types
import warnings

import numpy as np
import torch

warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
OUT = os.environ.get("DISSC_GOLDEN_OUT", HERE)  # where the fixtures are written (tests regenerate into a temp dir)
os.makedirs(OUT, exist_ok=True)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import synthdata as synth  # noqa: E402


def _import_ref_sr():
    sys.path.insert(0, os.path.join(REF, "sr"))
    import models as ref_models  # reference sr/models.py
    import utils as ref_utils  # reference sr/utils.py
    return ref_models, ref_utils


def make_generator():
    ref_models, ref_utils = _import_ref_sr()
    h = ref_utils.AttrDict(json.load(open(os.path.join(REF, "sr/configs/VCTK/hubert100_lut.json"))))
    out = {}
    for seed in (0,):
        g = ref_models.CodeGenerator(h)
        sd = synth.synth_generator_state_dict(seed=seed)
        g.load_state_dict(sd, strict=True)
        g.eval()
        g.remove_weight_norm()
        fsd = g.state_dict()
        # checksums of the folded weights (pins fold_weight_norm incl. ConvTranspose)
        for name in ("conv_pre", "ups.0", "ups.3", "resblocks.0.convs1.2", "resblocks.14.convs2.0", "conv_post"):
            wt = fsd[name + ".weight"].double()
            out[f"s{seed}/fold/{name}"] = np.array([wt.sum().item(), wt.abs().sum().item(), (wt * wt).sum().item()])
        out[f"s{seed}/fold/ups.4.weight"] = fsd["ups.4.weight"].numpy()

        # activations are captured with forward hooks on the reference modules
        def run(code, f0, spkr, want_taps):
            taps = {}
            hooks = []
            if want_taps:
                hooks.append(g.conv_pre.register_forward_hook(lambda m, i, o: taps.__setitem__("conv_pre", o.clone())))
                for i, up in enumerate(g.ups):
                    hooks.append(up.register_forward_hook(lambda m, i_, o, i=i: taps.__setitem__(f"up{i}", o.clone())))
                # the MRF output of stage i is the (pre-lrelu) input of ups[i+1] / conv_post
                for i, up in enumerate(g.ups):
                    if i > 0:
                        hooks.append(up.register_forward_pre_hook(
                            lambda m, a, i=i: taps.__setitem__(f"lrelu_mrf{i-1}", a[0].clone())))
                for j, rb in enumerate(g.resblocks):
                    hooks.append(rb.register_forward_hook(lambda m, i_, o, j=j: taps.__setitem__(f"rb{j}", o.clone())))
            with torch.no_grad():
                y = g(code=torch.from_numpy(code), f0=torch.from_numpy(f0), spkr=torch.from_numpy(spkr))
            for hk in hooks:
                hk.remove()
            return y, taps

        for T in (1, 2, 7, 33, 99):
            code, f0, spkr, _ = synth.synth_generator_inputs(1, T, seed=100 + T)
            y, taps = run(code, f0, spkr, want_taps=(T == 7))
            out[f"s{seed}/T{T}/wav"] = y.numpy()
            for k, v in taps.items():
                out[f"s{seed}/T{T}/{k}"] = v.numpy()
        # ragged batch: the reference never batches -> one call per utterance
        code, f0, spkr, _ = synth.synth_generator_inputs(4, 40, seed=777)
        lengths = np.array([40, 23, 9, 1], dtype=np.int32)
        for b in range(4):
            n = int(lengths[b])
            y, _ = run(code[b:b + 1, :n], f0[b:b + 1, :, :n], spkr[b:b + 1], False)
            out[f"s{seed}/ragged/wav{b}"] = y.numpy()
        out[f"s{seed}/ragged/lengths"] = lengths
    np.savez_compressed(os.path.join(OUT, "gen_vctk.npz"), **out)
    print("gen_vctk.npz", len(out), "arrays")


def make_generator_trained_like():
    """synthdata's kind="trained_like" checkpoint (seed 0) in the reference CodeGenerator -> gen_vctk_trainedlike.npz: the waveforms
    of trained-like inputs at T = 33 / 99 (seeds 100 + T, as make_generator's), fp32, and again with the folded module cast to
    float64 (.double() after remove_weight_norm: the fold stays fp32, as oracle.generator_ref.to_double does).  Outputs only: the
    weights and inputs come from the seeds."""
    ref_models, ref_utils = _import_ref_sr()
    h = ref_utils.AttrDict(json.load(open(os.path.join(REF, "sr/configs/VCTK/hubert100_lut.json"))))
    g = ref_models.CodeGenerator(h)
    g.load_state_dict(synth.synth_generator_state_dict(seed=0, kind="trained_like"), strict=True)
    g.eval()
    g.remove_weight_norm()
    out = {}
    for T in (33, 99):
        code, f0, spkr, _ = synth.synth_generator_inputs(1, T, seed=100 + T, kind="trained_like")
        with torch.no_grad():
            out[f"T{T}/wav"] = g(code=torch.from_numpy(code), f0=torch.from_numpy(f0), spkr=torch.from_numpy(spkr)).numpy()
    g.double()
    for T in (33, 99):
        code, f0, spkr, _ = synth.synth_generator_inputs(1, T, seed=100 + T, kind="trained_like")
        with torch.no_grad():
            y = g(code=torch.from_numpy(code), f0=torch.from_numpy(f0).double(), spkr=torch.from_numpy(spkr))
        assert y.dtype == torch.float64
        out[f"T{T}/wav64"] = y.numpy()
    np.savez_compressed(os.path.join(OUT, "gen_vctk_trainedlike.npz"), **out)
    print("gen_vctk_trainedlike.npz", {k: v.dtype.name for k, v in out.items()})


def _import_ref_root():
    """reference infer.py imports root utils.py -> `from tensorflow import summary`
    (reference utils.py:2); tensorflow is not installed, a stub module is enough."""
    import importlib.machinery
    tf = types.ModuleType("tensorflow")
    tf.__spec__ = importlib.machinery.ModuleSpec("tensorflow", None)  # torch._dynamo probes find_spec()
    tf.summary = None
    sys.modules.setdefault("tensorflow", tf)
    for m in ("utils", "models", "dataset"):
        sys.modules.pop(m, None)  # sr/utils.py may be cached under the same name
    if os.path.join(REF, "sr") in sys.path:
        sys.path.remove(os.path.join(REF, "sr"))
    sys.path.insert(0, REF)
    import argparse
    import infer as ref_infer
    from model.len_predictor import LenPredictor
    from model.pitch_predictor import PitchPredictor, PitchPredictorBase
    ref_infer.args = argparse.Namespace(n_tokens=100)
    return ref_infer, LenPredictor, PitchPredictor, PitchPredictorBase


def make_predictors():
    import json as _json
    import tempfile
    ref_infer, LenPredictor, PitchPredictor, PitchPredictorBase = _import_ref_root()
    out = {}
    n_spk = 108
    len_sd = synth.synth_len_state_dict(100, n_spk)
    mean, std = synth.synth_len_norm_stats()
    lm = LenPredictor(n_tokens=100, n_speakers=n_spk)
    lm.load_state_dict(len_sd, strict=True)
    lm.eval()
    lm.norm_mean, lm.norm_std = mean, std
    rs = np.random.RandomState(7)
    id2mean = torch.from_numpy((150 + 60 * rs.rand(n_spk)).astype(np.float32))
    id2std = torch.from_numpy((20 + 20 * rs.rand(n_spk)).astype(np.float32))
    out["id2pitch_mean"], out["id2pitch_std"] = id2mean.numpy(), id2std.numpy()
    pms = {}
    for kind, cls in (("new", PitchPredictor), ("base", PitchPredictorBase)):
        pm = cls(100, n_spk, id2pitch_mean=id2mean, id2pitch_std=id2std)
        pm.load_state_dict(synth.synth_pitch_state_dict(kind, 100, n_spk), strict=True)
        pm.eval()
        pms[kind] = pm
    seqs = synth.synth_unit_sequences(6, 8, 420, seed=99) + [np.array([5], dtype=np.int64),
                                                             np.array([3, 3, 3, 9], dtype=np.int64)]
    spks = [0, 17, 107, 3, 55, 9, 1, 2]
    out["n_seqs"] = np.array(len(seqs))
    with torch.no_grad():
        for i, (seq, spk) in enumerate(zip(seqs, spks)):
            out[f"seq{i}"] = seq
            out[f"spk{i}"] = np.array(spk)
            vals, counts = ref_infer.dedup_seq(seq)
            out[f"dd_vals{i}"], out[f"dd_counts{i}"] = np.array(vals), np.array(counts)
            dd = torch.tensor(vals).unsqueeze(0)
            spk_id = torch.tensor([[spk]])
            lens = lm(dd, spk_id)
            out[f"lens{i}"] = lens.numpy()
            fixed = ref_infer.len_carryover_correction(lens)
            out[f"lens_int{i}"] = fixed.numpy().astype(np.int64)
            exp = torch.repeat_interleave(dd, fixed).view(1, -1)
            out[f"expanded{i}"] = exp.numpy()
            for kind, pm in pms.items():
                if (exp.shape[-1] > 850 and kind == "new") or exp.shape[-1] == 0:
                    continue  # the reference itself crashes on an empty expansion / > 850 frames
                out[f"f0_{kind}_norm{i}"] = pm.infer_freq(exp, spk_id, True).numpy()
                out[f"f0_{kind}_hz{i}"] = pm.infer_freq(exp, spk_id, False).numpy()
        # direct carry-over vectors incl. .5 ties and values < 1
        for j, v in enumerate([[0.2, 0.49, 2.5, 3.5, 1.5, 0.5, 7.99, 1.01, 4.5, 2.49999],
                               [1.4] * 7 + [2.6] * 5 + [0.1] * 9, [1.0], [3.3, 3.3, 3.4, 0.0, -2.0, 9.7]]):
            t = torch.tensor([v], dtype=torch.float32)
            out[f"carry_in{j}"] = t.numpy()
            out[f"carry_out{j}"] = ref_infer.len_carryover_correction(t).numpy().astype(np.int64)
    # end-to-end reference infer_wild() on a JSONL manifest -> output JSONL (units exact, f0 floats)
    import pickle
    with tempfile.TemporaryDirectory() as td:
        os.makedirs(f"{td}/len"); os.makedirs(f"{td}/pitch"); os.makedirs(f"{td}/out")
        torch.save(len_sd, f"{td}/len/best_model.pth")
        torch.save((mean, std), f"{td}/len/len_norm_stats.pth")
        torch.save(synth.synth_pitch_state_dict("base", 100, 10), f"{td}/pitch/best_model.pth")
        spk_names = pickle.load(open(os.path.join(REF, "data/ESD/hubert100/id_to_spkr.pkl"), "rb"))
        f0_stats = os.path.join(REF, "data/ESD/hubert100/f0_stats.pkl")
        len_sd10 = synth.synth_len_state_dict(100, 10)
        torch.save(len_sd10, f"{td}/len/best_model.pth")
        man = f"{td}/wild.txt"
        wild = synth.synth_unit_sequences(3, 30, 200, seed=5)
        with open(man, "w") as f:
            for i, s in enumerate(wild):
                f.write(_json.dumps({"units": s.tolist(), "f0": [0.0] * len(s), "audio": f"s1_{i}.wav"}) + "\n")
        import argparse
        a = argparse.Namespace(input_path=man, out_path=f"{td}/out", len_model=f"{td}/len/",
                               f0_model=f"{td}/pitch/", f0_model_type="base", n_tokens=100, device="cpu",
                               f0_path=f0_stats, norm_pitch=True, target_speakers=[spk_names[2], spk_names[7]],
                               id_to_spkr=os.path.join(REF, "data/ESD/hubert100/id_to_spkr.pkl"))
        ref_infer.args = a
        ref_infer.infer_wild(man, "cpu", a)
        for t in a.target_speakers:
            lines = open(f"{td}/out/{t}_wild.txt").read().strip().split("\n")
            for i, ln in enumerate(lines):
                d = _json.loads(ln)
                out[f"wild/{t}/{i}/units"] = np.array(d["units"], dtype=np.int64)
                out[f"wild/{t}/{i}/f0"] = np.array(d["f0"], dtype=np.float64)
        out["wild/targets"] = np.array(a.target_speakers)
        for i, s in enumerate(wild):
            out[f"wild/in{i}"] = s
    # end-to-end reference infer() (reconstruction + 2 targets, "new" pitch model, VCTK speakers)
    import shutil
    with tempfile.TemporaryDirectory() as td:
        os.makedirs(f"{td}/len"); os.makedirs(f"{td}/pitch"); os.makedirs(f"{td}/out"); os.makedirs(f"{td}/in")
        torch.save(len_sd, f"{td}/len/best_model.pth")
        torch.save((mean, std), f"{td}/len/len_norm_stats.pth")
        torch.save(synth.synth_pitch_state_dict("new", 100, n_spk), f"{td}/pitch/best_model.pth")
        shutil.copy(os.path.join(REF, "data/VCTK/hubert100/id_to_spkr.pkl"), f"{td}/in/id_to_spkr.pkl")
        val = synth.synth_unit_sequences(3, 40, 260, seed=11)
        vnames = ["p226_001.wav", "p300_014.wav", "p231_100.wav"]
        rs2 = np.random.RandomState(12)
        with open(f"{td}/in/val.txt", "w") as f:
            for s_, nm in zip(val, vnames):
                f0 = (rs2.rand(len(s_)) > 0.3) * (120 + 80 * rs2.rand(len(s_)))
                f.write(_json.dumps({"units": s_.tolist(), "f0": f0.tolist(), "audio": nm}) + "\n")
        out["val/manifest"] = np.array(open(f"{td}/in/val.txt").read())
        a = argparse.Namespace(input_path=f"{td}/in/val.txt", n=3, out_path=f"{td}/out", pred_len=True,
                               pred_pitch=True, len_model=f"{td}/len/", f0_model=f"{td}/pitch/",
                               f0_model_type="new", n_tokens=100, device="cpu", seed=42,
                               f0_path=os.path.join(REF, "data/VCTK/hubert100/f0_stats.pkl"), vc=True,
                               norm_pitch=True, target_speakers=["p231", "p225"], sample_df=None,
                               wild_sample=False, id_to_spkr=None)
        ref_infer.args = a
        ref_infer.infer(a.input_path, "cpu", a)
        for fn in sorted(os.listdir(f"{td}/out")):
            for i, ln in enumerate(open(f"{td}/out/{fn}").read().strip().split("\n")):
                d = _json.loads(ln)
                out[f"val/{fn}/{i}/units"] = np.array(d["units"], dtype=np.int64)
                out[f"val/{fn}/{i}/f0"] = np.array(d["f0"], dtype=np.float64)
                out[f"val/{fn}/{i}/audio"] = np.array(d["audio"])
        # rhythm-only conversion (--pred_len without --pred_pitch): F0 is the source contour morphed
        # per unit run by utils.morph_seq_len (reference infer.py:40-41, utils.py:39-52)
        os.makedirs(f"{td}/out2")
        a2 = argparse.Namespace(**{**vars(a), "pred_pitch": False, "out_path": f"{td}/out2"})
        ref_infer.args = a2
        ref_infer.infer(a2.input_path, "cpu", a2)
        for fn in sorted(os.listdir(f"{td}/out2")):
            for i, ln in enumerate(open(f"{td}/out2/{fn}").read().strip().split("\n")):
                d = _json.loads(ln)
                out[f"lenonly/{fn}/{i}/units"] = np.array(d["units"], dtype=np.int64)
                out[f"lenonly/{fn}/{i}/f0"] = np.array(d["f0"], dtype=np.float64)
        # pitch-only conversion of listed pairs: --pred_pitch (base model) without --pred_len, F0 written
        # in Hz (norm_pitch off = de-normalised with the target's statistics), --sample_df
        import pandas as pd
        os.makedirs(f"{td}/out3")
        torch.save(synth.synth_pitch_state_dict("base", 100, n_spk), f"{td}/pitch/best_model.pth")
        pairs = pd.DataFrame({"syn_sample": ["p226_001", "p231_100", "p231_100"], "syn_trgt": ["p225", "p231", "p225"]})
        pairs.to_csv(f"{td}/in/pairs.csv")
        a3 = argparse.Namespace(**{**vars(a), "pred_len": False, "pred_pitch": True, "f0_model_type": "base",
                                   "norm_pitch": False, "sample_df": f"{td}/in/pairs.csv", "out_path": f"{td}/out3"})
        ref_infer.args = a3
        ref_infer.infer(a3.input_path, "cpu", a3)
        out["pitchonly/pairs"] = np.array([list(pairs.syn_sample), list(pairs.syn_trgt)])
        for fn in sorted(os.listdir(f"{td}/out3")):
            lines3 = open(f"{td}/out3/{fn}").read().strip().split("\n")
            out[f"pitchonly/{fn}/n"] = np.array(len(lines3))
            for i, ln in enumerate(lines3):
                d = _json.loads(ln)
                out[f"pitchonly/{fn}/{i}/units"] = np.array(d["units"], dtype=np.int64)
                out[f"pitchonly/{fn}/{i}/f0"] = np.array(d["f0"], dtype=np.float64)
                out[f"pitchonly/{fn}/{i}/audio"] = np.array(d["audio"])
        import utils as ref_utils_root  # reference root utils.py (tensorflow stubbed)
        rs3 = np.random.RandomState(5)
        for j, (u, tl) in enumerate([([3, 3, 3, 7, 7, 1], [5, 1, 2]), ([4], [3]), ([1, 2, 2, 2, 2, 9, 9], [2, 2, 5]),
                                     ([5, 5, 6, 6, 6], [0, 4])]):
            pitch = rs3.rand(len(u)) * 100
            out[f"morph/{j}/units"], out[f"morph/{j}/pitch"], out[f"morph/{j}/lens"] = np.array(u), pitch, np.array(tl)
            out[f"morph/{j}/out"] = np.asarray(ref_utils_root.morph_seq_len(np.array(u), pitch, np.array(tl)), dtype=np.float64)
    np.savez_compressed(os.path.join(OUT, "pred.npz"), **out)
    print("pred.npz", len(out), "arrays")


def make_sr_inference():
    """Run the reference's sr/inference.py worker code (init_worker + inference) on CPU.

    librosa / soundfile / amfm_decompy are not installed: tiny stand-in modules provide
    librosa.util.normalize (x / max|x| unless the peak is below float tiny -- its documented
    norm=inf behaviour), librosa.filters.mel (unused result) and soundfile.read (scipy)."""
    import json as _json
    import pickle
    import queue
    import shutil
    import tempfile
    from scipy.io import wavfile

    for m in list(sys.modules):
        if m in ("utils", "models", "dataset", "inference", "infer") or m.startswith(("model.", "modules")):
            sys.modules.pop(m, None)
    if REF in sys.path:
        sys.path.remove(REF)
    sys.path.insert(0, os.path.join(REF, "sr"))

    def _normalize(S, **kw):
        S = np.asarray(S)
        mag = np.abs(S).astype(float)
        length = np.max(mag, axis=0, keepdims=True)
        tiny = np.finfo(S.dtype).tiny if S.dtype.kind == "f" else np.finfo(np.float32).tiny
        length = np.where(length < tiny, 1.0, length)
        return (S / length).astype(S.dtype if S.dtype.kind == "f" else float)

    librosa = types.ModuleType("librosa")
    librosa.util = types.ModuleType("librosa.util")
    librosa.util.normalize = _normalize
    librosa.filters = types.ModuleType("librosa.filters")
    librosa.filters.mel = lambda sr, n_fft, n_mels, fmin, fmax: np.zeros((n_mels, n_fft // 2 + 1), np.float32)
    sf = types.ModuleType("soundfile")
    sf.read = lambda path, dtype="int16": (lambda r: (r[1], r[0]))(wavfile.read(str(path)))
    amfm = types.ModuleType("amfm_decompy")
    sys.modules.update({"librosa": librosa, "librosa.util": librosa.util, "librosa.filters": librosa.filters,
                        "soundfile": sf, "amfm_decompy": amfm,
                        "amfm_decompy.basic_tools": types.ModuleType("amfm_decompy.basic_tools"),
                        "amfm_decompy.pYAAPT": types.ModuleType("amfm_decompy.pYAAPT")})
    import inference as ref_inf  # reference sr/inference.py

    out = {}
    with tempfile.TemporaryDirectory() as td:
        os.makedirs(f"{td}/ckpt"); os.makedirs(f"{td}/wav"); os.makedirs(f"{td}/out"); os.makedirs(f"{td}/meta")
        cfg = _json.load(open(os.path.join(REF, "sr/configs/VCTK/hubert100_lut.json")))
        cfg.update({"input_training_file": f"{td}/meta/train.txt", "f0_normalize": False, "f0_stats": None})
        _json.dump(cfg, open(f"{td}/ckpt/config.json", "w"))
        torch.save({"generator": synth.synth_generator_state_dict(seed=0)}, f"{td}/ckpt/g_00000001")
        shutil.copy(os.path.join(REF, "data/VCTK/hubert100/id_to_spkr.pkl"), f"{td}/meta/id_to_spkr.pkl")
        names = ["p226_001.wav", "p300_002.wav"]
        srcs = ["s1_1.wav", "s1_2.wav"]
        lens = [90, 71]
        man = f"{td}/man.txt"
        with open(man, "w") as f:
            for i, (nm, sr_, T) in enumerate(zip(names, srcs, lens)):
                shutil.copy(os.path.join(REF, "data/unseen/wav_orig", sr_), f"{td}/wav/{nm}")
                code, f0, _, _ = synth.synth_generator_inputs(1, T, seed=900 + i)
                f.write(_json.dumps({"units": code[0].tolist(), "f0": f0[0, 0].tolist(), "audio": nm}) + "\n")
                out[f"sr/units{i}"], out[f"sr/f0{i}"] = code[0], f0[0, 0]
        import argparse
        a = argparse.Namespace(code_file=None, input_code_file=man, data_path=f"{td}/wav", output_dir=f"{td}/out",
                               checkpoint_file=f"{td}/ckpt/", f0_stats=None, vc=True,
                               target_speakers=["p231", "p225"], pad=None, debug=True, eval_mode=True,
                               parts=False, unseen_f0=None, unseen_speaker=False, id_to_spkr=None,
                               sample_df=None, n=-1)
        q = queue.Queue()
        q.put("cpu")
        try:
            ref_inf.init_worker(q, a)
        except TypeError:
            pass  # `seed = 52 + idx` with idx='cpu' (reference sr/inference.py:166): all globals are set by then
        for i in range(2):
            ref_inf.inference(i)
        for fn in sorted(os.listdir(f"{td}/out")):
            rate, data = wavfile.read(f"{td}/out/{fn}")
            assert rate == 16000
            out[f"sr/out/{fn}"] = data
        out["sr/names"] = np.array(names)

        # ---- scenario B: unseen source speaker + per-target F0 re-normalisation (--f0-stats) + --parts
        def run_ref(ns, n_items):
            q2 = queue.Queue()
            q2.put("cpu")
            try:
                ref_inf.init_worker(q2, ns)
            except TypeError:
                pass
            for i in range(n_items):
                ref_inf.inference(i)

        os.makedirs(f"{td}/data/wav"); os.makedirs(f"{td}/out_b"); os.makedirs(f"{td}/out_c")
        names_b = ["newspk_001.wav", "other_002_mic2.wav"]
        man_b = f"{td}/man_b.txt"
        with open(man_b, "w") as f:
            for i, (nm, sr_, T) in enumerate(zip(names_b, srcs, lens)):
                shutil.copy(os.path.join(REF, "data/unseen/wav_orig", sr_), f"{td}/data/wav/{nm}")
                code, f0, _, _ = synth.synth_generator_inputs(1, T, seed=950 + i)
                hz = np.where(f0[0, 0] != 0, 180.0 + 40.0 * f0[0, 0], 0.0).astype(np.float32)  # F0 in Hz
                f.write(_json.dumps({"units": code[0].tolist(), "f0": hz.tolist(), "audio": nm}) + "\n")
                out[f"srb/units{i}"], out[f"srb/f0{i}"] = code[0], hz
        id_to_spkr = pickle.load(open(f"{td}/meta/id_to_spkr.pkl", "rb"))
        tids = [id_to_spkr.index("p231"), id_to_spkr.index("p225")]
        stats = {tids[0]: {"f0_mean": 121.5, "f0_std": 23.25}, "f0_mean": 150.0, "f0_std": 30.0}  # p225 falls back
        torch.save(stats, f"{td}/meta/tgt_f0_stats.pt")
        b = argparse.Namespace(**{**vars(a), "input_code_file": man_b, "data_path": f"{td}/data/wav",
                                  "output_dir": f"{td}/out_b", "f0_stats": f"{td}/meta/tgt_f0_stats.pt",
                                  "parts": True, "unseen_speaker": True, "id_to_spkr": f"{td}/meta/id_to_spkr.pkl"})
        run_ref(b, 2)
        for fn in sorted(os.listdir(f"{td}/out_b")):
            out[f"srb/out/{fn.replace(os.path.basename(td) + '_', 'TD_')}"] = wavfile.read(f"{td}/out_b/{fn}")[1]
        out["srb/names"] = np.array(names_b)
        out["srb/stats"] = np.array([tids[0], 121.5, 23.25, 150.0, 30.0])

        # ---- scenario C: --sample_df (only the listed source/target pairs, no GT, no resynthesis)
        import pandas as pd
        names_c = ["p226_001.wav", "p300_002_mic2.wav"]
        man_c = f"{td}/man_c.txt"
        with open(man_c, "w") as f:
            for i, (nm, nb) in enumerate(zip(names_c, names_b)):
                shutil.copy(f"{td}/data/wav/{nb}", f"{td}/data/wav/{nm}")
                f.write(_json.dumps({"units": out[f"srb/units{i}"].tolist(), "f0": out[f"sr/f0{i}"][:lens[i]].tolist(),
                                     "audio": nm}) + "\n")
        df = pd.DataFrame({"syn_sample": ["p226_001", "p300_002", "p300_002"],
                           "syn_trgt": ["p231", "p225", "p231"]})
        df.to_csv(f"{td}/meta/pairs.csv")
        c = argparse.Namespace(**{**vars(a), "input_code_file": man_c, "data_path": f"{td}/data/wav",
                                  "output_dir": f"{td}/out_c", "sample_df": f"{td}/meta/pairs.csv",
                                  "target_speakers": ["p231", "p225", "p226"]})
        run_ref(c, 2)
        for fn in sorted(os.listdir(f"{td}/out_c")):
            out[f"src/out/{fn}"] = wavfile.read(f"{td}/out_c/{fn}")[1]
        out["src/pairs"] = np.array([list(df.syn_sample), list(df.syn_trgt)])
        out["src/names"] = np.array(names_c)
    np.savez_compressed(os.path.join(OUT, "sr_inference.npz"), **out)
    print("sr_inference.npz", sorted(k for k in out if k.startswith("sr/out")))


def make_hubert():
    """HF transformers.HubertModel (architecture oracle) + sklearn KMeans."""
    from sklearn.cluster import KMeans
    from transformers import HubertConfig, HubertModel
    from oracle import hubert_ref
    sd = synth.synth_hubert_state_dict(6)
    m = HubertModel(HubertConfig(num_hidden_layers=6)).eval()
    missing, unexpected = m.load_state_dict(hubert_ref.fairseq_to_hf(sd), strict=False)
    assert not unexpected and all("masked_spec_embed" in k for k in missing), (missing, unexpected)
    centers = synth.synth_kmeans_centers()
    km = KMeans(n_clusters=100, n_init=1)
    km.cluster_centers_ = centers.numpy().astype(np.float32)
    km._n_threads = 1
    km.n_features_in_ = 768
    out = {}
    for n in (400, 719, 4000, 16000, 32000):
        wav = torch.from_numpy(synth.synth_waveform(n, seed=n))[None]
        with torch.no_grad():
            o = m(wav, output_hidden_states=True)
            feats = m.feature_extractor(wav)
        dense = o.hidden_states[6][0].numpy()
        out[f"n{n}/dense"] = dense
        out[f"n{n}/units"] = km.predict(dense.astype(np.float32)).astype(np.int64)
        if n <= 4000:
            out[f"n{n}/cnn"] = feats.numpy()
            out[f"n{n}/h0"] = o.hidden_states[0][0].numpy()
    np.savez_compressed(os.path.join(OUT, "hubert.npz"), **out)
    print("hubert.npz", {k: v.shape for k, v in out.items() if k.endswith("units")})


# hubert_trained_like: the fixture's utterances (kind, samples, seed) and the ones the k-means centres are fitted on
HUBERT_TL_UTTS = (("speech_like", 32000, 31), ("speech_dc", 16000, 32), ("dither", 8000, 33))
HUBERT_TL_FIT = tuple(("speech_like" if i % 3 else "speech_dc", 48000 + 16000 * i, 40 + i) for i in range(6))
HUBERT_TL_KEEP = 5  # frames per utterance whose hidden states are stored (evenly spaced, both ends included): 1 MiB bounds the file


def make_hubert_trained_like():
    """synthdata's kind="trained_like" HuBERT (seed 3, 6 layers) -> hubert_trainedlike.npz:
    * centres: K = 100, sklearn KMeans (random_state 0, n_init 1) fitted on the float64 oracle's layer-6 features of the
      HUBERT_TL_FIT utterances (as km100 was fitted on HuBERT features: near-ties are frequent).  Stored, never refitted: the
      fit is not bit-stable across sklearn builds;
    * per HUBERT_TL_UTTS utterance u: HF HubertModel hidden_states[1..6] in fp32 (u/hs32 [6, F, 768]) and with the module in
      float64 (.double(); stored as u/hs64d = hs64 - hs32 in fp32, which keeps ~1e-14 of the float64 value) at the frames u/frames
      [F]; u/units: sklearn's fp32 predict on the fp32 layer-6 features of every frame."""
    from sklearn.cluster import KMeans
    from transformers import HubertConfig, HubertModel
    from oracle import hubert_ref
    sd = synth.synth_hubert_state_dict(6, kind="trained_like")
    sd64 = hubert_ref.to_double(sd)
    fit = []
    for kind, n, seed in HUBERT_TL_FIT:
        wav = torch.from_numpy(synth.synth_waveform(n, seed=seed, kind=kind))[None]
        fit.append(hubert_ref.encode(sd64, torch.zeros(1, 768), wav)[1].numpy())
    km = KMeans(n_clusters=100, n_init=1, random_state=0).fit(np.concatenate(fit))
    centers = km.cluster_centers_.astype(np.float32)
    km.cluster_centers_ = centers
    m = HubertModel(HubertConfig(num_hidden_layers=6)).eval()
    missing, unexpected = m.load_state_dict(hubert_ref.fairseq_to_hf(sd), strict=False)
    assert not unexpected and all("masked_spec_embed" in k for k in missing), (missing, unexpected)
    m64 = HubertModel(HubertConfig(num_hidden_layers=6)).eval()
    m64.load_state_dict(hubert_ref.fairseq_to_hf(sd), strict=False)
    m64.double()
    out = {"centers": centers}
    for kind, n, seed in HUBERT_TL_UTTS:
        wav = torch.from_numpy(synth.synth_waveform(n, seed=seed, kind=kind))[None]
        with torch.no_grad():
            h32 = m(wav, output_hidden_states=True).hidden_states
            h64 = m64(wav.double(), output_hidden_states=True).hidden_states
        T = h32[6].shape[1]
        frames = np.unique(np.linspace(0, T - 1, HUBERT_TL_KEEP).round().astype(np.int64))
        hs32 = np.stack([h32[L][0].numpy()[frames] for L in range(1, 7)])
        hs64 = np.stack([h64[L][0].numpy()[frames] for L in range(1, 7)])
        assert hs64.dtype == np.float64
        out[f"{kind}/frames"] = frames
        out[f"{kind}/hs32"] = hs32
        out[f"{kind}/hs64d"] = (hs64 - hs32).astype(np.float32)
        out[f"{kind}/units"] = km.predict(h32[6][0].numpy().astype(np.float32)).astype(np.int64)
    np.savez_compressed(os.path.join(OUT, "hubert_trainedlike.npz"), **out)
    print("hubert_trainedlike.npz", {k: v.shape for k, v in out.items()})


def synth_units_jsonl(seed=7, n_spk=5, utts_per_spk=6):
    """Encoded-dataset lines the way data/encode.py writes them: f0 in Hz as float32 values,
    exact 0.0 on unvoiced frames; one speaker is entirely unvoiced in one utterance."""
    rs = np.random.RandomState(seed)
    lines = []
    for s in range(n_spk):
        base = 90.0 + 35.0 * s
        for u in range(utts_per_spk):
            T = int(rs.randint(20, 60))
            f0 = (base + 20.0 * rs.randn(T)).astype(np.float32)
            f0[rs.rand(T) < 0.35] = 0.0
            if s == 1 and u == 0:
                f0[:] = 0.0
            units = rs.randint(0, 100, size=T)
            lines.append(json.dumps({"units": units.tolist(), "f0": f0.tolist(), "durations": [1] * T,
                                     "audio": f"sp{s:02d}_{u + 20}.wav"}))
    order = rs.permutation(len(lines))  # speakers interleaved, like os.listdir order
    return [lines[i] for i in order]


def make_prep_dataset():
    """reference data/data_utils.py calculate_pitch_stats + data_split on a synthetic encoded set."""
    import pickle
    import tempfile
    sys.path.insert(0, os.path.join(REF, "data"))
    import data_utils as ref_du
    lines = synth_units_jsonl()
    with open(os.path.join(OUT, "prep_units.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    out = {}
    with tempfile.TemporaryDirectory() as td:
        man = os.path.join(td, "all.txt")
        with open(man, "w") as f:
            f.write("\n".join(lines) + "\n")
        ref_du.calculate_pitch_stats(man, os.path.join(td, "stats.pkl"))
        stats = pickle.load(open(os.path.join(td, "stats.pkl"), "rb"))
        np.random.seed(42)
        tr, va = ref_du.data_split(man, "random")
        out["random"] = (open(tr).read(), open(va).read())
        tr, va = ref_du.data_split(man, "paired_val")
        out["paired_val"] = (open(tr).read(), open(va).read())
    with open(os.path.join(OUT, "prep_expected.pkl"), "wb") as f:
        pickle.dump({"stats": {k: {"mean": float(v["mean"]), "std": float(v["std"])} for k, v in stats.items()},
                     "split": out}, f)
    print("prep_expected.pkl", {k: (round(v["mean"], 3), round(v["std"], 3)) for k, v in stats.items()})


def synth_train_batch(kind, B=5, L=23, seed=11, n_spk=108):
    """a padded training batch the way the reference datasets build it (dataset/len_dataset.py:23-32,
    dataset/pitch_dataset.py:23-42): every row padded to the longest, pad token = n_tokens, pad label -1 / -100"""
    rs = np.random.RandomState(seed)
    lens_ = [L] + [int(v) for v in rs.randint(3, L, size=B - 1)]
    seq = np.full((B, L), 100, dtype=np.int64)
    pad = -1.0 if kind == "len" else -100.0
    tgt = np.full((B, L), pad, dtype=np.float32)
    for b, n in enumerate(lens_):
        seq[b, :n] = rs.randint(0, 100, size=n)
        if kind == "len":
            tgt[b, :n] = rs.randint(1, 9, size=n).astype(np.float32)
        else:
            f = rs.standard_normal(n).astype(np.float32)
            f[rs.rand(n) < 0.35] = 0.0
            tgt[b, :n] = f
    spk = rs.randint(0, n_spk, size=(B, 1)).astype(np.int64)
    keep = (rs.rand(B, L) <= (0.8 if kind == "len" else 0.6)).astype(np.float32)  # mask = uniform > keep_rate
    return seq, tgt, spk, keep


def compact(a):
    """small tensors whole; large ones as [sum, sum|.|, sum(.^2)] + every (numel // 509)-th element (fixtures stay small)"""
    a = np.asarray(a)
    if a.size <= 4096:
        return a.copy()
    f = a.reshape(-1).astype(np.float64)
    return np.concatenate([[f.sum(), np.abs(f).sum(), (f * f).sum()], f[::max(1, f.size // 509)]])


def _search_len_batch(model, fake_cuda, B, L, seed0, margin=2e-5, tries=400):
    """first seed >= seed0 whose batch keeps every LeakyReLU input of the length model (the train-mode BatchNorm
    outputs) at least `margin` away from 0; returns the batch, the seed and the smallest |pre-activation|"""
    acts = []
    hooks = [m.register_forward_hook(lambda _m, _i, o: acts.append(float(o.detach().abs().min())))
             for m in model.modules() if isinstance(m, torch.nn.BatchNorm1d)]
    state = {k: v.clone() for k, v in model.state_dict().items()}
    try:
        for seed in range(seed0, seed0 + tries):
            seq, tgt, spk, keep = synth_train_batch("len", B=B, L=L, seed=seed)
            fake_cuda.queue.append((torch.from_numpy(keep), model.keep_rate))
            acts.clear()
            with torch.no_grad():
                model(torch.from_numpy(seq).int(), torch.from_numpy(spk).int())
            model.load_state_dict(state)  # the probe forward moved the BatchNorm running statistics
            if min(acts) >= margin:
                return seq, tgt, spk, keep, seed, min(acts)
    finally:
        for h in hooks:
            h.remove()
    raise RuntimeError("no batch seed keeps the pre-activations away from 0")


def make_train():
    """Two optimisation steps of the REFERENCE models in train() mode on CPU (reference train_len_predictor.py:57-68,
    train_f0_predictor.py:58-66) with the random masks injected: torch.cuda.FloatTensor(...).uniform_() is replaced
    by a tensor holding chosen uniforms, nn.Dropout draws from the seeded CPU generator."""
    ref_infer, LenPredictor, PitchPredictor, PitchPredictorBase = _import_ref_root()
    sys.path.insert(0, REF)
    from loss.len_loss import LenSumLoss
    from loss.pitch_loss import PitchLoss
    out = {}
    n_spk = 108
    rs = np.random.RandomState(7)
    id2mean = torch.from_numpy((150 + 60 * rs.rand(n_spk)).astype(np.float32))
    id2std = torch.from_numpy((20 + 20 * rs.rand(n_spk)).astype(np.float32))
    out["id2pitch_mean"], out["id2pitch_std"] = id2mean.numpy(), id2std.numpy()

    class _FakeCudaFloat:
        """what `torch.cuda.FloatTensor(B, L).uniform_()` returns: uniforms u with (u > keep_rate) == masked"""
        queue = []

        def __init__(self, *shape):
            self.shape = shape

        def uniform_(self):
            keep, keep_rate = _FakeCudaFloat.queue.pop(0)
            assert tuple(keep.shape) == tuple(self.shape)
            return torch.where(keep > 0, torch.full_like(keep, keep_rate * 0.5), torch.full_like(keep, 0.5 + keep_rate * 0.5))

    real = torch.cuda.FloatTensor
    torch.cuda.FloatTensor = _FakeCudaFloat
    try:
        for kind in ("len", "new", "base"):
            if kind == "len":
                model = LenPredictor(n_tokens=100, n_speakers=n_spk, norm_mean=torch.tensor(3.3), norm_std=torch.tensor(2.1))
                model.load_state_dict(synth.synth_len_state_dict(100, n_spk), strict=True)
                crit = LenSumLoss(pad_idx=-1)
                lr = 3e-4
            else:
                cls = PitchPredictorBase if kind == "base" else PitchPredictor
                model = cls(100, n_spk, id2pitch_mean=id2mean, id2pitch_std=id2std)
                model.load_state_dict(synth.synth_pitch_state_dict(kind, 100, n_spk), strict=True)
                crit = PitchLoss(id2mean, id2std, pad_idx=-100)
                lr = 1e-3
            model.train()
            opt = torch.optim.Adam(model.parameters(), lr=lr)
            out[f"{kind}/lr"] = np.array(lr)
            for step in range(2):
                seq, tgt, spk, keep = synth_train_batch("len" if kind == "len" else "pitch", seed=11 + step)
                if kind == "len" and step == 0:
                    # LeakyReLU's derivative jumps at 0: a pre-activation within fp32 rounding of 0 takes the other
                    # branch in another implementation and moves every gradient below it by O(1 %).  Pick the first
                    # batch seed whose smallest |pre-activation| (all BatchNorm outputs, padding included) is far
                    # from rounding noise, so that the length model's gradients can be held to 1e-4 like the others.
                    seq, tgt, spk, keep, seed0, margin = _search_len_batch(model, _FakeCudaFloat, 5, 23, 11)
                    out["len/s0/seed"], out["len/s0/min_abs_preact"] = np.array(seed0), np.array(margin)
                for nm, arr in (("seq", seq), ("tgt", tgt), ("spk", spk), ("keep", keep)):
                    out[f"{kind}/s{step}/{nm}"] = arr
                _FakeCudaFloat.queue.append((torch.from_numpy(keep), model.keep_rate))
                if kind == "new":  # PositionalEncoding dropout(p = 0.4): first consumer of the CPU generator
                    torch.manual_seed(100 + step)
                    mult = torch.nn.functional.dropout(torch.ones(seq.shape[0], seq.shape[1], 32), 0.4, True)
                    out[f"{kind}/s{step}/pe_mult"] = mult.numpy()
                    torch.manual_seed(100 + step)
                opt.zero_grad()
                if kind == "len":
                    preds = model(torch.from_numpy(seq).int(), torch.from_numpy(spk).int())
                    loss = crit(preds, torch.from_numpy(tgt))
                else:
                    c, r = model(torch.from_numpy(seq).int(), torch.from_numpy(spk).int())
                    loss = crit(c, r, torch.from_numpy(tgt), torch.from_numpy(spk).int())
                loss.backward()
                out[f"{kind}/s{step}/loss"] = np.array(loss.item())
                for k, prm in model.named_parameters():
                    out[f"{kind}/s{step}/grad/{k}"] = compact((prm.grad if prm.grad is not None else torch.zeros_like(prm)).numpy())
                opt.step()
                for k, v in model.state_dict().items():
                    out[f"{kind}/s{step}/after/{k}"] = compact(v.numpy())
            if kind == "len":
                # a second single-step case on a batch longer than the 128-column tiles and no multiple of 64: the
                # time split of the weight-gradient kernel has a seam inside every utterance (fresh model, same rule
                # for the pre-activations)
                model = LenPredictor(n_tokens=100, n_speakers=n_spk, norm_mean=torch.tensor(3.3), norm_std=torch.tensor(2.1))
                model.load_state_dict(synth.synth_len_state_dict(100, n_spk), strict=True)
                model.train()
                seq, tgt, spk, keep, seed0, margin = _search_len_batch(model, _FakeCudaFloat, 3, 150, 300)
                out["len_long/seed"], out["len_long/min_abs_preact"] = np.array(seed0), np.array(margin)
                for nm, arr in (("seq", seq), ("tgt", tgt), ("spk", spk), ("keep", keep)):
                    out[f"len_long/{nm}"] = arr
                _FakeCudaFloat.queue.append((torch.from_numpy(keep), model.keep_rate))
                model.zero_grad()
                loss = crit(model(torch.from_numpy(seq).int(), torch.from_numpy(spk).int()), torch.from_numpy(tgt))
                loss.backward()
                out["len_long/loss"] = np.array(loss.item())
                for k, prm in model.named_parameters():
                    out[f"len_long/grad/{k}"] = compact(prm.grad.numpy())
            assert not _FakeCudaFloat.queue
    finally:
        torch.cuda.FloatTensor = real
    np.savez_compressed(os.path.join(OUT, "train.npz"), **out)
    print("train.npz", len(out), "arrays")


def make_upsample():
    """CodeGenerator.forward's `_upsample` branches (reference sr/models.py:206-210): the code stream shorter than f0 and f0 shorter
    than the code stream, by integer factors -> gen_upsample.npz (inputs + the reference's waveforms)"""
    ref_models, ref_utils = _import_ref_sr()
    h = ref_utils.AttrDict(json.load(open(os.path.join(REF, "sr/configs/VCTK/hubert100_lut.json"))))
    g = ref_models.CodeGenerator(h)
    g.load_state_dict(synth.synth_generator_state_dict(seed=0), strict=True)
    g.eval()
    g.remove_weight_norm()
    out = {}
    code, f0, spkr, _ = synth.synth_generator_inputs(1, 24, seed=4242)
    cases = {"code_short": (code[:, :12], f0[:, :, :24]), "f0_short": (code[:, :24], f0[:, :, :8]), "code_short3": (code[:, :5], f0[:, :, :15])}
    for name, (c, f) in cases.items():
        with torch.no_grad():
            y = g(code=torch.from_numpy(np.ascontiguousarray(c)), f0=torch.from_numpy(np.ascontiguousarray(f)), spkr=torch.from_numpy(spkr))
        out[f"{name}/code"], out[f"{name}/f0"], out[f"{name}/spkr"], out[f"{name}/wav"] = c, f, spkr, y.numpy()
    np.savez_compressed(os.path.join(OUT, "gen_upsample.npz"), **out)
    print("gen_upsample.npz", {k: v.shape for k, v in out.items() if k.endswith("wav")})


TARGETS = {"upsample": make_upsample, "train": make_train, "prep_dataset": make_prep_dataset, "hubert": make_hubert,
           "hubert_trained_like": make_hubert_trained_like, "sr_inference": make_sr_inference,
           "generator": make_generator, "generator_trained_like": make_generator_trained_like, "predictors": make_predictors}

if __name__ == "__main__":
    which = sys.argv[1:] or list(TARGETS)
    unknown = [w for w in which if w not in TARGETS]
    if unknown:
        sys.exit(f"unknown target(s) {unknown}; choose from {list(TARGETS)}")
    if len(which) == 1:
        TARGETS[which[0]]()
    else:
        import subprocess
        for w in which:  # a fresh interpreter per target keeps sys.path / sys.modules clean
            subprocess.check_call([sys.executable, os.path.abspath(__file__), w])
