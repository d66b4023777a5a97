#!/usr/bin/env python
"""Mel-spectrogram error of a vocoder checkpoint on the MI355X: the figure the reference's trainer logs as
``validation/mel_spec_error`` (reference sr/train.py:231-269), for picking ``g_*`` checkpoints and for judging the opt-in
precision modes.

    python sr/validate.py --checkpoint_file checkpoints/vctk_hubert/ [--all]
           [--input_code_file VAL.txt] [--data_path DIR] [--id_to_spkr PKL]
           [--pad N] [--precision fp32|split_bf16] [--output_dir DIR]

Defaults: the manifest is the config's ``input_validation_file``, the wavs come from ``val_base_path``, ``id_to_spkr.pkl``
sits next to ``input_training_file`` (where the trainer writes it).  Every manifest line is prepared as the trainer's
validation set prepares it (CodeDataset with eval_mode False, reference sr/dataset.py:221-317) with the code of
sr/inference.py: ground truth through ``load_gt``, code and F0 cut to the same hop count, F0 normalised by the source
speaker's statistics, source speaker id.  The generator runs in length-sorted batches and
``dissc_amd.MelSpectrogram.l1`` (``fmax_for_loss``) scores ground truth against output without storing either mel.

Prints ``validation/mel_spec_error`` (mean over utterances, as the trainer's mean over its batches of one) and the
frame-weighted mean, writes ``mel_spec_error.json`` with one row per file; ``--all`` scores every ``g_*`` of the directory
and lists them best first.

The figure is comparable in kind to the trainer's, not equal to it: whole utterances instead of seeded random
``segment_size`` crops; no ``drop_last``; utterances shorter than a segment are not doubled; utterances too short to be
mirrored by (n_fft - hop) / 2 samples are skipped with a message.  Single process.
"""
import argparse
import glob
import json
import os
import pickle
import sys
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PRECISIONS = ("fp32", "split_bf16")


def _inference():
    """sr/inference.py as a module (load_gt, build_jobs, scan_checkpoint live there)"""
    import importlib.util
    if "dissc_sr_inference" not in sys.modules:
        spec = importlib.util.spec_from_file_location("dissc_sr_inference", os.path.join(ROOT, "sr", "inference.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        sys.modules["dissc_sr_inference"] = mod
    return sys.modules["dissc_sr_inference"]


def prepare_items(h, samples, id_to_spkr, f0_stats_cfg, base_path, pad=None, min_samples=1):
    """manifest entries -> ([{name, code i64 [T], f0 f32 [T], spkr, gt f32 [T * code_hop_size]}], [(name, why skipped)]).
    The jobs are sr/inference.py's own (build_jobs with the ground-truth clipping of eval_mode False and no conversion)."""
    inf = _inference()
    a = argparse.Namespace(sample_df=None, target_speakers=None, data_path=base_path, debug=True, n=-1, parts=False,
                           eval_mode=False, pad=pad, unseen_speaker=False, vc=False)
    jobs, stems = inf.build_jobs(a, h, samples, id_to_spkr, f0_stats_cfg, None)
    assert len(jobs) == len(stems)
    hop = int(h["code_hop_size"])
    items, skipped = [], []
    for job, (stem, audio_path, code_len) in zip(jobs, stems):
        gt = inf.load_gt(str(audio_path), code_len, pad, h["sampling_rate"], hop)
        if gt is None or len(gt) != code_len * hop:
            raise ValueError(f"{audio_path}: ground truth of {0 if gt is None else len(gt)} samples for {code_len} units")
        if len(gt) < min_samples:
            skipped.append((audio_path.name, f"{len(gt)} samples: too short to mirror"))
            continue
        items.append(dict(name=audio_path.name, code=job["code"], f0=job["f0"], spkr=job["spkr"], gt=gt))
    return items, skipped


def score_items(items, scorer, max_batch=32, max_frames=None):
    """scorer(batch of items) -> (frames [B], mel error [B]); batches are harness.make_batches' (longest first).
    -> rows {name, frames, error} in manifest order"""
    from dissc_amd import harness
    lengths = [len(it["code"]) for it in items]
    kw = {} if max_frames is None else {"max_frames": max_frames}
    rows = [None] * len(items)
    for batch in harness.make_batches(range(len(items)), lengths, max_batch, **kw):
        frames, err = scorer([items[i] for i in batch])
        for k, i in enumerate(batch):
            rows[i] = {"name": items[i]["name"], "frames": int(frames[k]), "error": float(err[k])}
    return rows


def summarise(rows):
    """mean over utterances (the trainer's figure) and the mean weighted by frames"""
    if not rows:
        return {"mel_spec_error": float("nan"), "frame_weighted": float("nan"), "files": 0, "frames": 0}
    err = np.array([r["error"] for r in rows], np.float64)
    fr = np.array([r["frames"] for r in rows], np.float64)
    return {"mel_spec_error": float(err.mean()), "frame_weighted": float((err * fr).sum() / fr.sum()), "files": len(rows),
            "frames": int(fr.sum())}


def checkpoints_of(path, every=False):
    """the checkpoint(s) to score and the config next to them: a directory means its latest g_* (--all: each one)"""
    inf = _inference()
    if os.path.isdir(path):
        cps = sorted(glob.glob(os.path.join(path, "g_*"))) if every else [inf.scan_checkpoint(path, "g_")]
        return [c for c in cps if c], os.path.join(path, "config.json")
    return [path], os.path.join(os.path.split(path)[0], "config.json")


class GeneratorScorer:
    """one checkpoint on one GPU: generator forward, then the fused mel L1 against the ground truth"""

    def __init__(self, h, state_dict, device="cuda:0", precision="fp32"):
        import torch
        from dissc_amd import CodeGenerator, MelSpectrogram
        self.torch, self.device = torch, torch.device(device)
        g = CodeGenerator(h, precision=precision).to(self.device)
        g.load_state_dict(state_dict)
        g.eval()
        g.remove_weight_norm()
        g.prepare()
        self.generator = g
        self.mel = MelSpectrogram.from_config(h, for_loss=True).to(self.device)
        self.hop = int(np.prod(h["upsample_rates"]))

    def generate(self, batch):
        """-> (waveforms f32 [B, hop * Tmax] on the device, samples per utterance)"""
        torch = self.torch
        B, T = len(batch), max(len(it["code"]) for it in batch)
        code, f0 = np.zeros((B, T), np.int64), np.zeros((B, 1, T), np.float32)
        for k, it in enumerate(batch):
            code[k, :len(it["code"])] = it["code"]
            f0[k, 0, :len(it["code"])] = it["f0"]
        lens = np.array([len(it["code"]) for it in batch], np.int32)
        spkr = np.array([[it["spkr"]] for it in batch], np.int64)
        y = self.generator(code=torch.from_numpy(code).to(self.device), f0=torch.from_numpy(f0).to(self.device),
                           spkr=torch.from_numpy(spkr).to(self.device), lengths=torch.from_numpy(lens).to(self.device))
        return y.view(B, -1), lens.astype(np.int64) * self.hop

    def __call__(self, batch):
        y, ns = self.generate(batch)
        gt = np.zeros((len(batch), y.shape[1]), np.float32)
        for k, it in enumerate(batch):
            if len(it["gt"]) != ns[k]:
                raise ValueError(f"{it['name']}: {len(it['gt'])} ground-truth samples, {ns[k]} generated")
            gt[k, :ns[k]] = it["gt"]
        out = self.mel.l1(gt, y, ns)
        return ns // self.mel.hop_size, out["mean"].cpu().numpy()


def report(path, results):
    """mel_spec_error.json: per checkpoint the summary and the per-file rows"""
    with open(path, "w") as f:
        json.dump({"checkpoints": results}, f, indent=1)


def main(argv=None, make_scorer=None):
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--checkpoint_file", default="checkpoints/vctk_hubert/")
    parser.add_argument("--all", action="store_true", help="score every g_* of the checkpoint directory")
    parser.add_argument("--input_code_file", default=None, help="default: the config's input_validation_file")
    parser.add_argument("--data_path", default=None, help="directory of the ground-truth wavs (default: val_base_path)")
    parser.add_argument("--id_to_spkr", default=None, type=Path, help="default: next to the config's input_training_file")
    parser.add_argument("--pad", default=None, type=int)
    parser.add_argument("--precision", default="fp32", choices=PRECISIONS)
    parser.add_argument("--output_dir", default=None, help="where mel_spec_error.json goes (default: the checkpoint directory)")
    parser.add_argument("--device", default="cuda:0")
    parser.add_argument("--max_batch", default=32, type=int)
    a = parser.parse_args(argv)

    from dissc_amd import AttrDict, formats
    cps, config_file = checkpoints_of(a.checkpoint_file, a.all)
    if not cps:
        print(f"Didn't find checkpoints under {a.checkpoint_file}")
        return None
    with open(config_file) as f:
        h = AttrDict(json.loads(f.read()))
    samples = [s for s in formats.read_manifest(a.input_code_file or h["input_validation_file"]) if "units" in s]
    id_to_spkr = []
    if h.get("multispkr", None):
        id_to_spkr = formats.load_pickle(a.id_to_spkr or f"{os.path.dirname(h.input_training_file)}/id_to_spkr.pkl")
    f0_stats_cfg = None
    if h.get("f0_normalize", False) and h.get("f0_stats", None):
        with open(h["f0_stats"], "rb") as f:
            f0_stats_cfg = pickle.load(f)
    base = a.data_path if a.data_path is not None else h.get("val_base_path", "")
    pad_mirror = (int(h["n_fft"]) - int(h["hop_size"])) // 2
    items, skipped = prepare_items(h, samples, id_to_spkr, f0_stats_cfg, base, a.pad, min_samples=pad_mirror + 1)
    for name, why in skipped:
        print(f"skipped {name}: {why}")

    if make_scorer is None:
        def make_scorer(cp):
            import torch
            return GeneratorScorer(h, torch.load(cp, map_location="cpu")["generator"], a.device, a.precision)

    results = []
    for cp in cps:
        rows = score_items(items, make_scorer(cp), a.max_batch)
        results.append(dict(summarise(rows), checkpoint=os.path.basename(cp), precision=a.precision, rows=rows))
    results.sort(key=lambda r: (r["mel_spec_error"], r["checkpoint"]))
    for r in results:
        lead = f"{r['checkpoint']}  " if a.all else ""
        print(f"{lead}validation/mel_spec_error: {r['mel_spec_error']:.6f}   frame-weighted: {r['frame_weighted']:.6f}   "
              f"({r['files']} files, {r['frames']} frames)")
    out_dir = a.output_dir or (a.checkpoint_file if os.path.isdir(a.checkpoint_file) else os.path.dirname(a.checkpoint_file))
    os.makedirs(out_dir or ".", exist_ok=True)
    report(os.path.join(out_dir or ".", "mel_spec_error.json"), results)
    return results


if __name__ == "__main__":
    main()
