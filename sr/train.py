#!/usr/bin/env python
"""The vocoder's GAN training on one MI355X (reference sr/train.py): a checkpoint directory goes in, ``g_*`` / ``do_*`` files come
out, in the reference's format both ways.

    python sr/train.py --checkpoint_path checkpoints/vctk_hubert --config CONFIG.json
           [--training_epochs 2000] [--training_steps 400000] [--stdout_interval 5] [--checkpoint_interval 10000]
           [--summary_interval 100] [--validation_interval 1000] [--precision {fp32,split_bf16}]

The reference's arguments with its defaults (``--fine_tuning``, ``--local_rank`` and the two ``--distributed-*`` ones are
accepted); the config is copied to ``config.json`` in the checkpoint directory, ``id_to_spkr.pkl`` is written next to
``input_training_file``; the reference's epoch / step loop, its stdout line, checkpoints at ``steps % checkpoint_interval == 0 and
steps != 0``, resume at ``steps = saved + 1`` and ``last_epoch = saved epoch`` from the latest ``g_*`` / ``do_*``.  ``--precision``
(not the reference's; default ``fp32``) is ``GanTrainer``'s: ``split_bf16`` runs the ``nn.conv1d`` layers of the three modules on
the bf16 matrix cores in split arithmetic; checkpoints do not record it, so a run may resume in either.  The step itself
is ``dissc_amd.gan_train.GanTrainer``; the batches are ``SegmentSampler``'s (the corpus is prepared once by sr/validate.py's
``prepare_items`` and lives on the device).  As in the reference, ``--training_steps`` ends an epoch, not the run: every later
epoch still takes one step, so give ``--training_epochs`` too for a short run.

Validation goes through sr/validate.py's own functions (``prepare_items``, ``score_items``, a ``GeneratorScorer`` on the live
generator's ``state_dict()``): the figure logged as ``validation/mel_spec_error`` is validate.py's, whose docstring lists its
differences from the reference trainer's (whole utterances, no crops).  Every validation builds a fresh scorer from a host copy
of the generator's weights and packs them for inference again: nothing at the default interval of 1 000 steps, a cost to keep
in mind when ``--validation_interval`` is set small.  Scalars go to ``logs/scalars.jsonl`` always, and to
TensorBoard too where ``torch.utils.tensorboard`` imports.

Refused by name: ``WORLD_SIZE`` / ``num_gpus`` above 1 (no gradient all-reduce), the VQ-VAE options, ``f0_median``; the audio and
figure summaries of the reference's validation are not written.
"""
import argparse
import json
import os
import pickle
import shutil
import sys
import time
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _validate():
    """sr/validate.py as a module (prepare_items, score_items, summarise, GeneratorScorer live there)"""
    import importlib.util
    if "dissc_sr_validate" not in sys.modules:
        spec = importlib.util.spec_from_file_location("dissc_sr_validate", os.path.join(ROOT, "sr", "validate.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        sys.modules["dissc_sr_validate"] = mod
    return sys.modules["dissc_sr_validate"]


def get_parser():
    """the reference's arguments and defaults (sr/train.py:293-307)"""
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--group_name", default=None)
    parser.add_argument("--checkpoint_path", default="checkpoints/esd_hubert")
    parser.add_argument("--config", default="configs/ESD/hubert100_lut.json")
    parser.add_argument("--training_epochs", default=2000, type=int)
    parser.add_argument("--training_steps", default=400000, type=int)
    parser.add_argument("--stdout_interval", default=5, type=int)
    parser.add_argument("--checkpoint_interval", default=10000, type=int)
    parser.add_argument("--summary_interval", default=100, type=int)
    parser.add_argument("--validation_interval", default=1000, type=int)
    parser.add_argument("--fine_tuning", default=False, type=bool)
    parser.add_argument("--local_rank", default=0, type=int)
    parser.add_argument("--distributed-world-size", type=int)
    parser.add_argument("--distributed-port", type=int)
    parser.add_argument("--precision", default="fp32", choices=("fp32", "split_bf16"))  # (this trainer's own)
    return parser


def build_env(config, config_name, path):
    """the reference's sr/utils.py: the config next to the checkpoints"""
    target = os.path.join(path, config_name)
    os.makedirs(path, exist_ok=True)
    if os.path.abspath(config) != os.path.abspath(target):
        shutil.copyfile(config, target)


def load_data(h):
    """-> (training items, validation items, id_to_spkr): both manifests prepared by sr/validate.py's prepare_items; id_to_spkr as
    CodeDataset builds it (the sorted set of parse_speaker over the training files) and pickled next to input_training_file"""
    from dissc_amd import formats
    V = _validate()
    read = lambda path: [s for s in formats.read_manifest(path) if "units" in s]
    train, val = read(h["input_training_file"]), read(h["input_validation_file"])
    id_to_spkr = []
    if h.get("multispkr", None):
        files = [Path(str(h["train_base_path"]) + "/" + s["audio"].split("/")[-1]) for s in train]
        id_to_spkr = sorted(set(formats.parse_speaker(f, h["multispkr"]) for f in files))
    with open(os.path.join(os.path.dirname(h["input_training_file"]) or ".", "id_to_spkr.pkl"), "wb") as f:
        pickle.dump(id_to_spkr, f)
    stats = None
    if h.get("f0_normalize", False) and h.get("f0_stats", None):
        with open(h["f0_stats"], "rb") as f:
            stats = pickle.load(f)
    train_items, _ = V.prepare_items(h, train, id_to_spkr, stats, h["train_base_path"])
    mirror = (int(h["n_fft"]) - int(h["hop_size"])) // 2
    val_items, skipped = V.prepare_items(h, val, id_to_spkr, stats, h["val_base_path"], min_samples=mirror + 1)
    for name, why in skipped:
        print(f"validation skips {name}: {why}")
    return train_items, val_items, id_to_spkr


class ScalarLog:
    """logs/scalars.jsonl, one {"tag", "value", "step"} per line; TensorBoard too where torch.utils.tensorboard imports"""

    def __init__(self, log_dir):
        os.makedirs(log_dir, exist_ok=True)
        self.f = open(os.path.join(log_dir, "scalars.jsonl"), "a")
        try:
            from torch.utils.tensorboard import SummaryWriter
            self.sw = SummaryWriter(log_dir)
        except Exception:
            self.sw = None

    def add_scalar(self, tag, value, step):
        self.f.write(json.dumps({"tag": tag, "value": float(value), "step": int(step)}) + "\n")
        self.f.flush()
        if self.sw is not None:
            self.sw.add_scalar(tag, float(value), step)

    def close(self):
        self.f.close()
        if self.sw is not None:
            self.sw.close()


def train(a, h, trainer, train_items, val_items, log):
    """the reference's loop (sr/train.py:55-70, 126-287) around ``trainer`` (GanTrainer's surface: load, init, sampler, step, save,
    decay_lr, generator_state_dict or scorer) -> the step count it ends at"""
    V = _validate()
    found = trainer.load(a.checkpoint_path)
    if found is None:
        trainer.init(int(h.get("seed", 1234)))
        steps, last_epoch = 0, -1
    else:
        steps, last_epoch = found["steps"] + 1, found["epoch"]
    sampler = trainer.sampler(train_items, seed=1234)
    for epoch in range(max(0, last_epoch), a.training_epochs):
        start = time.time()
        print("Epoch: {}".format(epoch + 1))
        for batch in sampler:
            start_b = time.time()
            losses = trainer.step(batch)
            if steps % a.stdout_interval == 0:
                print("Steps : {:d}, Gen Loss Total : {:4.3f}, Mel-Spec. Error : {:4.3f}, s/b : {:4.3f}".format(
                    steps, float(losses["loss_gen_all"]), float(losses["mel_error"]), time.time() - start_b))
            if steps % a.checkpoint_interval == 0 and steps != 0:
                trainer.save(a.checkpoint_path, steps, epoch)
            if steps % a.summary_interval == 0:
                log.add_scalar("training/gen_loss_total", float(losses["loss_gen_all"]), steps)
                log.add_scalar("training/mel_spec_error", float(losses["mel_error"]), steps)
            if steps % a.validation_interval == 0:
                scorer = trainer.scorer() if hasattr(trainer, "scorer") else \
                    V.GeneratorScorer(h, trainer.generator_state_dict(), f"cuda:{a.local_rank}")
                rows = V.score_items(val_items, scorer, int(h.get("batch_size", 32)))
                log.add_scalar("validation/mel_spec_error", V.summarise(rows)["mel_spec_error"], steps)
            steps += 1
            if steps >= a.training_steps:
                break
        trainer.decay_lr()
        print("Time taken for epoch {} is {} sec\n".format(epoch + 1, int(time.time() - start)))
    print("Finished training")
    return steps


def main(argv=None, make_trainer=None):
    """make_trainer(h, device) -> the trainer (default: dissc_amd.gan_train.GanTrainer at --precision), as validate.main takes
    make_scorer"""
    print("Initializing Training Process..")
    a = get_parser().parse_args(argv)
    print("precision : ", a.precision)
    from dissc_amd import AttrDict, gan_train
    with open(a.config) as f:
        h = AttrDict(json.loads(f.read()))
    gan_train.refuse_unsupported(h)
    build_env(a.config, "config.json", a.checkpoint_path)
    train_items, val_items, _ = load_data(h)
    if len(train_items) < int(h["batch_size"]):
        raise ValueError(f"{len(train_items)} training items do not fill one batch of {h['batch_size']} (drop_last)")
    trainer = make_trainer(h, f"cuda:{a.local_rank}") if make_trainer else \
        gan_train.GanTrainer(h, f"cuda:{a.local_rank}", precision=a.precision)
    print("checkpoints directory : ", a.checkpoint_path)
    log = ScalarLog(os.path.join(a.checkpoint_path, "logs"))
    try:
        return train(a, h, trainer, train_items, val_items, log)
    finally:
        log.close()


if __name__ == "__main__":
    main()
