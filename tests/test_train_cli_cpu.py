"""sr/train.py on the CPU with a fake trainer on a synthetic tree: the reference's argument defaults, the resume arithmetic, the
steps at which it checkpoints and validates, the learning rate after k epochs against torch's ExponentialLR, the refusals."""
import json
import os
import pickle
import types

import numpy as np
import pytest
import torch

import gan_train_cases as GC


@pytest.fixture(scope="module")
def cli():
    import __graft_entry__ as ge
    ge.build()
    return GC.load_train_cli()


class FakeTrainer:
    """GanTrainer's surface; records what the loop asks for"""

    def __init__(self, h, device, saved=None):
        self.h, self.device, self.saved, self.calls, self.lr, self.steps_done = h, device, saved, [], float(h["learning_rate"]), 0

    def load(self, path):
        return self.saved

    def init(self, seed):
        self.calls.append(("init", seed))

    def sampler(self, items, seed=1234):
        self.calls.append(("sampler", len(items), seed))
        return list(range(len(items) // int(self.h["batch_size"])))

    def step(self, batch):
        self.calls.append(("step", batch))
        self.steps_done += 1
        return {"loss_gen_all": torch.tensor(3.0), "mel_error": torch.tensor(0.5)}

    def save(self, path, steps, epoch):
        self.calls.append(("save", steps, epoch))

    def decay_lr(self):
        self.calls.append(("decay",))
        self.lr *= float(self.h["lr_decay"])

    def scorer(self):
        self.calls.append(("validate", self.steps_done))
        return lambda batch: (np.array([len(it["code"]) for it in batch]), np.full(len(batch), 0.25))


def test_argument_defaults_are_the_references(cli):
    a = cli.get_parser().parse_args([])
    assert (a.checkpoint_path, a.config, a.training_epochs, a.training_steps) == ("checkpoints/esd_hubert", "configs/ESD/hubert100_lut.json", 2000, 400000)
    assert (a.stdout_interval, a.checkpoint_interval, a.summary_interval, a.validation_interval) == (5, 10000, 100, 1000)
    assert (a.fine_tuning, a.local_rank, a.group_name, a.distributed_world_size, a.distributed_port) == (False, 0, None, None, None)
    cli.get_parser().parse_args(["--distributed-world-size", "1", "--distributed-port", "1234", "--local_rank", "0"])


def run(cli, tmp_path, saved, extra=()):
    config = GC.write_tree(str(tmp_path / "data"))
    made = []

    def make(h, device):
        made.append(FakeTrainer(h, device, saved))
        return made[-1]
    ck = str(tmp_path / "ck")
    end = cli.main(["--checkpoint_path", ck, "--config", config, "--stdout_interval", "2", "--checkpoint_interval", "2",
                    "--summary_interval", "2", "--validation_interval", "2", *extra], make_trainer=make)
    return made[0], end, ck


def test_fresh_run_checkpoints_and_validates_at_the_references_steps(cli, tmp_path, capsys):
    t, end, ck = run(cli, tmp_path, None, ["--training_epochs", "2", "--training_steps", "5"])
    assert t.device == "cuda:0" and t.calls[0] == ("init", 1234) and t.calls[1] == ("sampler", 6, 1234)
    # three batches per epoch: steps 0, 1, 2 in epoch 0, steps 3, 4 in epoch 1, where training_steps ends the epoch
    assert [c for c in t.calls if c[0] == "step"] == [("step", b) for b in (0, 1, 2, 0, 1)] and end == 5
    assert [c for c in t.calls if c[0] == "save"] == [("save", 2, 0), ("save", 4, 1)]  # steps % 2 == 0 and steps != 0
    assert [c for c in t.calls if c[0] == "validate"] == [("validate", n) for n in (1, 3, 5)]  # at steps 0, 2, 4, after the step
    assert sum(c == ("decay",) for c in t.calls) == 2
    with open(os.path.join(ck, "config.json")) as f:
        assert json.load(f)["segment_size"] == 80
    with open(tmp_path / "data" / "id_to_spkr.pkl", "rb") as f:
        assert pickle.load(f) == ["p0", "p1", "p2"]
    rows = [json.loads(line) for line in open(os.path.join(ck, "logs", "scalars.jsonl"))]
    assert [(r["tag"], r["step"]) for r in rows] == [(tag, s) for s in (0, 2, 4) for tag in
                                                     ("training/gen_loss_total", "training/mel_spec_error", "validation/mel_spec_error")]
    assert [r["value"] for r in rows[:3]] == [3.0, 0.5, 0.25]
    out = capsys.readouterr().out
    assert "Steps : 2, Gen Loss Total : 3.000, Mel-Spec. Error : 0.500, s/b : " in out and "Steps : 1," not in out
    assert "Epoch: 2" in out and "Finished training" in out


def test_resume_arithmetic(cli, tmp_path):
    t, end, _ = run(cli, tmp_path, {"steps": 4, "epoch": 1}, ["--training_epochs", "3", "--training_steps", "7"])
    assert not any(c[0] == "init" for c in t.calls)
    # steps = saved + 1 = 5, the loop re-enters at epoch = saved epoch 1: steps 5, 6 there, then one step per later epoch
    assert [c for c in t.calls if c[0] == "save"] == [("save", 6, 1)]
    assert end == 8 and sum(c[0] == "step" for c in t.calls) == 3 and sum(c == ("decay",) for c in t.calls) == 2


def test_learning_rate_after_k_epochs_is_exponential_lrs(cli):
    from dissc_amd import AttrDict, gan_train
    t = object.__new__(gan_train.GanTrainer)
    t.h = AttrDict({"lr_decay": 0.999})
    t.optim_g, t.optim_d = types.SimpleNamespace(lr=2e-4), types.SimpleNamespace(lr=2e-4)
    opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=2e-4)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.999)
    for k in range(1, 8):
        t.decay_lr()
        sched.step()
        assert t.lr == t.optim_d.lr == opt.param_groups[0]["lr"], k


def test_refusals(cli, tmp_path, monkeypatch):
    config = GC.write_tree(str(tmp_path / "data"))
    with open(config) as f:
        h = json.load(f)
    for key, value, word in (("f0_median", True, "f0_median"), ("num_gpus", 2, "num_gpus"), ("code_vq_params", {"x": 1}, "code_vq_params")):
        bad = str(tmp_path / f"{key}.json")
        with open(bad, "w") as f:
            json.dump(dict(h, **{key: value}), f)
        with pytest.raises(NotImplementedError, match=word):
            cli.main(["--checkpoint_path", str(tmp_path / "ck"), "--config", bad], make_trainer=FakeTrainer)
    assert not os.path.exists(tmp_path / "ck")  # refused before anything is written
    monkeypatch.setenv("WORLD_SIZE", "8")
    with pytest.raises(NotImplementedError, match="WORLD_SIZE"):
        cli.main(["--checkpoint_path", str(tmp_path / "ck"), "--config", config], make_trainer=FakeTrainer)
    monkeypatch.delenv("WORLD_SIZE")
    with open(str(tmp_path / "big.json"), "w") as f:
        json.dump(dict(h, batch_size=7), f)
    with pytest.raises(ValueError, match="do not fill one batch"):
        cli.main(["--checkpoint_path", str(tmp_path / "ck"), "--config", str(tmp_path / "big.json")], make_trainer=FakeTrainer)
