"""nn.optimizer_state_to_reference / _from_reference and the modules' named_views() on the CPU: the flat-leaf optimiser state
against torch.optim.AdamW over torch restatements of the three modules in the reference's registration order (msd_cases.TorchMSD,
mpd_cases.TorchMPD, a weight-normed generator skeleton)."""
import itertools

import pytest
import torch

import gen_train_ref as GT
from gan_train_cases import GenSkeleton
import mpd_cases as MP
import msd_cases as M

PERIODS = (2, 3)  # two of the five period discriminators: every layer kind, a fifth of the floats


@pytest.fixture(scope="module")
def nn():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import nn
    return nn


@pytest.fixture(scope="module")
def sides(nn):
    """name -> (our modules, their torch restatements), in each optimiser's order (optim_d: msd first)"""
    h = GT.SMALL_CONFIG
    return {"optim_g": ([nn.CodeGenerator(h)], [GenSkeleton(h)]),
            "optim_d": ([nn.MultiScaleDiscriminator(), nn.MultiPeriodDiscriminator(PERIODS)], [M.TorchMSD(), MP.TorchMPD(PERIODS)])}


def named_params(torch_modules):
    return list(itertools.chain.from_iterable(m.named_parameters() for m in torch_modules))


def group(n):
    return {"lr": 2e-4, "betas": (0.8, 0.99), "eps": 1e-8, "weight_decay": 0.01, "amsgrad": False, "maximize": False, "foreach": None,
            "capturable": False, "differentiable": False, "fused": None, "decoupled_weight_decay": True, "initial_lr": 2e-4,
            "params": list(range(n))}


@pytest.mark.parametrize("which", ["optim_g", "optim_d"])
def test_named_views_follow_named_parameters(sides, which):
    ours, theirs = sides[which]
    keys = [k for m in ours for k in m.named_views(*[torch.zeros(s) for s in m.leaf_shapes()])]
    views = [v for m in ours for v in m.named_views(*[torch.zeros(s) for s in m.leaf_shapes()]).values()]
    ref = named_params(theirs)
    assert keys == [k for k, _ in ref]
    assert [tuple(v.shape) for v in views] == [tuple(p.shape) for _, p in ref]


@pytest.mark.parametrize("which", ["optim_g", "optim_d"])
def test_export_loads_into_torch_with_the_planted_values(nn, sides, which):
    ours, theirs = sides[which]
    flat, planted, at = {}, [], 0
    for m in ours:
        ms, vs = [torch.zeros(s) for s in m.leaf_shapes()], [torch.zeros(s) for s in m.leaf_shapes()]
        for (key, a), b in zip(m.named_views(*ms).items(), m.named_views(*vs).values()):
            a.fill_(len(planted) + 0.25), b.fill_(-float(len(planted)) - 0.5)
            planted.append(key)
        for j in range(len(ms)):
            flat[at + j] = {"step": torch.tensor(7.0 + at + j), "exp_avg": ms[j], "exp_avg_sq": vs[j]}
        at += len(ms)
    out = nn.optimizer_state_to_reference({"state": flat, "param_groups": [group(at)]}, ours)
    ref = named_params(theirs)
    assert out["param_groups"][0]["params"] == list(range(len(ref))) and out["param_groups"][0]["initial_lr"] == 2e-4
    opt = torch.optim.AdamW([p for _, p in ref], lr=1.0)
    opt.load_state_dict(out)
    assert opt.param_groups[0]["lr"] == 2e-4 and opt.param_groups[0]["betas"] == (0.8, 0.99)
    steps = set()
    for j, (key, p) in enumerate(ref):
        s = opt.state[p]
        assert key == planted[j]
        assert s["exp_avg"].shape == p.shape and s["exp_avg_sq"].shape == p.shape, key
        assert bool((s["exp_avg"] == j + 0.25).all()) and bool((s["exp_avg_sq"] == -float(j) - 0.5).all()), key
        assert s["step"].dtype == torch.float32 and s["step"].dim() == 0
        steps.add(float(s["step"]))
    assert steps == {7.0 + j for j in range(at)}  # every leaf's own step reached its parameters


@pytest.mark.parametrize("which", ["optim_g", "optim_d"])
def test_torch_state_after_two_steps_round_trips_bit_for_bit(nn, sides, which):
    ours, theirs = sides[which]
    ps = [p for _, p in named_params(theirs)]
    opt = torch.optim.AdamW(ps, lr=2e-4, betas=(0.8, 0.99))
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.999)
    gen = torch.Generator().manual_seed(3)
    for _ in range(2):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=gen)
        opt.step()
    sched.step()
    sd = opt.state_dict()
    flat = nn.optimizer_state_from_reference(sd, ours)
    n_leaves = sum(len(m.leaf_shapes()) for m in ours)
    assert sorted(flat["state"]) == list(range(n_leaves)) and flat["param_groups"][0]["params"] == list(range(n_leaves))
    assert all(float(s["step"]) == 2.0 for s in flat["state"].values())
    back = nn.optimizer_state_to_reference(flat, ours)
    assert back["param_groups"] == sd["param_groups"]
    assert sorted(back["state"]) == sorted(sd["state"])
    for j, s in sd["state"].items():
        for what in ("step", "exp_avg", "exp_avg_sq"):
            a, b = back["state"][j][what], s[what]
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.int32), b.reshape(-1).view(torch.int32)), (j, what)
    # and torch loads what came back
    torch.optim.AdamW(ps, lr=1.0).load_state_dict(back)


def test_import_refusals(nn, sides):
    ours, theirs = sides["optim_g"]
    ref = named_params(theirs)
    full = lambda: {"state": {j: {"step": torch.tensor(2.0), "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
                              for j, (_, p) in enumerate(ref)}, "param_groups": [group(len(ref))]}
    nn.optimizer_state_from_reference(full(), ours)
    sd = full()
    sd["state"][4]["step"] = torch.tensor(3.0)  # ups.0.weight_g: one parameter of the weight_g leaf ahead of the others
    with pytest.raises(nn.DisscError, match="different steps"):
        nn.optimizer_state_from_reference(sd, ours)
    sd = full()
    del sd["state"][0]  # conv_pre.bias without state, the other biases with
    with pytest.raises(nn.DisscError, match="different steps"):
        nn.optimizer_state_from_reference(sd, ours)
    sd = full()
    sd["state"][2]["exp_avg"] = torch.zeros(3)
    with pytest.raises(nn.DisscError, match="conv_pre.weight_v"):
        nn.optimizer_state_from_reference(sd, ours)
    sd = full()
    sd["param_groups"][0]["params"] = list(range(len(ref) - 1))
    with pytest.raises(nn.DisscError, match="param group"):
        nn.optimizer_state_from_reference(sd, ours)
    with pytest.raises(nn.DisscError, match="named_views"):
        ours[0].named_views(torch.zeros(3))
    # a leaf that never stepped has no state on either side
    sd = full()
    for j, (k, _) in enumerate(ref):
        if k in ("dict.weight", "spkr.weight"):
            del sd["state"][j]
    flat = nn.optimizer_state_from_reference(sd, ours)
    assert sorted(flat["state"]) == [0, 1, 2]
    assert sorted(nn.optimizer_state_to_reference(flat, ours)["state"]) == list(range(len(ref) - 2))
