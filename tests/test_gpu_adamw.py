"""dissc_amd.nn.AdamW on the GPU (csrc/adamw.hip): one launch over tensors at every edge of the chunk and of the float4 body, an
unaligned view, a tensor without a grad and one whose step count lags; p, exp_avg and exp_avg_sq after three steps with a changing
learning rate against the float64 replay of tests/adamw_ref.py with float32 torch.optim.AdamW(foreach=False) on the CPU as the
yardstick, bar 4 in each stratum of |g|; equal bits from run to run, from list to list and from the float4 to the scalar path;
grads and the skipped tensor untouched; the state dictionary through torch.optim.AdamW and back; refusals by name."""
import numpy as np
import pytest
import torch

import adamw_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BETAS, EPS, WD = (0.8, 0.99), 1e-8, 1e-2
LRS = (2e-4, 1e-3, 5e-5)
UNALIGNED, NO_GRAD, LATE = 8, 9, 10  # indices in sizes(): a one-element-offset view, never a grad, no grad at step 0


@pytest.fixture(scope="module")
def nn():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import nn
    return nn


def bits(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.int32)


def sizes(nn):
    c = nn.ADAMW_CHUNK
    return [1, 3, 4, 5, c - 1, c, c + 1, 2 * c + 3, c + 6, 7, 2 * c + 1]


@pytest.fixture(scope="module")
def case(nn):
    rs = np.random.RandomState(11)
    ns = sizes(nn)
    params = [rs.uniform(-1, 1, n).astype(np.float32) for n in ns]
    steps = [[None if i == NO_GRAD or (i == LATE and s == 0) else A.heavy_grads(rs, n) for i, n in enumerate(ns)] for s in range(3)]
    kw = dict(betas=BETAS, eps=EPS, wd=WD)
    return dict(params=params, steps=steps, r64=A.replay(params, steps, LRS, dtype=np.float64, **kw),
                r32=A.torch_replay(params, steps, LRS, **kw))


def leaves(case, which=None, align_all=False):
    """device leaves of the case's tensors (``which``: a subset); tensor UNALIGNED is a view one element into its buffer"""
    out = []
    for i in (range(len(case["params"])) if which is None else which):
        x = torch.from_numpy(case["params"][i])
        if i == UNALIGNED and not align_all:
            buf = torch.zeros(x.numel() + 1, device=DEV)
            buf[1:] = x.to(DEV)
            p = buf[1:].detach().requires_grad_(True)
            assert p.data_ptr() % 16 == 4
        else:
            p = x.to(DEV).requires_grad_(True)
            assert p.data_ptr() % 16 == 0
        out.append(p)
    return out


def run(nn, case, which=None, align_all=False):
    idx = list(range(len(case["params"]))) if which is None else list(which)
    ps = leaves(case, idx, align_all)
    opt = nn.AdamW(ps, lr=LRS[0], betas=BETAS, eps=EPS, weight_decay=WD)
    for s, lr in enumerate(LRS):
        opt.lr = lr
        grads = []
        for p, i in zip(ps, idx):
            g = case["steps"][s][i]
            p.grad = None if g is None else torch.from_numpy(g).to(DEV)
            grads.append(None if g is None else p.grad.clone())
        opt.step()
        torch.cuda.synchronize()
        for p, g in zip(ps, grads):  # grads are never written
            assert (p.grad is None) == (g is None) and (g is None or torch.equal(bits(p.grad), bits(g)))
    return ps, opt


def test_three_steps_against_the_float64_replay(nn, case):
    ps, opt = run(nn, case)
    bad = []
    for i, p in enumerate(ps):
        if i == NO_GRAD:
            assert i not in opt.state and torch.equal(bits(p), bits(torch.from_numpy(case["params"][i])))
            continue
        st = opt.state[i]
        assert st["step"] == case["r32"][3][i] == (2 if i == LATE else 3)
        for q, y in enumerate((p, st["exp_avg"], st["exp_avg_sq"])):
            bad += A.strata_check(f"t{i} n={p.numel()} {('p', 'exp_avg', 'exp_avg_sq')[q]}", y.detach().cpu().numpy(), case["r64"][q][i],
                                  case["r32"][q][i], case["steps"][-1][i])
    assert not bad, bad


def test_bits_do_not_depend_on_the_run_the_list_or_the_alignment(nn, case):
    ps, opt = run(nn, case)
    ps2, opt2 = run(nn, case)
    sub = [6, UNALIGNED, LATE, 0]
    ps3, opt3 = run(nn, case, which=sub)
    ps4, opt4 = run(nn, case, align_all=True)
    same = lambda a, b: torch.equal(bits(a), bits(b))
    everything = list(range(len(ps)))
    for tag, other, o, idx in (("run", ps2, opt2, everything), ("list", ps3, opt3, sub), ("alignment", ps4, opt4, everything)):
        for j, i in enumerate(idx):
            if i == NO_GRAD:
                continue
            assert same(ps[i], other[j]), (tag, i)
            assert same(opt.state[i]["exp_avg"], o.state[j]["exp_avg"]) and same(opt.state[i]["exp_avg_sq"], o.state[j]["exp_avg_sq"]), (tag, i)


def test_state_dict_goes_through_torch_and_back(nn, case):
    ps, opt = run(nn, case)
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [i for i in range(len(ps)) if i != NO_GRAD]
    theirs = torch.optim.AdamW(ps, lr=1.0)
    assert set(theirs.state_dict()["param_groups"][0]) | {"initial_lr"} == set(sd["param_groups"][0])
    theirs.load_state_dict(sd)
    assert theirs.param_groups[0]["lr"] == LRS[-1] and tuple(theirs.param_groups[0]["betas"]) == BETAS
    assert theirs.param_groups[0]["initial_lr"] == LRS[0]
    back = theirs.state_dict()
    opt2 = nn.AdamW(ps, lr=1.0)
    opt2.load_state_dict(back)
    assert (opt2.lr, opt2.betas, opt2.eps, opt2.weight_decay, opt2.initial_lr) == (LRS[-1], BETAS, EPS, WD, LRS[0])
    assert sorted(opt2.state) == sorted(opt.state)
    for i, s in opt.state.items():
        assert sd["state"][i]["step"].dtype == torch.float32 and sd["state"][i]["step"].dim() == 0
        assert opt2.state[i]["step"] == s["step"]
        for what in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(bits(opt2.state[i][what]), bits(s[what])) and opt2.state[i][what].data_ptr() != s[what].data_ptr()
    # and the two go on in step: one more update from either gives equal bits
    for p in ps:
        p.grad = None
    ps[5].grad = torch.full_like(ps[5], 0.25)
    before = ps[5].detach().clone()
    opt.step()
    a = ps[5].detach().clone()
    with torch.no_grad():
        ps[5].copy_(before)
    opt2.step()
    torch.cuda.synchronize()
    assert torch.equal(bits(a), bits(ps[5])) and opt2.state[5]["step"] == 4


def test_refusals(nn):
    good = lambda n=8: torch.zeros(n, device=DEV, requires_grad=True)
    for bad, name in ((torch.zeros(8, requires_grad=True), "CPU"), (torch.zeros(8, device=DEV, dtype=torch.float64), "float64"),
                      (torch.zeros(16, device=DEV)[::2], "strided"), (good() * 2, "no leaf"), (torch.zeros(0, device=DEV), "empty")):
        with pytest.raises(nn.DisscError, match=r"params\[1\]"):
            nn.AdamW([good(), bad])
    with pytest.raises(nn.DisscError, match="17 tensors"):
        nn.AdamW([good() for _ in range(nn.ADAMW_MAX_TENSORS + 1)])
    with pytest.raises(nn.DisscError, match="0 tensors"):
        nn.AdamW([])
    for kw in (dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(eps=-1e-8), dict(lr=-1.0), dict(weight_decay=-0.1)):
        with pytest.raises(ValueError):
            nn.AdamW([good()], **kw)
    ps = [good(), good()]
    opt = nn.AdamW(ps)
    ps[0].grad = torch.ones(8, device=DEV)
    ps[1].grad = torch.ones(16, device=DEV)[::2]
    keep = [p.detach().clone() for p in ps]
    with pytest.raises(nn.DisscError, match=r"grad of params\[1\]"):
        opt.step()
    torch.cuda.synchronize()
    assert not opt.state and all(torch.equal(bits(a), bits(b)) for a, b in zip(keep, ps))  # refused before any launch
    with pytest.raises(nn.DisscError, match="param group"):
        opt.load_state_dict({"state": {}, "param_groups": [dict(opt.state_dict()["param_groups"][0], params=[0])]})
    opt.zero_grad()
    assert all(p.grad is None for p in ps)
    opt.step()  # nothing to do: no launch, no state
    assert not opt.state


def test_shared_memory_and_bad_state_index_are_refused(nn):
    buf = torch.zeros(16, device=DEV)
    a, b = buf[:8].detach().requires_grad_(True), buf[4:12].detach().requires_grad_(True)
    with pytest.raises(nn.DisscError, match="share memory"):
        nn.AdamW([a, b])
    with pytest.raises(nn.DisscError, match="share memory"):
        nn.AdamW([a, a])
    opt = nn.AdamW([torch.zeros(8, device=DEV, requires_grad=True)])
    sd = opt.state_dict()
    sd["state"][3] = {"step": torch.tensor(1.0), "exp_avg": torch.zeros(8), "exp_avg_sq": torch.zeros(8)}
    with pytest.raises(nn.DisscError, match=r"state\[3\]"):
        opt.load_state_dict(sd)
