"""The AdamW update of csrc/adamw.hip as tests/adamw_ref.py restates it, on the CPU: the float32 replay stays inside the bar of
tests/test_gpu_adamw.py against float32 torch.optim.AdamW (the yardstick) in every stratum of |g|, and each seeded defect of
the helper is caught by one assertion of the same comparison."""
import numpy as np
import pytest

import adamw_ref as A

BETAS, EPS, WD = (0.8, 0.99), 1e-8, 1e-2
LRS = (2e-4, 1e-3, 5e-5)


@pytest.fixture(scope="module")
def case():
    """two tensors, three steps with the learning rate changed between them; tensor 1 has no grad at step 0, so its step count
    lags the optimiser's"""
    rs = np.random.RandomState(7)
    params = [rs.uniform(-1, 1, 6000).astype(np.float32), rs.uniform(-1, 1, 5000).astype(np.float32)]
    steps = [[A.heavy_grads(rs, 6000), None if s == 0 else A.heavy_grads(rs, 5000)] for s in range(3)]
    kw = dict(betas=BETAS, eps=EPS, wd=WD)
    return dict(params=params, steps=steps, kw=kw, r64=A.replay(params, steps, LRS, dtype=np.float64, **kw),
                r32=A.torch_replay(params, steps, LRS, **kw))


def violations(case, y, verbose=False):
    """per (tensor, quantity): the strata's violations"""
    out = {}
    for i in range(2):
        for q, what in enumerate(("p", "exp_avg", "exp_avg_sq")):
            out[(i, what)] = A.strata_check(f"t{i} {what}", y[q][i], case["r64"][q][i], case["r32"][q][i], case["steps"][-1][i], verbose)
    return out


def test_float32_replay_is_inside_the_bar(case):
    y = A.replay(case["params"], case["steps"], LRS, dtype=np.float32, **case["kw"])
    assert y[3] == case["r32"][3] == [3, 2]
    bad = violations(case, y, verbose=True)
    assert not any(bad.values()), bad


# the one quantity each defect must move beyond the bar: (tensor, quantity)
CAUGHT_BY = {"coupled_decay": (0, "exp_avg"), "float_one_minus_beta2": (0, "exp_avg_sq"), "shared_step": (1, "p"),
             "eps_inside_sqrt": (0, "p")}


@pytest.mark.parametrize("defect", A.DEFECTS)
def test_seeded_defect_is_caught(case, defect):
    y = A.replay(case["params"], case["steps"], LRS, dtype=np.float32, defect=defect, **case["kw"])
    bad = violations(case, y)
    assert bad[CAUGHT_BY[defect]], (defect, {k: v for k, v in bad.items() if v})
    if defect == "shared_step":  # the tensor that stepped every time has t = the shared count: untouched by this defect
        assert not any(bad[(0, w)] for w in ("p", "exp_avg", "exp_avg_sq"))
