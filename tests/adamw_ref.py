"""Shared by the tests of dissc_amd.nn.AdamW (not a test module): torch.optim.AdamW's non-capturable single-tensor update
(amsgrad False, maximize False, decoupled decay) replayed in numpy, in float64 and in float32 (every scalar formed in double and
rounded once, every product and sum rounded on its own -- the arithmetic of csrc/adamw.hip), with the seeded defects a CPU test
must catch; the heavy-tailed gradients of the tests; the three-strata comparison against float32 torch as the yardstick."""
import numpy as np
import torch

import conv_grad_ref as CG

DEFECTS = ("coupled_decay", "float_one_minus_beta2", "shared_step", "eps_inside_sqrt")
STRATA = (("|g| < 1e-8", 0.0, 1e-8), ("1e-8 <= |g| < 1e-2", 1e-8, 1e-2), ("|g| >= 1e-2", 1e-2, np.inf))
BAR = 4.0


def heavy_grads(rs, n):
    """Student-t (3 degrees of freedom) times 10^U(-12, 2), one tenth exact zeros"""
    g = rs.standard_t(3, n) * 10.0 ** rs.uniform(-12, 2, n)
    g[rs.uniform(size=n) < 0.1] = 0.0
    return g.astype(np.float32)


def replay(params, grad_steps, lrs, betas=(0.9, 0.999), eps=1e-8, wd=1e-2, dtype=np.float64, defect=None):
    """params: list of float32 arrays; grad_steps[s][i]: tensor i's grad at step s or None (the tensor is skipped: no state, its
    step count does not advance); lrs[s]: the learning rate of step s.  -> (p, m, v, t) lists; m / v of a never-stepped tensor None."""
    assert defect is None or defect in DEFECTS
    f = dtype
    b1, b2 = betas
    p = [x.astype(f) for x in params]
    m, v, t = [None] * len(p), [None] * len(p), [0] * len(p)
    for s, grads in enumerate(grad_steps):
        lr = float(lrs[s])
        for i, g in enumerate(grads):
            if g is None:
                continue
            if m[i] is None:
                m[i], v[i] = np.zeros_like(p[i]), np.zeros_like(p[i])
            t[i] += 1
            ti = s + 1 if defect == "shared_step" else t[i]
            g = g.astype(f)
            omb2 = f(np.float32(1.0) - np.float32(b2)) if defect == "float_one_minus_beta2" else f(1.0 - b2)
            if defect == "coupled_decay":
                g = g + f(wd) * p[i]
            else:
                p[i] = p[i] * f(1.0 - lr * wd)
            m[i] = m[i] + (g - m[i]) * f(1.0 - b1)
            v[i] = v[i] * f(b2) + (omb2 * g) * g
            if defect == "eps_inside_sqrt":
                denom = np.sqrt(v[i] + f(eps)) / f(np.sqrt(1.0 - b2 ** ti))
            else:
                denom = np.sqrt(v[i]) / f(np.sqrt(1.0 - b2 ** ti)) + f(eps)
            p[i] = p[i] - f(lr / (1.0 - b1 ** ti)) * (m[i] / denom)
    return p, m, v, t


def torch_replay(params, grad_steps, lrs, betas=(0.9, 0.999), eps=1e-8, wd=1e-2):
    """float32 torch.optim.AdamW(foreach=False) on the CPU, the yardstick -> (p, m, v, t), numpy"""
    ps = [torch.nn.Parameter(torch.from_numpy(x.copy())) for x in params]
    opt = torch.optim.AdamW(ps, lr=lrs[0], betas=betas, eps=eps, weight_decay=wd, foreach=False)
    for s, grads in enumerate(grad_steps):
        opt.param_groups[0]["lr"] = float(lrs[s])
        for q, g in zip(ps, grads):
            q.grad = None if g is None else torch.from_numpy(g.copy())
        opt.step()
    st = [opt.state.get(q, None) for q in ps]
    return ([q.detach().numpy() for q in ps], [None if s is None else s["exp_avg"].numpy() for s in st],
            [None if s is None else s["exp_avg_sq"].numpy() for s in st], [0 if s is None else int(s["step"]) for s in st])


def strata_check(tag, y, r64, r32, g_last, verbose=True):
    """one tensor against the float64 replay with float32 torch as the yardstick (conv_grad_ref.check, kind "vec", bar 4), on the
    elements of each stratum of the LAST gradient's magnitude separately, so that the rms of large elements cannot hide small
    ones -> the list of violations"""
    bad = []
    a = np.abs(g_last.reshape(-1).astype(np.float64))
    T = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x).reshape(-1)))
    for name, lo, hi in STRATA:
        sel = (a >= lo) & (a < hi)
        if sel.any():
            bad += CG.check(f"{tag} {name}", "vec", T(y)[sel], T(r64)[sel], T(r32)[sel], k_whole=BAR, k_ch=BAR, verbose=verbose)
    return bad
