"""tests/predictor_cases.py without a GPU: the restatement is the pinned oracle's (bit for bit on the inputs of
tests/golden/pred.npz), its float64 side is finite on every case of tests/test_gpu_predictors_tiles.py, torch's fp32 evaluation
alone stays inside the excluded-frame cap, the derived pitch dicts do what their names say, and the bars see the defects they
exist for: each seeded defect, applied to the float32 restatement, misses bar (c) with K at its cap."""
import os

import numpy as np
import pytest
import torch

import predictor_cases as C
from oracle import predictors_ref as pr

PITCH = [k for k in C.KINDS if k != "len"]


def test_float32_restatement_is_the_pinned_oracle_bit_for_bit(golden_dir):
    g = np.load(os.path.join(golden_dir, "pred.npz"))
    id2m, id2s = torch.from_numpy(g["id2pitch_mean"]), torch.from_numpy(g["id2pitch_std"])
    sds = {kind: C.state_dict(kind, "iid") for kind in C.KINDS}
    for i in range(int(g["n_seqs"])):
        spk = int(g[f"spk{i}"])
        dd = torch.from_numpy(g[f"dd_vals{i}"]).view(1, -1)
        want = pr.len_predictor(sds["len"], dd, torch.tensor([[spk]]), *C.LEN_NORM)
        got = C.forward("len", sds["len"], dd[0], spk)["lens"]
        assert got.dtype == torch.float32 and torch.equal(got, want[0]), ("len", i)
        np.testing.assert_array_equal(want.numpy(), g[f"lens{i}"])  # (the oracle is still the golden file's)
        ex = torch.from_numpy(g[f"expanded{i}"])
        for kind in PITCH:
            for norm in (True, False):
                want = pr.pitch_predictor(sds[kind], ex, torch.tensor([[spk]]), kind, norm, id2m, id2s)
                got = C.forward(kind, sds[kind], ex[0], spk, norm=norm, stats=(id2m, id2s))
                assert torch.equal(got["out"], want[0]), (kind, norm, i)
                assert torch.equal(got["out"], (got["cls"] > 0) * got["reg"])


def test_rows_and_masks():
    for kind in C.KINDS:
        lengths, seqs, spk = C.rows(kind)
        assert lengths == C.EDGE + ([850] if kind != "len" else []) and [len(s) for s in seqs] == lengths
        assert len(set(spk)) == len(spk) and max(spk) < C.N_SPEAKERS - 1
        seq, s, n = C.batch(seqs, spk, range(len(lengths)))
        for b, k in enumerate(lengths):
            assert (seq[b, k:] == C.NEVER_READ).all() and bool((seq[b, :k] < C.N_TOKENS).all())
        idx = C.big_batch_index(kind)
        assert len(idx) == 70 and lengths[idx[64]] == 0 and lengths[idx[63]] > 0 and lengths[idx[65]] > 0
        assert max(lengths[i] for i in idx) == 513 and all(idx.count(i) >= 2 for i in set(idx))
        mid = C.mid_batch_index(kind)
        assert (len(mid), max(lengths[i] for i in mid)) == ((40, 513) if kind == "len" else (20, 385))
    if_dedupd = C.rows("len")[1][-1]
    assert (if_dedupd[1:] != if_dedupd[:-1]).all()
    m = C.edge_mask([513, 5, 0, 100], 513)
    want = [t for t in range(513) if t % 64 < 12 or t % 64 >= 52 or t >= 501]
    assert np.flatnonzero(m[0]).tolist() == want and m[0, :12].all() and not m[0, 12:52].any() and m[0, 501:].all()
    assert m[1, :5].all() and not m[1, 5:].any() and not m[2].any()
    assert np.flatnonzero(m[3]).tolist() == list(range(12)) + list(range(52, 76)) + list(range(88, 100))


@pytest.mark.parametrize("weights", C.WEIGHTS)
@pytest.mark.parametrize("kind", C.KINDS)
def test_float64_is_finite_and_torch_fp32_alone_is_inside_the_cap(kind, weights):
    """every (kind, weight set, case) of the GPU file: the float64 outputs are finite and O(1 - 100), and torch's own fp32
    evaluation, held to the decision rule, excludes at most 0.2 % of the frames and meets the bars against itself"""
    lengths, _, _ = C.rows(kind)
    cases = [("natural", "lens", False)] if kind == "len" else [("natural", "out", True), ("natural", "out_hz", True),
                                                                 ("reg_exposed", "out", False), ("cls_exposed", "out", False)]
    for exposed, key, natural in cases:
        for second in ((False, True) if kind == "len" else (False,)):
            ref = C.reference(kind, weights, exposed, second)
            got = np.zeros((len(lengths), max(lengths)))
            for b, r in enumerate(ref):
                assert (r is None) == (lengths[b] == 0)
                if r is not None:
                    for p in r:
                        for name, v in p.items():
                            assert v.shape == (lengths[b],) and np.isfinite(v).all(), (exposed, name, b)
                    assert np.abs(r[0][key]).max() < 500 and (kind == "len" or np.abs(r[0]["cls"]).max() < 100)
                    got[b, :lengths[b]] = r[1][key]
            m = C.measure(got, ref, key, lengths, natural_pitch=natural)
            print(C.line(f"torch fp32 {kind} {weights} {exposed} {key}", m))
            assert m["valid"] == sum(lengths) and m["excluded"] <= C.EXCLUDED_CAP * m["valid"], m
            assert m["flips_outside"] == 0 and not C.violations(m), m
            assert max(m["a"], m["b"], m["c"]) <= 1.0 and m["e_cpu"] > 0, m


@pytest.mark.parametrize("weights", C.WEIGHTS)
@pytest.mark.parametrize("kind", PITCH)
def test_exposed_dicts_do_what_their_names_say(kind, weights):
    nat = C.reference(kind, weights)
    reg = C.reference(kind, weights, "reg_exposed")
    cls = C.reference(kind, weights, "cls_exposed")
    for b, n in enumerate(C.rows(kind)[0]):
        if n == 0:
            continue
        for d in (0, 1):  # float64 and float32
            assert (reg[b][d]["cls"] == 1.0).all() and np.array_equal(reg[b][d]["out"], reg[b][d]["reg"])
            assert np.array_equal(reg[b][d]["reg"], nat[b][d]["reg"])  # the regression of the natural dict, at every frame
            assert np.array_equal(cls[b][d]["cls"], nat[b][d]["cls"]) and np.array_equal(cls[b][d]["reg"], cls[b][d]["cls"])
            assert np.array_equal(cls[b][d]["out"], np.maximum(nat[b][d]["cls"], 0.0))
    assert any((r[0]["cls"] > 0).any() and (r[0]["cls"] < 0).any() for r in nat if r is not None)  # both decisions occur


# ---- the seeded defects ---------------------------------------------------------------------------------------------------
LAYER = "cnn13"  # the 128-row layer the conv defects sit in
AFFINE = {"len": "bn13", "new": "bn2", "base": "bn13"}  # the per-row affine defect 2 misplaces ("new" has one BatchNorm)


def _drop_right_halo_tap(kind, sd):
    """1. columns 63 / 127 / 255 of one layer lose the tap that reads the next tile's first column"""
    def hook(name, x, y):
        if name == LAYER:
            w = sd[name + ".weight"].to(x.dtype)
            for t in (63, 127, 255):
                if t + 1 < x.shape[-1]:
                    y[0, :, t] -= w[:, :, 2] @ x[0, :, t + 1]
        return y
    return dict(hook=hook)


def _affine_of_row_r_on_row_r_plus_32(kind, sd):
    """2. rows 32..63 of one layer take scale / shift of rows 0..31"""
    sd = {k: v.clone() for k, v in sd.items()}
    for part in ("weight", "bias", "running_mean", "running_var"):
        sd[f"{AFFINE[kind]}.{part}"][32:64] = sd[f"{AFFINE[kind]}.{part}"][0:32]
    return dict(sd=sd)


def _no_affine_on_the_head(kind, sd):
    """3. the head's affine is skipped: the length head's * std + mean, bn_c1 / bn_r1 of "base"; the head of "new" has none, so
    its one BatchNorm (bn2, the layer before) stands in"""
    return {"len": dict(skip_len_norm=True), "base": dict(skip_bn=("bn_c1", "bn_r1")), "new": dict(skip_bn=("bn2",))}[kind]


def _one_unmasked_column(kind, sd):
    """4. one layer reads the column beyond a row's length, where the workspace holds a stale 1.0 instead of the padding's 0"""
    def hook(name, x, y):
        if name == LAYER:
            w = sd[name + ".weight"].to(x.dtype)
            y[0, :, -1] += w[:, :, 2] @ torch.ones(x.shape[1], dtype=x.dtype)
        return y
    return dict(hook=hook)


DEFECTS = {"halo_tap": _drop_right_halo_tap, "affine_row": _affine_of_row_r_on_row_r_plus_32, "head_affine": _no_affine_on_the_head,
           "unmasked_column": _one_unmasked_column}
# every defect misses bar (c) at the cap K_CAP = 19 by at least this factor.  The iid weights are the sensitive set: torch's own
# fp32 error on the trained-like ones, which sets the bar, is up to 10 x larger (dead channels: x * 316 gamma - mean * 316 gamma)
MISS = {"iid": 1000.0, "trained_like": 50.0}


@pytest.mark.parametrize("weights", C.WEIGHTS)
@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("defect", list(DEFECTS))
def test_bars_see_the_seeded_defect(defect, kind, weights):
    """the float32 restatement with one defect, held like the kernel's output: bar (c) fails with K at its cap, by a factor of
    at least MISS[weights].  Smallest factors measured (ratio (c) / 19) over the kinds, iid / trained-like: halo_tap 6.2e3 / 2.0e3,
    affine_row 1.6e4 / 2.4e5, head_affine 5.1e4 / 1.3e4, unmasked_column 3.8e3 / 1.4e2 (a stale 1.0 in one column of one layer of
    "new", whose trunk runs at 900 x that magnitude)."""
    lengths, seqs, spk = C.rows(kind)
    sd = C.state_dict(kind, weights)
    kw = DEFECTS[defect](kind, sd)
    sd = kw.pop("sd", sd)
    ref = C.reference(kind, weights)
    key = "lens" if kind == "len" else "out"
    got = np.zeros((len(lengths), max(lengths)))
    for b, (s, k) in enumerate(zip(seqs, spk)):
        if len(s):
            got[b, :len(s)] = C.forward(kind, sd, s, k, **kw)[key].double().numpy()
    m = C.measure(got, ref, key, lengths, natural_pitch=kind != "len")
    factor = m["c"] / C.K_CAP
    print(f"defect {defect:16s} {kind:4s} {weights:12s} ratio (c) {m['c']:.3e} = {factor:.3e} x the cap; (a) {m['a']:.3e} (b) {m['b']:.3e}")
    assert any(v[0] == "bar (c)" for v in C.violations(m, (C.K_CAP,) * 3) if isinstance(v, tuple)), (defect, kind, weights, m)
    assert factor >= MISS[weights], (f"{defect} on {kind} / {weights} misses bar (c) at K = {C.K_CAP} by a factor of {factor:.3g} only "
                                     f"(want >= {MISS[weights]})")
