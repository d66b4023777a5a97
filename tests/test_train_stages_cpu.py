"""The stage-wise restatement of the training step (oracle/train_stages_ref.py) checked on the CPU:
  * chained in float64 into whole steps it equals autograd on oracle/train_ref.py (loss, every gradient, updated
    parameters, Adam moments, running statistics) to 1e-11 -- which is what makes the per-stage references of
    tests/test_gpu_train_stages.py trustworthy;
  * the bars of that file bite: an fp32 "kernel result" with one seeded defect fails its bar by >= 100x while the clean
    fp32 result passes;
  * the one capped exclusion (sign of d in the pitch loss) stays inside its cap at the shapes the GPU test runs."""
import numpy as np
import pytest
import torch

from oracle import train_ref as TR
from oracle import train_stages_ref as S
from dissc_amd.train import init_state_dict, layer_names
import train_stage_cases as C


def _rel(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm() / b.norm().clamp(min=1e-300))


def _f64(sd):
    return {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}


def test_layer_tables_agree():
    for kind in ("len", "new", "base"):
        assert [l["conv"] for l in S.layers(kind)] == layer_names(kind)
        sd = init_state_dict(kind, 100, 108, seed=0)
        assert set(S.trainable_keys(kind)) == set(TR.trainable_keys(sd))


@pytest.mark.parametrize("kind", ["len", "new", "base"])
def test_chained_stages_equal_autograd_in_float64(kind):
    """two consecutive steps (the second with non-zero Adam moments and moved running statistics), B = 4 ragged rows
    of up to 37 positions (L % 4 = 1: an incomplete last group of four)"""
    hp = C.hyper(kind)
    sd = _f64(init_state_dict(kind, 100, 108, seed=3))
    sd_ref = {k: v.clone() for k, v in sd.items()}
    keys = S.trainable_keys(kind)
    opt = dict(m={k: torch.zeros_like(sd[k]) for k in keys}, v={k: torch.zeros_like(sd[k]) for k in keys}, step=0)
    state = {}
    for step in range(2):
        batch = C.make_batch(kind, 4, 37, seed=20 + step)
        out, _ = S.run(kind, sd, opt, batch, hp, torch.float64)
        pm = batch["pe_mult"].double() if batch["pe_mult"] is not None else None
        loss, grads = TR.train_step(kind, sd_ref, batch["seq"], batch["spk"], batch["tgt"].double(), batch["keep"].double(),
                                    hp["lr"], state, norm=hp["norm"], stats=tuple(s.double() for s in hp["stats"]),
                                    pe_mult=pm, pad_value=hp["pad"])
        assert abs(float(out["loss"]) - float(loss)) <= 1e-11 * abs(float(loss))
        for k in keys:
            if k in BN_FED(kind):  # exactly zero in exact arithmetic: float64 noise on both sides, no relative bar
                wn = float(grads[k[:-4] + "weight"].norm())
                assert float((out["grad/" + k] - grads[k]).norm()) <= 1e-11 * wn, k
            else:
                assert _rel(out["grad/" + k], grads[k]) <= 1e-11, (k, _rel(out["grad/" + k], grads[k]))
                assert _rel(out["after/" + k], sd_ref[k]) <= 1e-11 and _rel(out["m/" + k], state["m"][k]) <= 1e-11, k
            # Adam normalises the gradient, so its state is compared from the reference's own gradient
            p, m, v = S.adam(sd[k], grads[k], opt["m"][k], opt["v"][k], step + 1, hp["lr"])
            assert _rel(p, sd_ref[k]) <= 1e-11 and _rel(m, state["m"][k]) <= 1e-11, k
            assert float((v - state["v"][k]).norm()) <= 1e-11 * float(state["v"][k].norm()) + 1e-300, k
        for k in sd_ref:
            if k.endswith(("running_mean", "running_var")):
                assert _rel(out["after/" + k], sd_ref[k]) <= 1e-11, k
        # padding rows: exactly zero gradient
        assert not out["grad/token_emb.weight"][100].any()
        if kind != "len":
            assert not out["grad/spk_emb.weight"][108].any()
        # carry the reference's state into the next step (identical up to 1e-11 by the assertions above)
        for k in keys:
            opt["m"][k], opt["v"][k] = state["m"][k].clone(), state["v"][k].clone()
        opt["step"] = step + 1
        sd = {k: v.clone() for k, v in sd_ref.items()}


def BN_FED(kind):
    from train_cases import BN_FED_BIASES
    return BN_FED_BIASES[kind]


# ---------------------------------------------------------------------------------------------------------
# the bars bite
# ---------------------------------------------------------------------------------------------------------
def _fp32_step(kind, B, L, seed):
    """a whole fp32 step on the CPU stands in for the engine: its stage outputs are the 'taps'"""
    hp = C.hyper(kind)
    sd = init_state_dict(kind, 100, 108, seed=seed)
    rs = np.random.RandomState(seed)
    for k in sd:  # not the initial statistics
        if k.endswith("running_var"):
            sd[k] = torch.from_numpy(rs.uniform(0.5, 2.0, sd[k].numel()).astype(np.float32))
    keys = S.trainable_keys(kind)
    opt = dict(m={k: 1e-3 * torch.randn_like(sd[k]) for k in keys}, v={k: 1e-6 * torch.rand_like(sd[k]) for k in keys}, step=3)
    batch = C.make_batch(kind, B, L, seed)
    Y, _ = S.run(kind, sd, opt, batch, hp, torch.float32)
    R64, aux = S.run(kind, sd, opt, batch, hp, torch.float64, taps=Y)
    R32, _ = S.run(kind, sd, opt, batch, hp, torch.float32, taps=Y)
    return sd, batch, Y, R64, R32, aux


def _fails_by(kind, Y, R64, R32, aux, key, value):
    """worst (ratio / bar) of ``key`` with its value replaced by the defective one; every other tensor untouched"""
    Yd = dict(Y)
    Yd[key] = value
    bad, _ = C.check_step(kind, Yd, R64, R32, aux, "defect", verbose=False)
    assert bad and all(b[1] == key for b in bad), bad
    return max(b[3] / b[4] for b in bad)


def test_seeded_defects_fail_their_bars_by_100x():
    kind, B, L = "new", 3, 129
    sd, batch, Y, R64, R32, aux = _fp32_step(kind, B, L, seed=5)
    bad, _ = C.check_step(kind, Y, R64, R32, aux, "clean fp32")
    assert not bad, bad
    dz, a_in, w = Y["cnn13/dz"], Y["cnn12/a"], sd["cnn13.weight"]
    ap = torch.nn.functional.pad(a_in, (1, 1))

    def partial(bs, t0, t1):  # the weight gradient's terms of rows bs, positions t0 .. t1 - 1
        return torch.stack([torch.einsum("bot,bit->oi", dz[bs, :, t0:t1], ap[bs, :, t0 + j:t1 + j]) for j in range(3)], -1)

    # 1. last column of a 64-chunk dropped in the weight gradient
    f = _fails_by(kind, Y, R64, R32, aux, "grad/cnn13.weight", Y["grad/cnn13.weight"] - partial(slice(None), 63, 64))
    print("defect: chunk's last column dropped  x", f)
    assert f >= 100
    # 2. one of the B x 2 partials (utterance 1, first time half: positions 0 .. 127) left out
    f = _fails_by(kind, Y, R64, R32, aux, "grad/cnn13.weight", Y["grad/cnn13.weight"] - partial(slice(1, 2), 0, 128))
    print("defect: one partial left out         x", f)
    assert f >= 100
    # 3. taps not flipped in backward-data
    unflipped = torch.nn.functional.conv1d(dz, w.transpose(0, 1).contiguous(), padding=1)
    f = _fails_by(kind, Y, R64, R32, aux, "cnn12/da", unflipped)
    print("defect: taps not flipped             x", f)
    assert f >= 100
    # 5. the second consumer's da overwrites instead of adding (cnn2 feeds cnn_reg1, then cnn_class1)
    f = _fails_by(kind, Y, R64, R32, aux, "cnn2/da", S.bwd_data(Y["cnn_class1/dz"], sd["cnn_class1.weight"]))
    print("defect: second consumer overwrites   x", f)
    assert f >= 100
    # 6. slope applied on a >= 0
    da, a = Y["cnn13/da"], Y["cnn13/a"]
    f = _fails_by(kind, Y, R64, R32, aux, "cnn13/dz", torch.where(a >= 0, da * S.SLOPE, da))
    print("defect: slope on the wrong branch    x", f)
    assert f >= 100
    # 4. n instead of n - 1 in the running variance (a model with BatchNorm in the trunk)
    kind = "len"
    sd, batch, Y, R64, R32, aux = _fp32_step(kind, B, L, seed=6)
    bad, _ = C.check_step(kind, Y, R64, R32, aux, "clean fp32")
    assert not bad, bad
    rv = S.bn_stats(Y["cnn13/z"], sd["bn13.running_mean"], sd["bn13.running_var"], unbiased_n=B * L)[3]
    f = _fails_by(kind, Y, R64, R32, aux, "after/bn13.running_var", rv)
    print("defect: n instead of n - 1           x", f)
    assert f >= 100


@pytest.mark.parametrize("kind,B,L", [("new", 32, 850), ("base", 13, 601)])
def test_pitch_sign_exclusion_stays_inside_its_cap(kind, B, L):
    """at the large shapes of the GPU test: the positions whose sign of d fp32 cannot decide number at most 0.2 % of
    the voiced ones and 50, and outside them the fp32 restatement takes float64's sign everywhere"""
    hp = C.hyper(kind)
    sd = init_state_dict(kind, 100, 108, seed=1)
    batch = C.make_batch(kind, B, L, seed=100)
    Y, aux32 = S.run(kind, sd, None, batch, hp, torch.float32, forward_only=True)
    _, aux64 = S.run(kind, sd, None, batch, hp, torch.float64, taps=Y, forward_only=True)
    skip, nv, cap = C.pitch_skip(aux64)
    assert nv > 0.3 * B * L / 2 and cap >= 1
    assert int(skip.sum()) <= cap, (int(skip.sum()), cap)
    differ = aux64["pitch/voiced"] & ~skip & (torch.sign(aux32["pitch/d"]).double() != torch.sign(aux64["pitch/d"]))
    assert int(differ.sum()) == 0, int(differ.sum())
