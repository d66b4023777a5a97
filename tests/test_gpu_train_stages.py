"""Every kernel of the training engine (dissc_amd/csrc/train.hip, and conv_mfma32_kernel as the trainer uses it) against
float64, stage by stage, at real batch sizes.

One optimisation step is taken on the GPU; every buffer it wrote is read back (Trainer.tap / grads / state_dict /
adam_state); then each stage of oracle/train_stages_ref.py is evaluated on the ENGINE's inputs to that stage, in float64
(R64, the reference) and in fp32 on the CPU (R32, the yardstick).  Per stage output: e_gpu = rms(Y - R64) <=
K * max(rms(R32 - R64), 2^-24 rms(R64)), over the whole tensor and per channel / weight row; K and the measured ratios
are in tests/train_stage_cases.py and profiles/train_stage_error.md.  No upstream rounding and no LeakyReLU branch
decision enters a comparison (the reference applies the engine's rule to the engine's own activation), so nothing is
excluded except the capped sign-of-d positions of the pitch loss (train_stage_cases.pitch_skip).

tests/test_train_stages_cpu.py pins the stage functions to float64 autograd and shows that these bars catch a dropped
column, a missing partial, unflipped taps, n for n - 1, an overwritten second consumer and a wrong LeakyReLU branch."""
import time

import numpy as np
import pytest
import torch

from oracle import train_ref as TR
from oracle import train_stages_ref as S
from train_cases import BN_FED_BIASES, _flip_tolerant
import train_stage_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _new_trainer(kind, sd):
    from dissc_amd.train import Trainer
    return Trainer(kind, sd, C.LR, norm=C.NORM, stats=C.pitch_stats()).to("cuda:0")


def _step(tr, batch):
    return float(tr.step(batch["seq"], batch["spk"], batch["tgt"], keep=batch["keep"], pe_mult=batch["pe_mult"]))


def _trained(kind, harsh=False):
    """freshly initialised weights advanced by three engine steps (BatchNorm affine parameters, running statistics
    and Adam moments off their initial values; the packed conv weights rebuilt on the device three times); harsh: then
    the scaled weights / wide-range BatchNorm affine of train_stage_cases.harshen and one more step"""
    from dissc_amd.train import init_state_dict
    tr = _new_trainer(kind, init_state_dict(kind, 100, 108, seed=1))
    for i in range(3):
        _step(tr, C.make_batch(kind, 4, 40, seed=900 + i))
    if harsh:
        tr = _new_trainer(kind, C.harshen(kind, tr.state_dict()))
        _step(tr, C.make_batch(kind, 4, 40, seed=903))
    return tr


def _engine_step(tr, kind, batch):
    """one step; returns (state before, Adam state before, every buffer the step wrote)"""
    pre = tr.state_dict()
    m, v, n = tr.adam_state()
    Y = {"loss": torch.tensor(_step(tr, batch), dtype=torch.float64)}
    Y["x0"], Y["dx0"] = tr.tap("x0"), tr.tap("dx0")
    for l in S.layers(kind):
        name = l["conv"]
        for which in ("z", "dz") + (("a", "da") if l["cout"] > 1 else ()) + (("mean", "invstd") if l["bn"] else ()):
            Y[f"{name}/{which}"] = tr.tap(name, which)
    for k, g in tr.grads().items():
        Y["grad/" + k] = g
    m1, v1, n1 = tr.adam_state()
    assert n1 == n + 1
    post = tr.state_dict()
    for k in m1:
        Y["after/" + k], Y["m/" + k], Y["v/" + k] = post[k], m1[k], v1[k]
    for k in post:
        if k.endswith(("running_mean", "running_var")):
            Y["after/" + k] = post[k]
    return pre, dict(m=m, v=v, step=n), Y


def _check_stages(kind, tr, batch, tag):
    hp = C.hyper(kind)
    pre, opt, Y = _engine_step(tr, kind, batch)
    R64, aux = S.run(kind, pre, opt, batch, hp, torch.float64, taps=Y)
    R32, _ = S.run(kind, pre, opt, batch, hp, torch.float32, taps=Y)
    bad, _ = C.check_step(kind, Y, R64, R32, aux, tag)
    for key, y in Y.items():
        assert torch.isfinite(y).all(), key
    # the embedding is products by 0 / 1 / 1/(1-p) and one addition: exact
    assert torch.equal(Y["x0"], R32["x0"])
    # padding rows of the embeddings have no gradient and never move
    assert not Y["grad/token_emb.weight"][100].any() and torch.equal(Y["after/token_emb.weight"][100], pre["token_emb.weight"][100])
    if kind != "len":
        assert not Y["grad/spk_emb.weight"][108].any()
    assert not bad, bad
    return pre, Y


# ---------------------------------------------------------------------------------------------------------
# the three full-size batches
# ---------------------------------------------------------------------------------------------------------
LARGE = {"len": (32, 333), "new": (32, 850), "base": (13, 601)}


@pytest.mark.parametrize("harsh", [False, True], ids=["trained", "harsh"])
@pytest.mark.parametrize("kind", ["len", "new", "base"])
def test_stages_at_full_size(kind, harsh):
    """len 32 x 333: L > 256, L % 4 = 1, wgrad halves of three chunks with a 13-column last chunk, padding inside groups
    of four; new 32 x 850: the positional encoding's limit, four trips of the strided loops, pe_mult, k = 1 heads,
    two-consumer da; base 13 x 601: BatchNorm on the head branches, 26 weight-gradient partials = 3 x 8 + 2"""
    B, L = LARGE[kind]
    t0 = time.time()
    _check_stages(kind, _trained(kind, harsh), C.make_batch(kind, B, L, seed=100), f"{kind} {B}x{L}{' harsh' if harsh else ''}")
    print(f"TS {kind} {B}x{L} took {time.time() - t0:.1f} s")


@pytest.mark.parametrize("kind", ["len", "new", "base"])
def test_whole_step_at_full_size(kind):
    """the existing whole-step style at the new shapes: loss and gradients against float64 autograd (bars of
    train_cases._flip_tolerant), the same step twice from the same state gives identical bits, state_dict layout"""
    B, L = LARGE[kind]
    batch, hp = C.make_batch(kind, B, L, seed=100), C.hyper(kind)
    outs = []
    for rep in range(2):
        tr = _trained(kind)
        pre = tr.state_dict()
        outs.append((_step(tr, batch), tr.grads(), tr.state_dict(), tr.adam_state()))
    assert outs[0][0] == outs[1][0]
    for k in outs[0][1]:
        assert torch.equal(outs[0][1][k], outs[1][1][k]), k
        assert torch.equal(outs[0][3][0][k], outs[1][3][0][k]) and torch.equal(outs[0][3][1][k], outs[1][3][1][k]), k
    for k in outs[0][2]:
        assert torch.equal(outs[0][2][k], outs[1][2][k]), k
    from dissc_amd.train import init_state_dict
    sd = outs[0][2]
    assert list(sd) == list(init_state_dict(kind, 100, 108, seed=1))
    nbt = [k for k in sd if k.endswith("num_batches_tracked")]
    assert nbt and all(int(sd[k]) == 4 for k in nbt)
    sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in pre.items()}
    pm = batch["pe_mult"].double() if batch["pe_mult"] is not None else None
    want_loss, want = TR.train_step(kind, sd64, batch["seq"], batch["spk"], batch["tgt"].double(), batch["keep"].double(),
                                    hp["lr"], {}, norm=hp["norm"], stats=tuple(s.double() for s in hp["stats"]), pe_mult=pm,
                                    pad_value=hp["pad"])
    assert abs(outs[0][0] - float(want_loss)) <= 5e-5 * float(want_loss), (outs[0][0], float(want_loss))
    for k, g in outs[0][1].items():
        if k in BN_FED_BIASES[kind]:
            continue
        _flip_tolerant(g.numpy(), want[k].numpy(), k)
    for k in sd64:  # running statistics after the step
        if k.endswith(("running_mean", "running_var")):
            np.testing.assert_allclose(sd[k].double().numpy(), sd64[k].numpy(), rtol=1e-4, atol=1e-5, err_msg=k)


# ---------------------------------------------------------------------------------------------------------
# boundaries of the 64-column chunks, the two time halves and the 128-column launch grids; the poisoned workspace
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [64, 65, 127, 128, 129, 257])
@pytest.mark.parametrize("kind", ["len", "new", "base"])
def test_stages_at_chunk_boundaries(kind, L):
    tr = _trained(kind)
    batch = C.make_batch(kind, 3, L, seed=200 + L)
    pre, Y = _check_stages(kind, tr, batch, f"{kind} 3x{L}")
    if L % 4 == 0:
        return
    # the same step with the workspace pre-filled with 0xFF bytes (NaN): nothing may read row padding (L .. ld - 1) or
    # a buffer before it is written -- loss, gradients and state bit-identical and finite
    from dissc_amd._lib import lib
    tp = _trained(kind)
    need = lib.dissc_train_workspace_bytes(tp._h, 3, L)
    tp._ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda:0")
    assert torch.isnan(tp._ws[: need // 4 * 4].view(torch.float32)).all()
    loss = _step(tp, batch)
    assert tp._ws.numel() == need
    assert np.isfinite(loss) and loss == float(Y["loss"]), (loss, float(Y["loss"]))
    for k, g in tp.grads().items():
        assert torch.isfinite(g).all() and torch.equal(g, Y["grad/" + k]), k
    post, (m, v, _) = tp.state_dict(), tp.adam_state()
    for k in m:
        assert torch.equal(post[k], Y["after/" + k]) and torch.equal(m[k], Y["m/" + k]) and torch.equal(v[k], Y["v/" + k]), k
    for k in post:
        if k.endswith(("running_mean", "running_var")):
            assert torch.equal(post[k], Y["after/" + k]), k


@pytest.mark.parametrize("L", [1, 2, 5])
@pytest.mark.parametrize("kind", ["len", "new", "base"])
def test_stages_at_tiny_shapes(kind, L):
    """B = 1: L = 1 is the n - 1 guard of the running variance (n = 1) and a single column; L < 4 has no complete
    group of four in the length loss"""
    _check_stages(kind, _trained(kind), C.make_batch(kind, 1, L, seed=300 + L), f"{kind} 1x{L}")


# ---------------------------------------------------------------------------------------------------------
# the API around the step
# ---------------------------------------------------------------------------------------------------------
def test_a_batch_longer_than_the_positional_encoding_is_refused():
    from dissc_amd._lib import DisscError, lib
    tr = _trained("new")
    before, steps = tr.state_dict(), int(lib.dissc_train_steps(tr._h))
    m0, v0, _ = tr.adam_state()
    with pytest.raises(DisscError, match=r"851 frames exceed the positional encoding \(850\)") as e:
        _step(tr, C.make_batch("new", 2, 851, seed=1))
    assert "(-1)" in str(e.value)  # DISSC_EINVAL
    assert int(lib.dissc_train_steps(tr._h)) == steps
    after = tr.state_dict()
    m1, v1, _ = tr.adam_state()
    for k in before:
        assert torch.equal(before[k], after[k]), k
    for k in m0:
        assert torch.equal(m0[k], m1[k]) and torch.equal(v0[k], v1[k]), k
    _step(tr, C.make_batch("new", 2, 850, seed=1))  # and the limit itself is accepted
    assert int(lib.dissc_train_steps(tr._h)) == steps + 1


def test_two_live_trainers_return_their_own_taps():
    """x0 / dx0 used to live in two process-wide statics: with two trainers alive, the taps of the one that stepped
    first were the other's buffers"""
    from dissc_amd._lib import DisscError
    a, b = _trained("len"), _trained("new")
    ba, bb = C.make_batch("len", 3, 70, seed=1), C.make_batch("new", 2, 45, seed=2)
    _step(a, ba)
    _step(b, bb)
    before = {"len": a.state_dict(), "new": b.state_dict()}
    _step(a, ba)
    _step(b, bb)
    for tr, kind, batch in ((a, "len", ba), (b, "new", bb)):
        sd = before[kind]
        x0 = S.embed(batch["seq"], batch["spk"].reshape(-1), batch["keep"], batch["pe_mult"], sd["token_emb.weight"],
                     sd["spk_emb.weight"], sd["pe.pe"] if kind == "new" else None)
        assert torch.equal(tr.tap("x0"), x0), kind
        assert tr.tap("dx0").shape == x0.shape and torch.isfinite(tr.tap("dx0")).all()
    assert a.layers()[-1] == "cnn2" and b.layers()[-2:] == ["cnn_class2", "cnn_reg2"]
    assert a.tap("cnn2", "z").shape == (3, 70) and b.tap("cnn_reg2", "dz").shape == (2, 45)
    assert b.tap("cnn2", "invstd").shape == (128,)
    with pytest.raises(DisscError):  # no BatchNorm on that layer
        b.tap("cnn1", "mean")
    with pytest.raises(DisscError):  # a scalar head has no separate activation
        a.tap("cnn2", "a")
