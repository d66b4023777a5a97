"""GanTrainer(..., precision="split_bf16") on the GPU at gen_train_ref.SMALL_CONFIG (its 32-channel stage and conv_pre run split,
its 16-channel stage and conv_post fp32; convs.4 / convs.6 of every discriminator split) with the 64-point mel of
tests/test_gpu_gan_train.py, 2 utterances of 40 frames (that file's segment at this config's hop of 8: 320 samples), one fixed
batch: one step bit for bit against the same lines written out with the three modules built at precision="split_bf16"; resume
across the modes in both directions (a checkpoint records no precision); the mel term falls, and the first step's losses next to
the fp32 trainer's from the same weights."""
import numpy as np
import pytest
import torch

import gan_train_cases as GC
import gen_train_ref as GT
import split_bf16_model as sm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = dict(GC.TRAIN_CONFIG, **GT.SMALL_CONFIG, segment_size=320, code_hop_size=8)
SPLIT = "split_bf16"


@pytest.fixture(scope="module")
def gt():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import gan_train
    return gan_train


def batch(seed):
    rs = np.random.RandomState(seed)
    F = H["segment_size"] // H["code_hop_size"]
    to = lambda a: torch.from_numpy(a).to(DEV)
    return {"y": to((0.5 * rs.uniform(-1, 1, (2, 1, H["segment_size"]))).astype(np.float32)),
            "code": to(rs.randint(0, H["num_embeddings"], (2, F)).astype(np.int64)),
            "f0": to(rs.uniform(-1, 1, (2, 1, F)).astype(np.float32)), "spkr": to(rs.randint(0, 200, (2, 1)).astype(np.int64))}


def everything(t):
    """every state tensor of a trainer on the host: the three modules under the reference's keys, both optimisers' flat states
    and scalars (as tests/test_gpu_gan_train.py takes them)"""
    torch.cuda.synchronize()
    out = {}
    for name, sd in (("g", t.generator.state_dict()), ("mpd", t.mpd.state_dict()), ("msd", t.msd.state_dict())):
        out.update({f"{name}/{k}": v for k, v in sd.items()})
    for name, opt in (("optim_g", t.optim_g), ("optim_d", t.optim_d)):
        for i, s in opt.state.items():
            out[f"{name}/{i}/exp_avg"], out[f"{name}/{i}/exp_avg_sq"] = s["exp_avg"].cpu(), s["exp_avg_sq"].cpu()
            out[f"{name}/{i}/step"] = torch.tensor(float(s["step"]))
        out[f"{name}/lr"] = torch.tensor(opt.lr, dtype=torch.float64)
    return out


def assert_same_bits(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = a[k].contiguous().reshape(-1), b[k].contiguous().reshape(-1)
        assert x.dtype == y.dtype and x.shape == y.shape, k
        bits = torch.int32 if x.dtype == torch.float32 else torch.int64
        assert torch.equal(x.view(bits), y.view(bits)), k


def test_one_split_step_equals_the_lines_written_out(gt):
    from dissc_amd import MelSpectrogram, nn
    t = gt.GanTrainer(H, DEV, precision=SPLIT).init(seed=1)
    assert (t.generator.precision, t.mpd.precision, t.msd.precision) == (SPLIT,) * 3
    rep = t.generator.precision_report()
    assert rep["conv_pre"][0] and rep["resblocks.0.convs1.0"] == (True, True, True) and rep["conv_post"] == (False, False, False)
    before = everything(t)
    b = batch(0)
    losses = t.step(b)
    got = everything(t)
    assert all(bool(torch.isfinite(v).all()) for v in losses.values())
    assert any(not torch.equal(before[k], got[k]) for k in before if k.startswith("g/"))
    sg, sp, ss = gt.init_state_dicts(H, 1)
    G, P, S = (nn.CodeGenerator(H, precision=SPLIT).to(DEV), nn.MultiPeriodDiscriminator(precision=SPLIT).to(DEV),
               nn.MultiScaleDiscriminator(precision=SPLIT).to(DEV))
    G.load_state_dict(sg), P.load_state_dict(sp), S.load_state_dict(ss)
    ms = MelSpectrogram.from_config(H, for_loss=True).to(DEV)
    og = nn.AdamW(G.parameters(), lr=H["learning_rate"], betas=(H["adam_b1"], H["adam_b2"]))
    od = nn.AdamW(S.parameters() + P.parameters(), lr=H["learning_rate"], betas=(H["adam_b1"], H["adam_b2"]))
    y = b["y"]
    y_hat = G(code=b["code"], f0=b["f0"], spkr=b["spkr"])
    od.zero_grad()
    loss_f = nn.discriminator_loss(P(y, y_hat.detach()))[0]
    loss_s = nn.discriminator_loss(S(y, y_hat.detach()))[0]
    (loss_s + loss_f).backward()
    od.step()
    og.zero_grad()
    loss_mel = ms.l1_loss(y, y_hat) * 45
    out_f, out_s = P(y, y_hat, param_grads=False), S(y, y_hat, param_grads=False)
    loss_g = nn.generator_loss(out_s)[0] + nn.generator_loss(out_f)[0] + nn.feature_loss(out_s) + nn.feature_loss(out_f) + loss_mel
    loss_g.backward()
    og.step()

    class Hand:
        generator, mpd, msd, optim_g, optim_d = G, P, S, og, od
    assert_same_bits(got, everything(Hand))
    assert torch.equal(losses["loss_gen_all"].cpu(), loss_g.detach().cpu()) and torch.equal(losses["loss_disc_all"].cpu(), (loss_s + loss_f).detach().cpu())
    # and the mode is not the default's: the same step in fp32 ends elsewhere
    f = gt.GanTrainer(H, DEV).init(seed=1)
    f.step(b)
    fp = everything(f)
    assert any(not torch.equal(fp[k], got[k]) for k in got if k.startswith("g/"))


@pytest.mark.parametrize("first, then", [(SPLIT, "fp32"), ("fp32", SPLIT)])
def test_resume_across_modes(gt, tmp_path, first, then):
    b = [batch(s) for s in (10, 11, 12)]
    a = gt.GanTrainer(H, DEV, precision=first).init(seed=2)
    for x in b[:2]:
        a.step(x)
    saved = everything(a)
    a.save(str(tmp_path), 2, 0)
    r1, r2 = gt.GanTrainer(H, DEV, precision=then), gt.GanTrainer(H, DEV, precision=then)
    assert r1.load(str(tmp_path)) == {"steps": 2, "epoch": 0} and r2.load(str(tmp_path)) == {"steps": 2, "epoch": 0}
    assert r1.precision == then and r1.generator.precision == then
    s1 = everything(r1)
    assert_same_bits(s1, everything(r2))
    assert_same_bits(s1, saved)  # nothing of the mode is in a checkpoint: the state is the writer's
    losses = r1.step(b[2])
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in losses.values()), {k: float(v) for k, v in losses.items()}
    assert all(bool(torch.isfinite(v).all()) for v in everything(r1).values())


# The worst relative model error of a split layer recorded by tests/test_conv_split_ref_cpu.py (its "model to float64" lines: gw of
# 33 -> 64 k 7, 4.648e-06 of the tensor's rms; the forward's are 2.4e-06 .. 2.6e-06).
WORST_LAYER_E_MODEL = 4.648e-06


def test_mel_term_falls_and_first_step_losses_are_the_fp32_trainers(gt):
    t = gt.GanTrainer(H, DEV, precision=SPLIT).init(seed=1)
    b = batch(0)
    first = {k: float(v) for k, v in t.step(b).items()}
    trace = [first["mel_error"]] + [float(t.step(b)["mel_error"]) for _ in range(10)]
    print("\nGSB mel term, split-bf16:", " ".join(f"{x:.4f}" for x in trace))
    assert np.isfinite(trace).all() and trace[10] < trace[0]
    f32 = {k: float(v) for k, v in gt.GanTrainer(H, DEV).init(seed=1).step(b).items()}
    # Derivation of the bar.  A first-step loss is a mean, over thousands of elements, of a function of the modules' forward
    # outputs with Lipschitz constant <= 1 in units of the loss's own scale (|.| of mel differences, squares of scores near their
    # targets, |.| of feature differences).  Replacing fp32 layers by split layers perturbs each layer's output by a relative rms
    # of that layer's model error e_model / rms, and the per-element perturbations have no common sign, so the mean moves by at
    # most the aligned worst case: the worst layer's e_model / rms relative to the loss, times sm.MODEL_FACTOR for the fp32
    # accumulation and the summation order, as sm.block_bar prices a chain.  (The losses behind optim_d.step() also see the
    # discriminators' first update, lr = 2e-4 times a split gradient: a perturbation of the same relative order of a term 2e-4
    # of the weights.)
    bar = sm.MODEL_FACTOR * WORST_LAYER_E_MODEL
    worst = 0.0
    for k in sorted(first):
        rel = abs(first[k] - f32[k]) / max(abs(f32[k]), 1e-30)
        worst = max(worst, rel)
        print(f"GSB first step {k:14s}: split {first[k]:.7f} fp32 {f32[k]:.7f} relative difference {rel:.3e} (bar {bar:.3e})")
    assert worst <= bar, (worst, bar)
