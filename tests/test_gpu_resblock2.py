"""ResBlock2 (HiFi-GAN V3-style configs, "resblock": "2") on the GPU: the inference generator against waveforms and block
outputs of the reference itself (tests/golden/gen_resblock2.npz, recipe make_resblock2_golden.py), the direct conv kernels at tap
spans in (60, 72] in both families at every stage width, nn.conv1d's gradients at span 72, and the trainable generator and the
GAN trainer on a small config with the three V3 blocks.  Measured figures: profiles/resblock2.md."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

import conv_grad_harness as H
import conv_grad_ref as R
import gen_train_ref as GT
import resblock2_cases as RB
import synthdata as synth
import tile_harness as TH
from generator_cases import NORTH_STAR_RMS, _rms
from tile_harness import lib  # noqa: F401  (the module fixture that builds the library)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_resblock2.npz")
# The regression guard of this config's exact-fp32 path (generator_cases.FP32_GUARD_RMS was calibrated on the ResBlock1 model and
# is not reused): below 10 x the largest rms measured over the golden cases on an MI355X (4.5e-7 at T = 99; profiles/resblock2.md
# has every case), the rule of test_fp32_guard_rejects_split_bf16 -- and below what split-bf16 delivers here (3.2e-6 .. 3.9e-6 from
# T = 7 on), so the guard tells the two apart.
RB2_GUARD_RMS = 3e-6


@pytest.fixture(scope="module")
def env(lib):
    import dissc_amd
    h = RB.vctk_config()
    sd = RB.state_dict(h, seed=0)
    g = dissc_amd.CodeGenerator(h).to(DEV)
    g.load_state_dict(sd)
    g.eval().remove_weight_norm()
    return dict(h=h, sd=sd, g=g, z=np.load(GOLDEN), dissc_amd=dissc_amd)


def _wave_bars(tag, y, ref, guard=RB2_GUARD_RMS):
    e, s = _rms(y - ref), _rms(ref)
    print(f"\nRB2 {tag}: rms err {e:.3e}, signal rms {s:.3f}, max err {float(np.abs(y - ref).max()):.3e}")
    assert e <= NORTH_STAR_RMS and e <= 1e-3 * s and e <= guard, (tag, e, s)


def _golden_inputs(T):
    code, f0, spkr, _ = synth.synth_generator_inputs(1, T, seed=100 + T)
    return torch.from_numpy(code), torch.from_numpy(f0), torch.from_numpy(spkr)


# ---- (a) the inference generator against the reference's own outputs -------------------------------------------------------------
@pytest.mark.parametrize("T", RB.GOLDEN_T)  # T = 1 / 2: 5 / 10 columns in the first stage, shorter than the (7; 3, 12) reach
def test_generator_matches_the_reference(env, T):
    code, f0, spkr = _golden_inputs(T)
    y = env["g"](code=code, f0=f0, spkr=spkr).cpu().numpy()
    ref = env["z"][f"T{T}/wav"]
    assert y.shape == ref.shape == (1, 1, 320 * T)
    _wave_bars(f"T {T}", y, ref)


def test_generator_ragged_batch_is_one_batch(env):
    code, f0, spkr, _ = synth.synth_generator_inputs(4, 40, seed=777)
    lengths = env["z"]["ragged/lengths"]
    assert list(lengths) == RB.RAGGED_LENGTHS
    for b, n in enumerate(lengths):  # poison beyond each length: ids and f0 of the padding are never read
        code[b, n:], f0[b, :, n:] = 99, 1e30
    y = env["g"](code=torch.from_numpy(code), f0=torch.from_numpy(f0), spkr=torch.from_numpy(spkr),
                 lengths=torch.from_numpy(lengths)).cpu().numpy()
    got, ref = [], []
    for b, n in enumerate(lengths):
        assert not y[b, :, 320 * n:].any(), ("not zero beyond the utterance", b)
        got.append(y[b, 0, :320 * n])
        ref.append(env["z"][f"ragged/wav{b}"].reshape(-1))
        _wave_bars(f"ragged utterance {b} ({n} frames)", got[-1], ref[-1])
    _wave_bars("ragged batch", np.concatenate(got), np.concatenate(ref))


def test_block_outputs_at_T7(env):
    """every block's output at T = 7: nn.resblock2 (the direct conv kernels with the residual epilogue, at all five stage widths
    and all three (k; d0, d1)) on the trainable generator's own stage inputs, against the reference's block outputs"""
    from dissc_amd import nn
    h, z = env["h"], env["z"]
    G = nn.CodeGenerator(h).to(DEV)
    G.load_state_dict(env["sd"])
    code, f0, spkr = _golden_inputs(7)
    taps = []
    with torch.no_grad():
        wav = G(code=code, f0=f0, spkr=spkr, taps=taps)
        _wave_bars("nn.CodeGenerator T 7", wav.cpu().numpy(), z["T7/wav"])
        assert len(taps) == len(RB.conv_input_rates(h))
        w = {k: v.to(DEV).contiguous() for k, v in RB.fold(env["sd"]).items()}
        nk, mul, at = len(RB.V3_BLOCKS), 1, 1
        for i, u in enumerate(h["upsample_rates"]):
            mul *= u
            n = 7 * mul
            for j, (k, dil) in enumerate(RB.V3_BLOCKS):
                x = taps[at + 1 + 2 * j]  # the block's first conv input = the stage's input
                assert j == 0 or torch.equal(x, taps[at + 1])
                pre = f"resblocks.{i * nk + j}."
                wts = {key[len(pre):]: t for key, t in w.items() if key.startswith(pre)}
                r = nn.resblock2(x, wts, k, dil, lengths=torch.tensor([n], dtype=torch.int32, device=DEV))
                _wave_bars(f"block {i * nk + j} (C {x.shape[1]}, k {k}, d {dil})", r.cpu().numpy()[:, :, RB.edge_cols(n)], z[f"T7/rb{i * nk + j}"])
            at += 1 + 2 * nk


def test_flops_are_the_hand_count(env):
    g, per = env["g"], RB.flops_per_frame(env["h"])
    assert g.flops(1) == per == g.flops_executed(1) and g.flops(99) == 99 * per  # two direct convs per block: executed = algorithmic


# ---- (b) the one-launch form gives the two-launch form's bits ---------------------------------------------------------------------
RB2_ALL = 63  # "rb2_fused": every (stage width, k) with an instance


def _generator_under(env, lib, **options):
    """a handle created under the options (it snapshots them); both narrow stages' six blocks in the form the mask gives"""
    with TH.options(lib, **options):
        forms = [_info(lib, C, k, d)[0] for C in (32, 16) for k, d in RB.V3_BLOCKS]
        g = env["dissc_amd"].CodeGenerator(env["h"]).to(DEV)
        g.load_state_dict(env["sd"])
        g.eval().remove_weight_norm().prepare()
    return g, forms


def _info(lib, C, k, d):
    form, tile = ctypes.c_int(-1), ctypes.c_int(-1)
    lib.check(lib.lib.dissc_resblock2_info(C, k, d[0], d[1], ctypes.byref(form), ctypes.byref(tile)), "dissc_resblock2_info")
    return form.value, tile.value


def test_one_launch_form_is_bit_identical_in_the_generator(env, lib):
    fused, forms1 = _generator_under(env, lib, rb2_fused=RB2_ALL)
    plain, forms0 = _generator_under(env, lib, rb2_fused=0)
    assert forms1 == [1] * 6 and forms0 == [0] * 6
    cases = [_golden_inputs(T) + (None,) for T in RB.GOLDEN_T]
    code, f0, spkr, _ = synth.synth_generator_inputs(4, 40, seed=777)
    cases.append((torch.from_numpy(code), torch.from_numpy(f0), torch.from_numpy(spkr), torch.tensor(RB.RAGGED_LENGTHS)))
    code, f0, spkr, lengths = synth.synth_generator_inputs(4, 61, seed=31, ragged=True)  # 19 520 columns in the last stage
    cases.append((torch.from_numpy(code), torch.from_numpy(f0), torch.from_numpy(spkr), torch.from_numpy(lengths)))
    for code, f0, spkr, lengths in cases:
        kw = {} if lengths is None else {"lengths": lengths}
        a, b = fused(code=code, f0=f0, spkr=spkr, **kw), plain(code=code, f0=f0, spkr=spkr, **kw)
        assert torch.equal(a, b) and bool(a.abs().sum() > 0), tuple(code.shape)


# ---- (c) dissc_resblock2_1d at tile edges ----------------------------------------------------------------------------------------
def _block(lib, mode, x, w1, b1, w2, b2, lengths, k, d, epi, acc0):
    B, C, ld = x.shape
    y = torch.full_like(x, TH.SENTINEL)
    acc = None if epi == 1 else acc0.clone()
    ln = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    lib.check(lib.lib.dissc_resblock2_1d(x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), y.data_ptr(),
                                         None if acc is None else acc.data_ptr(), ln.data_ptr(), B, C, k, d[0], d[1], ld, max(lengths),
                                         ctypes.c_float(TH.SLOPE), epi, ctypes.c_float(3.0), mode, None), "dissc_resblock2_1d")
    return y if epi == 1 else acc


@pytest.mark.parametrize("k,d", RB.V3_BLOCKS)
@pytest.mark.parametrize("C", [32, 16])
def test_one_launch_block_at_tile_edges(lib, C, k, d):
    with TH.options(lib, rb2_fused=RB2_ALL):
        form, W = _info(lib, C, k, d)
    p0, p1 = d[0] * (k - 1) // 2, d[1] * (k - 1) // 2
    assert form == 1 and W == 256 - 2 * p1
    lengths = [2 * W + 3, 1, p1, p0 + p1 + 1, W - 1, W, W + 1]  # the y1 halo, the full halo + 1, around the tile width
    B, ld = len(lengths), (max(lengths) + 3) // 4 * 4
    rs = np.random.RandomState(1000 * C + 10 * k + d[1])
    x = TH.make_x(rs, B, C, ld, lengths).to(DEV)  # NaN beyond every length
    w1, w2 = (torch.from_numpy((rs.standard_normal((C, C, k)) / np.sqrt(C * k)).astype(np.float32)) for _ in range(2))
    b1, b2 = (torch.from_numpy(rs.standard_normal(C).astype(np.float32)) for _ in range(2))  # non-zero: bias + conv(zeros) != 0
    beyond = TH.beyond_mask(lengths, ld).to(DEV)
    acc0 = torch.from_numpy(rs.standard_normal((B, C, ld)).astype(np.float32)).to(DEV)
    acc0 = torch.where(beyond.expand(B, C, ld), torch.full_like(acc0, TH.SENTINEL), acc0)  # the sentinel beyond every length
    # float64: reference64 composed twice, y1 zero beyond the length
    inside = (~beyond).double()
    r1 = (torch.nan_to_num(x.double()) + TH.reference64(x, w1, b1, lengths, k, d[0])) * inside
    r2 = r1 + TH.reference64(r1, w2, b2, lengths, k, d[1])
    with pytest.raises(lib.DisscError, match="no one-launch instance"):
        _block(lib, 1, x, w1, b1, w2, b2, lengths, k, (d[0] + 1, d[1]), 1, acc0)
    for epi in (1, 2, 3, 4):
        two = _block(lib, 0, x, w1, b1, w2, b2, lengths, k, d, epi, acc0)
        one = _block(lib, 1, x, w1, b1, w2, b2, lengths, k, d, epi, acc0)
        TH.check_edges(one, beyond, (C, k, d, epi, "one launch"))
        TH.check_edges(two, beyond, (C, k, d, epi, "two launches"))
        assert torch.equal(one, two), (C, k, d, epi, "the two forms differ")
        want = r2 if epi <= 2 else (acc0.double() + r2) / (3.0 if epi == 4 else 1.0)
        e = torch.where(beyond.expand_as(one), torch.zeros_like(want), one.double() - want)
        print(f"\nRB2 one launch C {C} k {k} d {d} epi {epi}: max err {float(e.abs().max()):.2e}, rms {float(e.pow(2).mean().sqrt()):.2e}, tile {W}")
        assert float(e.abs().max()) <= 2 * 2e-5  # test_conv1d_matches_torch's bar for one conv, doubled
    for i, n in enumerate(lengths):  # an utterance alone has the batch's bits
        alone = _block(lib, 1, x[i:i + 1].clone(), w1, b1, w2, b2, [n], k, d, 1, acc0)
        assert torch.equal(alone[0, :, :n], _block(lib, 1, x, w1, b1, w2, b2, lengths, k, d, 1, acc0)[i, :, :n]), (i, n)


# ---- (g) split-bf16 --------------------------------------------------------------------------------------------------------------
def test_split_bf16_within_the_acceptance_bar(env):
    g = env["dissc_amd"].CodeGenerator(env["h"], precision="split_bf16").to(DEV)
    g.load_state_dict(env["sd"])
    g.eval().remove_weight_norm()
    for T in RB.GOLDEN_T:
        code, f0, spkr = _golden_inputs(T)
        y = g(code=code, f0=f0, spkr=spkr).cpu().numpy()
        exact = env["g"](code=code, f0=f0, spkr=spkr).cpu().numpy()
        e = _rms(y - env["z"][f"T{T}/wav"])
        print(f"\nRB2 split-bf16 T {T}: rms err {e:.3e}")
        assert e <= NORTH_STAR_RMS, (T, e)
        assert T < 7 or not np.array_equal(y, exact), "the fp32 kernels ran"


# ---- (d) tap spans in (60, 72], both direct families, every stage width ----------------------------------------------------------
WIDE_TILE = 256  # the time tile of the wide-span instances
WIDE_LENGTHS = [2 * WIDE_TILE + 3, 1, 36, 37, WIDE_TILE - 1, WIDE_TILE, WIDE_TILE + 1]


@pytest.mark.parametrize("family", [32, 16])
@pytest.mark.parametrize("k,d", [(7, 12), (11, 7)])  # spans 72 and 70
@pytest.mark.parametrize("C", [16, 32, 64, 128, 256, 512])
def test_wide_span_conv(lib, family, C, k, d):
    """dissc_conv1d: test_conv1d_matches_torch's data and bar (2e-5 per element), against float64, NaN beyond every length and the
    sentinel behind it"""
    rs = np.random.RandomState(C * 100 + k * 10 + d)
    lengths = WIDE_LENGTHS
    B, ld = len(lengths), (max(lengths) + 3) // 4 * 4
    x = TH.make_x(rs, B, C, ld, lengths).to(DEV)
    w = torch.from_numpy((rs.standard_normal((C, C, k)) / np.sqrt(C * k)).astype(np.float32))
    b = torch.from_numpy(rs.standard_normal(C).astype(np.float32))
    beyond = TH.beyond_mask(lengths, ld).to(DEV)
    with TH.options(lib, mfma32=1 if family == 32 else 0):
        y = TH.run_conv(lib, x, w, b, lengths, k, d, TH.SLOPE)
        # every utterance alone: the bits of the batch
        for i in (1, 3, 5):
            one = TH.run_conv(lib, x[i:i + 1].clone(), w, b, [lengths[i]], k, d, TH.SLOPE)
            assert torch.equal(one[0, :, :lengths[i]], y[i, :, :lengths[i]]), ("alone", i)
    TH.check_edges(y, beyond, (family, C, k, d))
    r64 = TH.reference64(x, w, b, lengths, k, d)
    err = float(torch.where(beyond.expand_as(y), torch.zeros_like(r64), y.double() - r64).abs().max())
    print(f"\nRB2 wide span family {family} C {C} k {k} d {d}: max err {err:.2e}")
    assert err <= 2e-5, err


# One span-60 shape per family, bit for bit what the library built from the parent commit gave on an MI355X (sha256 of the
# float32 bytes of the valid columns, recorded in profiles/resblock2.md): spans <= 60 keep their instances.
SPAN60_DIGESTS = {32: "729b96e4b768e50f1dd74211655603bae6c38792b9ee644ee26dc599b598f449", 16: "52944acac6e46a55a01f784e2b75ee2af766d8f150ab55950a1db3ef6d11911b"}


def span60_digest(lib, family):
    C, k, d = (64, 11, 6) if family == 32 else (16, 11, 6)
    rs = np.random.RandomState(60 + family)
    lengths = [300, 1, 255, 257]
    x = TH.make_x(rs, len(lengths), C, 300, lengths).to(DEV)
    w = torch.from_numpy((rs.standard_normal((C, C, k)) / np.sqrt(C * k)).astype(np.float32))
    b = torch.from_numpy(rs.standard_normal(C).astype(np.float32))
    with TH.options(lib, mfma32=1 if family == 32 else 0):
        y = TH.held(TH.run_conv(lib, x, w, b, lengths, k, d, TH.SLOPE), TH.beyond_mask(lengths, 300).to(DEV))
    return hashlib.sha256(y.numpy().tobytes()).hexdigest()


@pytest.mark.parametrize("family", [32, 16])
def test_span_60_keeps_the_parents_bits(lib, family):
    assert span60_digest(lib, family) == SPAN60_DIGESTS[family]


# ---- (e) nn.conv1d at span 72 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [16, 32, 64])
def test_nn_conv1d_gradients_at_span_72(lib, C):
    from dissc_amd import nn
    spec = H.Spec("conv1d", C, C, 7, 12)
    lengths, ld, plan = H.lengths_for(nn, spec)
    print(f"\nRB2 layer {spec}: lengths {lengths}, ld {ld}, (P, pairs) {plan}")
    H.assert_layer_gradients(H.gpu_run(nn, spec), spec, lengths, ld, 7 * C + 19)


# ---- (f) the trainable generator and the trainer ---------------------------------------------------------------------------------
SMALL = RB.config(GT.SMALL_CONFIG)  # stage widths 32 and 16: the six (C; k; d0, d1) of the narrow stages


def _kind(key, t):
    return "weight" if t.dim() >= 2 and not key.endswith(".weight_g") else "vec"


def test_trainable_generator_forward_and_gradients(env):
    from dissc_amd import nn
    h, sd = SMALL, RB.state_dict(SMALL, seed=3)
    G = nn.CodeGenerator(h).to(DEV)
    G.load_state_dict(sd)
    B, T, lengths = 3, 13, [13, 7, 1]
    code, f0, spkr, _ = synth.synth_generator_inputs(B, T, seed=5, n_spk=200, n_codes=h["num_embeddings"])
    code, f0, spkr = torch.from_numpy(code), torch.from_numpy(f0), torch.from_numpy(spkr)
    gwav = torch.from_numpy(np.random.RandomState(6).randn(B, 1, 8 * T).astype(np.float32))
    taps = []
    wav = G(code=code, f0=f0, spkr=spkr, lengths=lengths, taps=taps)
    wav.backward(gwav.to(DEV))
    torch.cuda.synchronize()
    grads, wav = G.named_grads(), wav.detach().cpu()
    assert len(taps) == len(RB.conv_input_rates(h)) and list(grads) == list(G.named_leaves())
    # the inference class on the trainable class's state dict
    out = G.state_dict()
    assert list(out) != [] and set(out) == set(sd) and all(torch.equal(out[k], sd[k]) for k in sd)
    inf = env["dissc_amd"].CodeGenerator(h).to(DEV)
    inf.load_state_dict(out)
    y = inf(code=code, f0=f0, spkr=spkr, lengths=torch.tensor(lengths)).cpu()
    e = _rms((y - wav).numpy())
    print(f"\nRB2 inference twin vs trainable forward: rms {e:.3e}")
    assert e <= RB2_GUARD_RMS
    # every leaf against float64 on the engine's own branch decisions, at tests/test_gpu_gen_train.py's ratio bar (K = 4)
    masks = [t.detach().cpu() > 0 for t in taps]
    args = (sd, h, code, f0, spkr, lengths)
    w64, g64 = RB.generator_ref(*args, torch.float64, gwav=gwav, masks=masks)
    w32, g32 = RB.generator_ref(*args, torch.float32, gwav=gwav, masks=masks)
    assert set(grads) == set(sd) == set(g64)
    bad = R.check("rb2 wav", "act", wav, w64, w32)
    for key, t in grads.items():
        kind = _kind(key, t)
        flat = (lambda a: a.reshape(-1)) if kind == "vec" else (lambda a: a)
        bad += R.check(f"rb2 {key}", kind, flat(t.detach().cpu()), flat(g64[key]), flat(g32[key]))
    assert not bad, bad
    assert not wav[1, :, 8 * 7:].any() and not wav[2, :, 8:].any()  # nothing beyond the lengths


def _everything(t):
    torch.cuda.synchronize()
    out = {}
    for name, sd in (("g", t.generator.state_dict()), ("mpd", t.mpd.state_dict()), ("msd", t.msd.state_dict())):
        out.update({f"{name}/{k}": v for k, v in sd.items()})
    for name, opt in (("optim_g", t.optim_g), ("optim_d", t.optim_d)):
        for i, s in opt.state.items():
            out[f"{name}/{i}/exp_avg"], out[f"{name}/{i}/exp_avg_sq"] = s["exp_avg"].cpu(), s["exp_avg_sq"].cpu()
            out[f"{name}/{i}/step"] = torch.tensor(float(s["step"]))
    return out


def test_trainer_resumes_bit_for_bit(env, tmp_path):
    from dissc_amd import gan_train, nn
    h = dict(SMALL, segment_size=160, code_hop_size=8, sampling_rate=16000, n_fft=64, num_mels=20, hop_size=16, win_size=64, fmin=0,
             fmax=8000, fmax_for_loss=None, batch_size=2, learning_rate=2e-4, adam_b1=0.8, adam_b2=0.99, lr_decay=0.999, seed=1234,
             num_gpus=0, f0_normalize=True)

    def batch(seed):
        rs = np.random.RandomState(seed)
        F = h["segment_size"] // h["code_hop_size"]
        to = lambda a: torch.from_numpy(a).to(DEV)
        return {"y": to((0.5 * rs.uniform(-1, 1, (2, 1, h["segment_size"]))).astype(np.float32)),
                "code": to(rs.randint(0, h["num_embeddings"], (2, F)).astype(np.int64)),
                "f0": to(rs.uniform(-1, 1, (2, 1, F)).astype(np.float32)), "spkr": to(rs.randint(0, 200, (2, 1)).astype(np.int64))}

    # fresh weights under the reference's keys in its named_parameters() order
    sg = gan_train.init_state_dicts(h, 2)[0]
    order = list(nn.CodeGenerator(h).named_leaves())
    assert sorted(sg) == sorted(order) and [k for k in order if ".convs." in k][:3] == \
        ["resblocks.0.convs.0.bias", "resblocks.0.convs.0.weight_g", "resblocks.0.convs.0.weight_v"]
    b = [batch(s) for s in (10, 11, 12)]
    a = gan_train.GanTrainer(h, DEV).init(seed=2)
    for x in b[:2]:
        losses = a.step(x)
    assert all(bool(torch.isfinite(v).all()) for v in losses.values())
    g_path, _ = a.save(str(tmp_path), 2, 0)
    a.step(b[2])
    r = gan_train.GanTrainer(h, DEV)
    assert r.load(str(tmp_path)) == {"steps": 2, "epoch": 0}
    r.step(b[2])
    ea, er = _everything(a), _everything(r)
    assert sorted(ea) == sorted(er)
    for k in ea:
        assert ea[k].dtype == er[k].dtype and ea[k].contiguous().numpy().tobytes() == er[k].contiguous().numpy().tobytes(), k
    # the saved g_* loads into the inference class and runs
    sd = torch.load(g_path, map_location="cpu")["generator"]
    assert list(sd) == order
    inf = env["dissc_amd"].CodeGenerator(h).to(DEV)
    inf.load_state_dict(sd)
    y = inf(code=b[0]["code"], f0=b[0]["f0"], spkr=b[0]["spkr"])
    assert y.shape == (2, 1, h["segment_size"]) and bool(torch.isfinite(y).all())
