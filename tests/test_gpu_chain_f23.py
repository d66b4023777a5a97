"""The one-launch F(2,3) chains of the k = 3 ResBlocks of the 32- and 16-channel stages (reschain32_f23_kernel in respair_f23.hip,
reschain16_f23_kernel in respair16_f23.hip; option "chain_f23") through the C ABI (dissc_reschain1d mode 1) against float64 and
against the three one-launch pairs they replace (mode 0): lengths around the halo, the tile, two tiles and a wave's owned span;
batch independence; the four epilogues; an empty row; then the switches that leave the shipped three-pair plan, and the whole
generator with the option on against off.  Data, reference and bars: tests/chain_model.py (tests/test_chain_f23_model_cpu.py holds
the same data to the same bars in a numpy model of the kernels).  Run with -s for the measured figures."""
import ctypes

import pytest
import torch

import chain_model as cm
import pair_harness as ph
import trained_like_cases as ttl
from generator_cases import FP32_GUARD_RMS, _generator_with, _pair_cases, _rms
from trained_like_cases import tl  # noqa: F401  (its module fixture: trained-like checkpoint and the float64 oracle's layer taps)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dissc_amd import _lib
    return _lib


def run_chain(lib, mode, x, w6, b6, lengths, epi=1, acc=None, k=cm.K, dils=cm.DILS, div=3.0, check=True):
    """x / acc on the device, the six weights and biases on the host; y starts as the sentinel -7.  Returns (rc, y or acc)"""
    B, C, ld = x.shape
    y = torch.full_like(x, -7.0)
    ln = torch.as_tensor(lengths, dtype=torch.int32, device=DEV)
    a = None if acc is None else acc.clone()
    wp = (ctypes.c_void_p * 6)(*[w.data_ptr() for w in w6])
    bp = (ctypes.c_void_p * 6)(*[b.data_ptr() for b in b6])
    dl = (ctypes.c_int32 * 3)(*dils)
    rc = lib.lib.dissc_reschain1d(x.data_ptr(), wp, bp, y.data_ptr(), None if a is None else a.data_ptr(), ln.data_ptr(), B, C, k, dl, ld,
                                  int(max(lengths)), ctypes.c_float(cm.SLOPE), epi, ctypes.c_float(div), mode, None)
    if check:
        lib.check(rc, f"dissc_reschain1d mode {mode}")
    return rc, (y if epi == 1 else a)


@pytest.mark.parametrize("C", [32, 16])
def test_chain_matches_float64_and_the_three_launches(lib, C):
    """every length of chain_model.lengths_for; NaN beyond every utterance and a sentinel behind it; rms <= max(3 x the three
    launches', 1e-6) and max <= 3 x the three launches' max; other bits than the three launches; rows alone and as a repeated row
    against the same rows in the batch; EPI_RES and the three MRF epilogues, the accumulator untouched beyond every length"""
    lengths = cm.lengths_for(C)
    x, w6, b6 = cm.data(C, lengths, cm.LD, seed=2300 + C)
    x = x.to(DEV)
    ref = cm.reference(x, w6, b6, lengths)
    y = run_chain(lib, 1, x, w6, b6, lengths)[1]
    y0 = run_chain(lib, 0, x, w6, b6, lengths)[1]
    for i, n in enumerate(lengths):
        assert torch.isfinite(y[i, :, :n]).all(), (i, n)
        assert (y[i, :, n:] == -7.0).all(), f"utterance {i}: wrote beyond its {n} samples"
    err, base = cm.errors(y, ref, lengths), cm.errors(y0, ref, lengths)
    print(f"C={C}: chain max err {err[0]:.2e} rms {err[1]:.2e}; three launches {base[0]:.2e} / {base[1]:.2e}")
    assert not torch.equal(y[0], y0[0])  # (not the three launches' kernels)
    assert cm.within_bars(err, base), (err, base)
    for i in (1, 3, 5, 12, len(lengths) - 6, len(lengths) - 2):
        one = run_chain(lib, 1, x[i:i + 1].clone(), w6, b6, lengths[i:i + 1])[1]
        assert torch.equal(one[0, :, :lengths[i]], y[i, :, :lengths[i]]), i
    i = lengths.index(cm.geo(C).wout + 1)
    rep = run_chain(lib, 1, x[i:i + 1].repeat(5, 1, 1), w6, b6, [lengths[i]] * 5)[1]
    for j in range(5):
        assert torch.equal(rep[j, :, :lengths[i]], y[i, :, :lengths[i]]), j
    acc0 = torch.rand(len(lengths), C, cm.LD, device=DEV)
    for epi in (2, 3, 4):
        a = run_chain(lib, 1, x, w6, b6, lengths, epi=epi, acc=acc0)[1]
        for i, n in enumerate(lengths):
            want = y[i, :, :n] if epi == 2 else acc0[i, :, :n] + y[i, :, :n]
            if epi == 4:  # on the CPU: a true division (pair_harness.check_pair)
                want = (want.cpu() / 3.0).to(DEV)
            assert torch.equal(a[i, :, :n], want), (epi, i)
            assert torch.equal(a[i, :, n:], acc0[i, :, n:])


@pytest.mark.parametrize("C", [32, 16])
def test_an_empty_row_in_a_70_row_batch(lib, C):
    """70 ragged rows, one of them empty: every row equals itself alone in bits and float64 within 1e-5; nothing is written to
    the empty row"""
    g = torch.Generator().manual_seed(70 + C)
    lengths = [int(v) for v in torch.randint(1, 601, (70,), generator=g)]
    lengths[0], lengths[33] = 600, 0
    x, w6, b6 = cm.data(C, lengths, 600, seed=70 + C)
    x = x.to(DEV)
    ref = cm.reference(x, w6, b6, lengths)
    y = run_chain(lib, 1, x, w6, b6, lengths)[1]
    assert (y[33] == -7.0).all()
    for i, n in enumerate(lengths):
        assert (y[i, :, n:] == -7.0).all(), i
        if n:
            assert float((y[i, :, :n].double() - ref[i, :, :n]).abs().max()) <= 1e-5, (i, n)
    for i in (0, 32, 34, 69):
        one = run_chain(lib, 1, x[i:i + 1].clone(), w6, b6, lengths[i:i + 1])[1]
        assert torch.equal(one[0, :, :lengths[i]], y[i, :, :lengths[i]]), i


@pytest.mark.parametrize("C,k,dils", [(64, 3, (1, 3, 5)), (32, 7, (1, 3, 5)), (32, 3, (1, 3, 3)), (16, 3, (1, 1, 1))])
def test_mode_1_refuses_a_shape_without_an_instance(lib, C, k, dils):
    lengths = [64]
    g = torch.Generator().manual_seed(1)
    x = torch.rand(1, C, 64, generator=g).to(DEV)
    w6 = [torch.rand(C, C, k, generator=g) * 0.01 for _ in range(6)]
    b6 = [torch.zeros(C) for _ in range(6)]
    rc, y = run_chain(lib, 1, x, w6, b6, lengths, k=k, dils=dils, check=False)
    assert rc != 0 and (y == -7.0).all()
    info = lib.DisscChainInfo()
    assert lib.lib.dissc_chain_info(C, k, (ctypes.c_int32 * 3)(*dils), ctypes.byref(info)) != 0


def _ref_chain(x, w6, b6, dtype):
    for m, d in enumerate(cm.DILS):
        x = ttl._ref_pair(x, w6[2 * m], b6[2 * m], w6[2 * m + 1], b6[2 * m + 1], cm.K, d, dtype)
    return x


@pytest.mark.parametrize("stage,C", [(3, 32), (4, 16)])
def test_trained_like_chains(tl, stage, C):  # noqa: F811
    """the k = 3 ResBlock of the stage (resblocks.9 / resblocks.12) with its trained-like weights, as one chain launch (mode 1)
    and as the three launches (mode 0, "direct"), against float64: (a) the float64 oracle's input of the block; (b) the
    adversarial rows of pair_harness.trained_like_pair_layer (bursts after silence at every offset modulo the unit widths 2 d,
    spikes, ragged lengths) drawn from the oracle's inputs of all three layers, and windows of them around the chain's tile.
    A one-launch chain has no output per layer, so "the chain's three layers" is read as: the bars on the BLOCK's output, with
    every layer's own oracle input among the rows.  The bars of trained_like_cases._check with the chain as the plan's form: TD_RMS and TD_CH x the three launches', LEAK.
    Leak unit: a loud input of size u reaches an output through at most prod_m (1 + s1_m s2_m) u, s = a conv's largest
    absolute row sum; the last conv's own row sums keep it per channel."""
    lib, folded = tl["_lib"], tl["folded"]
    p = f"resblocks.{3 * stage}"
    w6 = [folded[f"{p}.convs{1 + l % 2}.{l // 2}.weight"].contiguous() for l in range(6)]
    b6 = [folded[f"{p}.convs{1 + l % 2}.{l // 2}.bias"].contiguous() for l in range(6)]
    assert w6[0].shape == (C, C, cm.K)
    taps = [tl["inp"][f"{p}.convs1.{m}"] for m in range(3)]
    wout = cm.geo(C).wout
    rows = [(taps[0], None)]
    for m in range(3):
        rows += ttl._adversarial_rows(taps[m], [2 * d for d in cm.DILS] + [wout], seed=2300 + 10 * stage + m)
        rows += [(taps[m][:, c0:c0 + ln].clone(), None) for c0, ln in ph.tile_windows(wout)]
    x, lens = ttl._batch(rows)
    xd = x.to(DEV)
    for i, n in enumerate(lens):
        xd[i, :, n:] = float("nan")  # never read
    s = [float(w.double().abs().sum((1, 2)).max()) for w in w6]
    gain = (1 + s[0] * s[1]) * (1 + s[2] * s[3])
    wsum = gain * (1.0 + w6[5].double().abs().sum((1, 2)) * s[4])
    unit = torch.nn.functional.leaky_relu(x, ttl.SLOPE).abs().amax((1, 2)).clamp(min=1e-30)
    refs = [_ref_chain(x[i, :, :n], w6, b6, torch.float64) for i, n in enumerate(lens)]
    res, outs = {}, {}
    for name, mode in (("cpu", None), ("direct", 0), ("chain", 1)):
        if mode is None:
            y = [_ref_chain(x[i, :, :n], w6, b6, torch.float32) for i, n in enumerate(lens)]
        else:
            yb = run_chain(lib, mode, xd, w6, b6, lens)[1].cpu()
            for i, n in enumerate(lens):
                assert (yb[i, :, n:] == -7.0).all(), (name, i, "wrote beyond the utterance")
                assert torch.isfinite(yb[i, :, :n]).all(), (name, i)
            y = [yb[i, :, :n] for i, n in enumerate(lens)]
            outs[name] = yb
        acc_a, acc_b = ttl._Acc(C), ttl._Acc(C)
        for i, (r, loud) in enumerate(rows):
            if i == 0:
                acc_a.add(y[i], refs[i])
            else:
                acc_b.add(y[i], refs[i], loud, cm.geo(C).halo, float(unit[i]) * wsum * ttl.U)
        res[name] = (acc_a.metrics(), acc_b.metrics())
    assert not torch.equal(outs["chain"], outs["direct"])  # (the chain kernel really ran)
    worst = max(float((outs["chain"][i, :, :n].double() - refs[i]).abs().max()) for i, n in enumerate(lens))
    worst0 = max(float((outs["direct"][i, :, :n].double() - refs[i]).abs().max()) for i, n in enumerate(lens))
    print(f"TL {p}: max error chain {worst:.3e}, three launches {worst0:.3e}")
    bad = ttl._check(f"{p}.chain", ["direct", "chain"], res, "chain")
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------
# the whole generator
# ------------------------------------------------------------------------------------------------------------------------
def _wave(g, case):
    code, f0, spkr, lengths = case
    return g(code=torch.from_numpy(code), f0=torch.from_numpy(f0), spkr=torch.from_numpy(spkr), lengths=torch.from_numpy(lengths)).cpu()


def test_each_switch_leaves_the_three_pair_plan(lib):
    """chain_f23 = 0, pair_f23 = 0, pair_max_c = 0, wino = 0 and precision = 1 each give the plan a handle without the chains runs: bit for bit the
    waveform, and the executed FLOPs, of a "chain_f23" = 0 handle under the same setting (wino = 0 changes the wide stages too, so
    there as well the handle to compare with is the "chain_f23" = 0 one with wino = 0)"""
    import synthdata as synth
    L = lib.lib
    case = _pair_cases(synth)[0]
    g_off = _generator_with(L, synth, chain_f23=0)
    y_off = _wave(g_off, case)
    g_on = _generator_with(L, synth, chain_f23=3)
    assert not torch.equal(_wave(g_on, case), y_off)  # (the switch under test does something)
    assert torch.equal(_wave(_generator_with(L, synth, chain_f23=0), case), y_off)
    for kw in (dict(wino=0), dict(pair_f23=0), dict(pair_max_c=0), dict(precision="split_bf16")):
        a, b = _generator_with(L, synth, chain_f23=3, **kw), _generator_with(L, synth, chain_f23=0, **kw)
        assert torch.equal(_wave(a, case), _wave(b, case)), kw
        assert a.flops_executed(1000) == b.flops_executed(1000), kw


@pytest.mark.parametrize("mask", [1, 2, 3])
def test_generator_with_chains_agrees_with_the_three_pair_plan(lib, mask):
    """a handle with "chain_f23" = mask against one with 0: the waveform to fp32 rounding (rms <= 2e-6, max <= 5e-5), the
    algorithmic FLOPs equal, the executed ones lower by exactly 2 frames mul 3 2 C^2 per enabled stage, one utterance alone the
    same bits, and the fp32 parity guard against the float64 oracle on the two shortest rows"""
    import synthdata as synth
    from oracle import generator_ref as gr
    L = lib.lib
    g = _generator_with(L, synth, chain_f23=mask)
    g0 = _generator_with(L, synth, chain_f23=0)
    assert g.flops(1000) == g0.flops(1000)
    assert synth.VCTK_CONFIG["upsample_rates"] == [5, 4, 4, 2, 2] and synth.VCTK_CONFIG["upsample_initial_channel"] == 512
    want = 0.0
    for bit, C, mul in ((1, 32, 160), (2, 16, 320)):
        if mask & bit:
            want -= 2.0 * 1000 * mul * 3 * 2 * C * C
    got = g.flops_executed(1000) - g0.flops_executed(1000)
    print(f"executed FLOPs per 1000 frames: {g.flops_executed(1000):.6g} against {g0.flops_executed(1000):.6g}")
    assert abs(got - want) <= 1e-9 * g.flops_executed(1000), (got, want)
    folded64 = gr.to_double(gr.fold_state_dict(synth.synth_generator_state_dict(seed=0)))
    cases = _pair_cases(synth) + [synth.synth_generator_inputs(3, 1203, seed=5, ragged=True)]
    if mask != 3:
        cases = cases[:1]  # (the single bits: the short ragged case only)
    for case in cases:
        code, f0, spkr, lengths = case
        y, y0 = _wave(g, case), _wave(g0, case)
        assert torch.isfinite(y).all()
        assert not torch.equal(y, y0)  # (the new kernels really ran)
        e = (y - y0).double()
        rms = float(e.pow(2).mean().sqrt())
        print(f"mask {mask} B={code.shape[0]} T={code.shape[1]}: chains vs three pairs: rms {rms:.2e}, max {float(e.abs().max()):.2e}")
        assert rms <= 2e-6 and float(e.abs().max()) <= 5e-5
        one = _wave(g, (code[:1], f0[:1], spkr[:1], lengths[:1]))[0]
        assert torch.equal(one, y[0])
        for b in sorted(range(len(lengths)), key=lambda i: int(lengths[i]))[:2]:
            n = int(lengths[b])
            if n == 0:
                continue
            ref = gr.code_generator(folded64, synth.VCTK_CONFIG, code[b:b + 1, :n], f0[b:b + 1, :, :n], spkr[b:b + 1]).numpy()
            err = _rms(y[b:b + 1, :, :320 * n].numpy() - ref)
            print(f"  row {b} ({n} frames): rms against float64 {err:.2e}")
            assert err <= FP32_GUARD_RMS, (b, err)
