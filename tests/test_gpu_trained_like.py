"""Generator parity on trained-like weights and inputs (synthdata kind="trained_like": per-channel gains over decades, outlier
channels, Student-t directions, f0 peaks, exact silence next to loud onsets).  The rounding error of a Toom-Cook form scales with
the largest value of a tile after its input transform and spreads over the whole tile, so the bars measured on benign data are
re-checked here, per layer and on the whole generator, against the float64 oracle (oracle.generator_ref.to_double).

Per layer (every ResBlock conv / residual pair of the VCTK config, through every form with an instance for its shape):
  e_rms  RMS error over the valid outputs against a float64 conv of the same fp32 weights and inputs
  e_ch   the worst output channel's RMS error over that channel's reference RMS (floor: 1e-3 of the layer's RMS)
  leak   on the adversarial rows, the largest |error| at outputs whose receptive field holds no loud sample, in units of
         (loud level x sum|w| x 2^-24): a wrong tile or halo gives ~2^24, which no averaging hides
Inputs: (a) the float64 oracle's tap of the layer on a trained-like T = 99 utterance; (b) rows built from the tap's own channel
statistics: bursts after exact silence with their edges at every offset modulo the forms' tile widths (x dilation), isolated
spikes at 100x the channel RMS, ragged lengths (1, tile +- 1, the kernels' work tiles +- 1, long); NaN beyond every length.
Run with -s for one line per (layer, form)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pair_harness as ph
from generator_cases import FP32_GUARD_RMS, NORTH_STAR_RMS, _generator_with, _rms, _run_conv
from trained_like_cases import (DILS, DIRECT_VS_CPU, GUARD_FACTOR, KS, SLOPE, STAGES, U, _Acc, _adversarial_rows, _batch, _check,  # noqa: F401
                                _plan_conv_form, tl)  # (tl: the module fixture)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------------
# per-layer: the ResBlock convs of the C >= 64 stages through dissc_conv1d
# ------------------------------------------------------------------------------------------------------------------------
def _conv_forms(C, k, d, experimental):
    """(name, wino, wino8, wino8_r4, tile width) of every form dissc_conv1d has an instance for (conv_wino8.hip's
    wino8_supported / wino8_r4_supported, conv_wino.hip's wino_supported)"""
    forms = [("direct", 0, 0, 0, 4), ("F(4,3)", 2, 0, 0, 4)]
    if k in (7, 11) or experimental or (C == 64 and d == 1):
        forms.append(("F(6,3)", 1, 2, 0, 6))
    if k in (7, 11):
        forms.append(("F(5,4)", 1, 2, 2, 5))
    return forms


def _with_options(lib, opts, fn):
    saved = {}
    try:
        for key, v in opts.items():
            cur = ctypes.c_int(0)
            assert lib.dissc_get_option(key.encode(), ctypes.byref(cur)) == 0
            saved[key] = cur.value
            assert lib.dissc_set_option(key.encode(), v) == 0
        return fn()
    finally:
        for key, v in saved.items():
            lib.dissc_set_option(key.encode(), v)


def _ref_conv(x, w, b, k, d, slope, dtype):
    return F.conv1d(F.leaky_relu(x.to(dtype)[None], slope), w.to(dtype), b.to(dtype), padding=(k - 1) * d // 2, dilation=d)[0]


@pytest.mark.parametrize("stage,j", [(i, j) for i in range(3) for j in range(3)])
def test_trained_like_resblock_convs(tl, stage, j):
    """every ResBlock conv of the 256 / 128 / 64-channel stages (convs1 at d = 1 / 3 / 5, convs2 at d = 1) through the direct
    kernel and every transform-domain form with an instance for its shape"""
    lib, folded = tl["lib"], tl["folded"]
    C, k = STAGES[stage], KS[j]
    bad = []
    for grp in (1, 2):
        for m in range(3):
            d = DILS[m] if grp == 1 else 1
            name = f"resblocks.{3 * stage + j}.convs{grp}.{m}"
            w, b = folded[name + ".weight"], folded[name + ".bias"]
            forms = _conv_forms(C, k, d, tl["experimental"])
            tap = tl["inp"][name]
            adv = _adversarial_rows(tap, [f[4] * d for f in forms], seed=1000 * stage + 100 * j + 10 * grp + m)
            rows = [(tap, None)] + adv
            x, lens = _batch(rows)
            pad = (k - 1) * d // 2
            unit = F.leaky_relu(x, SLOPE).abs().amax((1, 2))  # loud level per row
            wsum = w.double().abs().sum((1, 2))
            refs = [_ref_conv(x[i, :, :n], w, b, k, d, SLOPE, torch.float64) for i, n in enumerate(lens)]
            cpu = [_ref_conv(x[i, :, :n], w, b, k, d, SLOPE, torch.float32) for i, n in enumerate(lens)]
            res, outs = {}, {}
            for form, wo, w8, r4, _tile in [("cpu", 0, 0, 0, 0)] + forms:
                acc_a, acc_b = _Acc(C), _Acc(C)
                if form == "cpu":
                    y = cpu
                else:
                    yb = _with_options(lib, dict(wino=wo, wino8=w8, wino8_r4=r4),
                                       lambda: _run_conv(dict(lib=lib, _lib=tl["_lib"]), x, w, b, lens, k, d, SLOPE))
                    outs[form] = yb
                    for i, n in enumerate(lens):
                        assert (yb[i, :, n:] == -7.0).all(), (name, form, i, "wrote beyond the utterance")
                        assert torch.isfinite(yb[i, :, :n]).all(), (name, form, i)
                    y = [yb[i, :, :n] for i, n in enumerate(lens)]
                for i, (r, loud) in enumerate(rows):
                    if i == 0:
                        acc_a.add(y[i], refs[i])
                    else:
                        acc_b.add(y[i], refs[i], loud, pad, float(unit[i]) * wsum * U)
                res[form] = (acc_a.metrics(), acc_b.metrics())
            bad += _check(name, [f[0] for f in forms], res, _plan_conv_form(lib, C, k, d))
            for form, *_ in forms[1:]:
                assert not torch.equal(outs[form], outs["direct"]), (name, form, "the form did not run")
            if "F(6,3)" in outs and "F(5,4)" in outs:
                assert not torch.equal(outs["F(6,3)"], outs["F(5,4)"]), (name, "F(5,4) did not run")
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------
# per-layer: the residual pairs of the 32 / 16-channel stages through dissc_respair1d
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage,j", [(i, j) for i in (3, 4) for j in range(3)])
def test_trained_like_residual_pairs(tl, stage, j):
    """every residual pair of the 32 / 16-channel stages: two direct launches (mode 0), the fused direct pair (mode 1) and every
    register-only form mode 3 can build for the shape (dissc_pair_info: the shipped plan's, and F(2,3) under "pair_tc6" = 0 where
    the plan's is the six-point one); the plan's form is the first of those, the fused direct pair where there is none"""
    C, k = STAGES[stage], KS[j]
    bad = []
    for m, d in enumerate(DILS):
        reg = ph.register_only_forms(tl["_lib"], C, k, d)
        bad += ph.trained_like_pair_layer(tl, C, k, d, f"resblocks.{3 * stage + j}", m, [ph.TL_DIRECT, ph.TL_FUSED] + reg,
                                          reg[0].name if reg else "fused", [2 * d, 4 * d, 6 * d], 1000 * stage + 100 * j + m)
    assert not bad, bad


@pytest.mark.parametrize("name", ["conv_pre"] + [f"ups.{i}" for i in range(5)])
def test_trained_like_outer_layers_on_the_direct_kernels(tl, name):
    """conv_pre (no activation on its input) and the five ConvTranspose1d layers on their float64-oracle inputs, direct
    kernels: e_rms within 4x of CPU fp32.  (Their split-bf16 forms on conv_bf3_kernel have stand-alone entries of their own,
    dissc_conv1d_prec / dissc_conv_transpose1d_prec: tests/test_gpu_gen_split_bf16.py.  Only conv_post, on its own fused kernel
    with the tanh in gen_misc.hip and fp32 in both modes, is reached through the whole-generator tests below alone.)"""
    h = tl["synth"].VCTK_CONFIG
    w, b = tl["folded"][name + ".weight"], tl["folded"][name + ".bias"]
    tap = tl["inp"][name]
    n = tap.shape[1]
    lens = [n, max(1, n // 3), 1]
    x = torch.stack([tap, torch.roll(tap, n // 2, 1), tap])
    if name.startswith("ups"):
        i = int(name[4:])
        u, k = h["upsample_rates"][i], h["upsample_kernel_sizes"][i]
        y = _run_conv(tl, x, w, b, lens, k, 1, SLOPE, transpose=True, stride=u)

        def f(xi, dtype):
            return F.conv_transpose1d(F.leaky_relu(xi.to(dtype)[None], SLOPE), w.to(dtype), b.to(dtype), stride=u,
                                      padding=(k - u) // 2)[0]
    else:
        u, k, slope = 1, w.shape[2], 1.0
        y = _run_conv(tl, x, w, b, lens, k, 1, slope)

        def f(xi, dtype):
            return _ref_conv(xi, w, b, k, 1, slope, dtype)
    acc_g, acc_c = _Acc(y.shape[1]), _Acc(y.shape[1])
    for i, ln in enumerate(lens):
        ref = f(x[i, :, :ln], torch.float64)
        acc_g.add(y[i, :, :ln * u], ref)
        acc_c.add(f(x[i, :, :ln], torch.float32), ref)
        assert (y[i, :, ln * u:] == -7.0).all(), (name, i)
    mg, mc = acc_g.metrics(), acc_c.metrics()
    print(f"TL {name:24s} direct   e_rms {mg['e_rms']:.3e} e_ch {mg['e_ch']:.3e} | cpu-fp32 e_rms {mc['e_rms']:.3e} "
          f"e_ch {mc['e_ch']:.3e} direct/cpu {mg['e_rms'] / mc['e_rms']:.2f}")
    assert mg["e_rms"] <= DIRECT_VS_CPU * mc["e_rms"], (name, mg, mc)


# ------------------------------------------------------------------------------------------------------------------------
# whole generator under every plan
# ------------------------------------------------------------------------------------------------------------------------
PLANS = {
    "default": {},
    "f43": dict(wino8=0),
    "f63": dict(wino8=1, wino8_r4=0, wino8_mask=0o777777777),
    "f54": dict(wino8=1, wino8_r4=1, wino8_mask=0o777777777, wino8_r4_mask=0o777777777),
    "direct": dict(wino=0),
    "pair_direct": dict(pair_f23=0),
    "split_bf16": dict(precision="split_bf16"),
}


@pytest.fixture(scope="module")
def plans(tl):
    out = {}
    for name, opts in PLANS.items():
        opts = dict(opts)
        prec = opts.pop("precision", None)
        out[name] = _generator_with(tl["lib"], tl["synth"], state_dict=tl["sd"], precision=prec, **opts)
    return out


def _run(g, code, f0, spkr, lengths=None):
    kw = dict(code=torch.from_numpy(code), f0=torch.from_numpy(f0), spkr=torch.from_numpy(spkr))
    if lengths is not None:
        kw["lengths"] = torch.from_numpy(lengths)
    return g(**kw).cpu()


def _bars(plan, e, ref_rms, e32o, tag, discriminate=True):
    """north star for every plan; the fp32 guard for the fp32 plans -- and split-bf16 must fail it (discriminate: False for
    clips of a few hundred samples, where the RMS of split-bf16's error does not yet separate from the guard's floor)"""
    guard = max(FP32_GUARD_RMS, GUARD_FACTOR * e32o)
    print(f"TLGEN {tag} {plan:12s} rms {e:.3e} (fp32 oracle {e32o:.3e}, guard {guard:.2e}, signal {ref_rms:.3f})")
    assert e <= NORTH_STAR_RMS and e <= 1e-3 * ref_rms, (tag, plan, e)
    if plan == "split_bf16":
        assert e > guard or not discriminate, (tag, "the fp32 guard no longer rejects split-bf16", e, guard)
    else:
        assert e <= guard, (tag, plan, e, guard)


@pytest.mark.parametrize("T", [33, 99])
def test_trained_like_generator_matches_reference_fixture(tl, plans, golden_dir, T):
    import os
    gold = np.load(os.path.join(golden_dir, "gen_vctk_trainedlike.npz"))
    code, f0, spkr, _ = tl["synth"].synth_generator_inputs(1, T, seed=100 + T, kind="trained_like")
    ref64, ref32 = gold[f"T{T}/wav64"], gold[f"T{T}/wav"]
    e32o = _rms(ref32 - ref64)
    for name, g in plans.items():
        y = _run(g, code, f0, spkr).numpy()
        assert y.shape == ref64.shape and np.isfinite(y).all()
        _bars(name, _rms(y - ref64), _rms(ref64), e32o, f"T={T}")


def test_trained_like_ragged_batch(tl, plans):
    """B = 6 with a 0- and a 1-frame row, inputs poisoned beyond every length: each row against the float64 oracle, zeros
    beyond it, and bit-identical when decoded alone"""
    gr, synth = tl["gr"], tl["synth"]
    code, f0, spkr, lengths = synth.synth_generator_inputs(6, 41, seed=21, ragged=True, kind="trained_like")
    lengths = lengths.copy()
    lengths[1], lengths[2], lengths[4] = 0, 1, 41
    code2, f02 = code.copy(), f0.copy()
    for b in range(6):
        code2[b, lengths[b]:] = 99
        f02[b, 0, lengths[b]:] = 1e9
    w64 = gr.to_double(tl["folded"])
    refs = {}
    for b in range(6):
        n = int(lengths[b])
        if n:
            args = (code[b:b + 1, :n], f0[b:b + 1, :, :n], spkr[b:b + 1])
            refs[b] = (gr.code_generator(w64, synth.VCTK_CONFIG, *args).numpy(),
                       gr.code_generator(tl["folded"], synth.VCTK_CONFIG, *args).numpy())
    for name, g in plans.items():
        y = _run(g, code2, f02, spkr, lengths).numpy()
        assert y.shape == (6, 1, 320 * 41) and np.isfinite(y).all()
        for b in range(6):
            n = int(lengths[b]) * 320
            assert not y[b, :, n:].any(), (name, b, "wrote beyond the row")
            if b in refs:
                r64, r32 = refs[b]
                _bars(name, _rms(y[b:b + 1, :, :n] - r64), max(_rms(r64), 1e-1), _rms(r32 - r64), f"ragged b={b} n={n // 320}",
                      discriminate=n >= 20 * 320)
        for b in (0, 2, 3):
            n = int(lengths[b])
            one = _run(g, code2[b:b + 1, :n], f02[b:b + 1, :, :n], spkr[b:b + 1]).numpy()
            assert np.array_equal(one[0], y[b, :, :320 * n]), (name, b)


@pytest.fixture(scope="module")
def full_case(tl):
    gr, synth = tl["gr"], tl["synth"]
    code, f0, spkr, _ = synth.synth_generator_inputs(32, 500, seed=1234, kind="trained_like")
    w64 = gr.to_double(tl["folded"])
    refs = {}
    for b in (0, 3, 8, 13, 17, 22, 26, 31):  # the oracle on 8 of the 32 utterances
        args = (code[b:b + 1], f0[b:b + 1], spkr[b:b + 1])
        refs[b] = (gr.code_generator(w64, synth.VCTK_CONFIG, *args).numpy(),
                   gr.code_generator(tl["folded"], synth.VCTK_CONFIG, *args).numpy())
    return code, f0, spkr, refs


@pytest.mark.parametrize("plan", list(PLANS))
def test_trained_like_generator_full_size(tl, plans, full_case, plan):
    """B = 32 x T = 500 under each plan: 8 utterances against the float64 oracle, batch independence for 3"""
    code, f0, spkr, refs = full_case
    g = plans[plan]
    y = _run(g, code, f0, spkr).numpy()
    assert y.shape == (32, 1, 160000) and np.isfinite(y).all() and np.abs(y).max() <= 1.0
    for b, (r64, r32) in refs.items():
        _bars(plan, _rms(y[b:b + 1] - r64), _rms(r64), _rms(r32 - r64), f"B=32xT=500 b={b}")
    for b in (7, 19, 30):
        one = _run(g, code[b:b + 1], f0[b:b + 1], spkr[b:b + 1]).numpy()
        assert np.array_equal(one[0], y[b]), (plan, b)
