"""GPU parity tests of the HIP generator path (through the C ABI) against the CPU
oracle and the committed reference golden vectors.  Run with -m gpu on an MI355X."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from generator_cases import FP32_GUARD_RMS, NORTH_STAR_RMS, _generator_with, _pair_cases, _rms, _run_conv

pytestmark = pytest.mark.gpu

WINO_SV_DEFAULT = 1  # csrc/conv_wino.hip g_wino_sv


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import dissc_amd
    from dissc_amd import _lib
    from oracle import generator_ref as gr
    import synthdata as synth
    sd = synth.synth_generator_state_dict(seed=0)
    g = dissc_amd.CodeGenerator(synth.VCTK_CONFIG).to("cuda:0")
    g.load_state_dict(sd)
    g.eval()
    g.remove_weight_norm()
    return dict(lib=_lib.lib, _lib=_lib, gr=gr, synth=synth, g=g, folded=gr.fold_state_dict(sd))


@pytest.mark.parametrize("C,k,d", [(16, 3, 1), (16, 11, 5), (32, 7, 3), (64, 11, 1), (128, 3, 5),
                                   (256, 7, 1), (48, 5, 2), (20, 3, 1)])
def test_conv1d_matches_torch(env, C, k, d):
    rs = np.random.RandomState(C * 100 + k * 10 + d)
    B, L = 3, 700
    lengths = [700, 333, 1]
    x = torch.from_numpy(rs.standard_normal((B, C, L)).astype(np.float32))
    w = torch.from_numpy((rs.standard_normal((C, C, k)) / np.sqrt(C * k)).astype(np.float32))
    b = torch.from_numpy(rs.standard_normal(C).astype(np.float32))
    y = _run_conv(env, x, w, b, lengths, k, d, 0.1)
    for i, n in enumerate(lengths):
        ref = F.conv1d(F.leaky_relu(x[i:i + 1, :, :n], 0.1), w, b, padding=(k - 1) * d // 2, dilation=d)
        err = (y[i, :, :n] - ref[0]).abs().max().item()
        assert err <= 2e-5, (i, err)
        assert (y[i, :, n:] == -7.0).all()  # nothing written beyond the utterance


@pytest.mark.parametrize("C,k,d", [(64, 11, 1), (64, 3, 5), (64, 7, 3), (128, 7, 3), (128, 3, 1), (128, 11, 5),
                                   (256, 11, 1), (256, 7, 1), (256, 3, 3)])
def test_toom_cook_conv_matches_torch_and_the_direct_kernel(env, C, k, d):
    """conv_wino_kernel (Toom-Cook F(4,3) over 3-tap sub-filters, csrc/conv_wino.hip) through the stand-alone entry
    (option "wino" = 2): same bar against F.conv1d as the direct kernel, rms error within 2x of the direct kernel's,
    ragged lengths incl. 1 and tile-boundary cases, NaN-poisoned padding, nothing written beyond an utterance."""
    lib = env["lib"]
    rs = np.random.RandomState(C * 100 + k * 10 + d)
    lengths = [1000, 1, 255, 256, 257, 613, 240, 241]
    B, L = len(lengths), 1000
    x = torch.from_numpy(rs.standard_normal((B, C, L)).astype(np.float32))
    w = torch.from_numpy((rs.standard_normal((C, C, k)) / np.sqrt(C * k)).astype(np.float32))
    b = torch.from_numpy(rs.standard_normal(C).astype(np.float32))
    out = {}
    try:
        for mode in (0, 2):
            assert lib.dissc_set_option(b"wino", mode) == 0
            out[mode] = _run_conv(env, x, w, b, lengths, k, d, 0.1)
        # this launch is small (8 utterances x 1000 columns): it ran on 32 x 32 wave tiles.  The 64 x 64 tiles of a
        # chip-filling launch ("small_grid" = 0 forces them) must give the same bits.
        assert lib.dissc_set_option(b"small_grid", 0) == 0
        big = _run_conv(env, x, w, b, lengths, k, d, 0.1)
        # ... and so must both forms of the input transform (option "wino_sv": 0 = each wave its own V tile, 1 = shared
        # between the waves for C >= 128)
        forms = []
        for sv in (0, 1):
            assert lib.dissc_set_option(b"wino_sv", sv) == 0
            forms.append(_run_conv(env, x, w, b, lengths, k, d, 0.1))
    finally:
        lib.dissc_set_option(b"wino", 1)
        lib.dissc_set_option(b"small_grid", 1)
        lib.dissc_set_option(b"wino_sv", WINO_SV_DEFAULT)
    assert torch.equal(big, out[2])
    for f in forms:
        assert torch.equal(f, out[2])
    assert not torch.equal(out[0], out[2])  # really another evaluation order
    se = {0: 0.0, 2: 0.0}
    cnt = 0
    for i, n in enumerate(lengths):
        ref = F.conv1d(F.leaky_relu(x[i:i + 1, :, :n].double(), 0.1), w.double(), b.double(), padding=(k - 1) * d // 2,
                       dilation=d)[0]
        for mode in (0, 2):
            y = out[mode]
            e = (y[i, :, :n].double() - ref)
            assert e.abs().max().item() <= 2e-5, (mode, i, e.abs().max().item())
            assert (y[i, :, n:] == -7.0).all()  # nothing written beyond the utterance
            se[mode] += float((e ** 2).sum())
        cnt += ref.numel()
    r0, r2 = (se[0] / cnt) ** 0.5, (se[2] / cnt) ** 0.5
    print(f"C={C} k={k} d={d}: rms error direct {r0:.2e}, transform domain {r2:.2e}")
    assert r2 <= 2.0 * r0 + 1e-8


def test_toom_cook_conv_rejects_unaligned_rows(env):
    """conv_wino_kernel moves 16 bytes at a time: a row stride that is not a multiple of 4 floats (or a base pointer
    off a 16-byte boundary) is refused with DISSC_EINVAL and a message, never launched."""
    lib, _lib = env["lib"], env["_lib"]
    C, k, L = 64, 7, 64
    w = torch.zeros(C, C, k)
    b = torch.zeros(C)
    x = torch.zeros(1, C, 72, device="cuda")
    y = torch.zeros(1, C, 72, device="cuda")
    try:
        assert lib.dissc_set_option(b"wino", 2) == 0
        for ldx, ldo, xoff in ((66, 68, 0), (68, 66, 0), (68, 68, 4)):
            rc = lib.dissc_conv1d(x.data_ptr() + xoff, w.data_ptr(), b.data_ptr(), y.data_ptr(), None, 1, C, C, k, 1,
                                  ldx, ldo, L, ctypes.c_float(0.1), None)
            assert rc != 0
            assert b"16-byte" in lib.dissc_last_error()
        rc = lib.dissc_conv1d(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), None, 1, C, C, k, 1, 68, 68, L,
                              ctypes.c_float(0.1), None)
        _lib.check(rc, "conv")
    finally:
        lib.dissc_set_option(b"wino", 1)
    torch.cuda.synchronize()
    assert (y == 0).all()


def test_toom_cook_conv_random_shapes(env):
    """tools/wino_fuzz.py: random (C, k, d, B, row length, ragged utterance lengths) -- both transform forms and both tile
    sizes bit-identical, within fp32 rounding of the direct kernel, nothing written beyond an utterance."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "wino_fuzz.py"), "24", "3"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "24 cases ok" in r.stdout


def test_toom_cook_generator_agrees_with_the_direct_generator(env):
    """The default generator (wide ResBlock convs in the transform domain) against an instance built with option
    "wino" = 0 (every conv direct, the round-2 path): same waveform to fp32 rounding on a ragged batch and at the
    BASELINE size; the direct instance stays available and bit-identical to itself across batch shapes."""
    import dissc_amd
    lib, g, synth = env["lib"], env["g"], env["synth"]
    try:
        assert lib.dissc_set_option(b"wino", 0) == 0
        gd = dissc_amd.CodeGenerator(synth.VCTK_CONFIG).to("cuda:0")
        gd.load_state_dict(synth.synth_generator_state_dict(seed=0))
        gd.eval().remove_weight_norm()
        c1, f1, s1, _ = synth.synth_generator_inputs(1, 3, seed=1)
        gd(code=torch.from_numpy(c1), f0=torch.from_numpy(f1), spkr=torch.from_numpy(s1))  # the native handle is built here
    finally:
        lib.dissc_set_option(b"wino", 1)
    code, f0, spkr, lengths = synth.synth_generator_inputs(6, 41, seed=21, ragged=True)
    lengths = lengths.copy()
    lengths[1], lengths[2] = 1, 41
    for (c, f, s_, ln) in ((code, f0, spkr, lengths), synth.synth_generator_inputs(32, 500, seed=1234)):
        kw = dict(code=torch.from_numpy(c), f0=torch.from_numpy(f), spkr=torch.from_numpy(s_), lengths=torch.from_numpy(ln))
        yw, yd = g(**kw).cpu(), gd(**kw).cpu()
        assert torch.isfinite(yw).all() and not torch.equal(yw, yd)
        e = (yw - yd).double()
        rms, ref = float(e.pow(2).mean().sqrt()), float(yd.double().pow(2).mean().sqrt())
        print(f"B={c.shape[0]} T={c.shape[1]}: transform-domain vs direct generator: rms {rms:.2e} (signal rms {ref:.2f}), "
              f"max {float(e.abs().max()):.2e}")
        assert rms <= 5e-6 and float(e.abs().max()) <= 1e-4
        assert torch.equal(gd(code=kw["code"][:1], f0=kw["f0"][:1], spkr=kw["spkr"][:1], lengths=kw["lengths"][:1]).cpu()[0],
                           yd[0])


def test_conv1d_rect_and_identity_slope(env):
    rs = np.random.RandomState(3)
    x = torch.from_numpy(rs.standard_normal((2, 257, 130)).astype(np.float32))
    w = torch.from_numpy((rs.standard_normal((512, 257, 7)) / 42.0).astype(np.float32))
    b = torch.from_numpy(rs.standard_normal(512).astype(np.float32))
    y = _run_conv(env, x, w, b, None, 7, 1, 1.0)
    ref = F.conv1d(x, w, b, padding=3)
    assert (y - ref).abs().max().item() <= 2e-5


@pytest.mark.parametrize("cin,k,s", [(512, 11, 5), (256, 8, 4), (128, 8, 4), (64, 4, 2), (32, 4, 2)])
def test_conv_transpose_matches_torch(env, cin, k, s):
    rs = np.random.RandomState(cin + k)
    B, L = 2, 150
    lengths = [150, 37]
    cout = cin // 2
    x = torch.from_numpy(rs.standard_normal((B, cin, L)).astype(np.float32))
    w = torch.from_numpy((rs.standard_normal((cin, cout, k)) / np.sqrt(cin * k / s)).astype(np.float32))
    b = torch.from_numpy(rs.standard_normal(cout).astype(np.float32))
    y = _run_conv(env, x, w, b, lengths, k, 1, 0.1, transpose=True, stride=s)
    for i, n in enumerate(lengths):
        ref = F.conv_transpose1d(F.leaky_relu(x[i:i + 1, :, :n], 0.1), w, b, stride=s, padding=(k - s) // 2)
        assert ref.shape[-1] == n * s
        err = (y[i, :, :n * s] - ref[0]).abs().max().item()
        assert err <= 2e-5, (i, err)


@pytest.mark.parametrize("T", [1, 2, 7, 33, 99])
def test_generator_matches_reference_golden(env, golden_dir, T):
    gold = np.load(os.path.join(golden_dir, "gen_vctk.npz"))
    code, f0, spkr, _ = env["synth"].synth_generator_inputs(1, T, seed=100 + T)
    y = env["g"](code=torch.from_numpy(code), f0=torch.from_numpy(f0), spkr=torch.from_numpy(spkr))
    torch.cuda.synchronize()
    ref = gold[f"s0/T{T}/wav"]
    assert tuple(y.shape) == ref.shape
    err = y.cpu().numpy() - ref
    # north_star tolerance: <= 1e-4 RMS vs the reference CPU path (and 1e-3 relative) -- and the fp32 regression guard
    print(f"golden T={T}: rms {_rms(err):.3e} (guard {FP32_GUARD_RMS:.0e}, bar {NORTH_STAR_RMS:.0e})")
    assert _rms(err) <= NORTH_STAR_RMS, _rms(err)
    assert _rms(err) <= FP32_GUARD_RMS, _rms(err)
    assert _rms(err) <= 1e-3 * _rms(ref)
    assert np.abs(err).max() <= 1e-3


@pytest.mark.parametrize("case", ["code_short", "f0_short", "code_short3"])
def test_generator_upsample_branches_match_reference_golden(env, golden_dir, case):
    """`_upsample` of the shorter stream (code OR f0; reference sr/models.py:206-210) in the HIP path's front end"""
    gold = np.load(os.path.join(golden_dir, "gen_upsample.npz"))
    y = env["g"](code=torch.from_numpy(gold[f"{case}/code"]), f0=torch.from_numpy(gold[f"{case}/f0"]),
                 spkr=torch.from_numpy(gold[f"{case}/spkr"])).cpu().numpy()
    ref = gold[f"{case}/wav"]
    assert y.shape == ref.shape
    assert _rms(y - ref) <= FP32_GUARD_RMS, _rms(y - ref)


def test_generator_ragged_batch_matches_reference_golden(env, golden_dir):
    gold = np.load(os.path.join(golden_dir, "gen_vctk.npz"))
    code, f0, spkr, _ = env["synth"].synth_generator_inputs(4, 40, seed=777)
    lengths = gold["s0/ragged/lengths"]
    # poison inputs beyond each length
    code2, f02 = code.copy(), f0.copy()
    for b in range(4):
        code2[b, lengths[b]:] = 99
        f02[b, 0, lengths[b]:] = 1e9
    y = env["g"](code=torch.from_numpy(code2), f0=torch.from_numpy(f02), spkr=torch.from_numpy(spkr),
                 lengths=torch.from_numpy(lengths)).cpu().numpy()
    for b in range(4):
        n = int(lengths[b]) * 320
        ref = gold[f"s0/ragged/wav{b}"][0]
        assert _rms(y[b, :, :n] - ref) <= NORTH_STAR_RMS
        assert _rms(y[b, :, :n] - ref) <= FP32_GUARD_RMS, (b, _rms(y[b, :, :n] - ref))
        assert not y[b, :, n:].any()


def test_generator_full_size_properties(env):
    """BASELINE config: B=32 x T=500.  Oracle on 8 of the 32 utterances + batch-independence
    (an utterance's samples do not depend on what it is batched with)."""
    g, gr, synth = env["g"], env["gr"], env["synth"]
    code, f0, spkr, _ = synth.synth_generator_inputs(32, 500, seed=1234)
    tc, tf, ts = torch.from_numpy(code), torch.from_numpy(f0), torch.from_numpy(spkr)
    y = g(code=tc, f0=tf, spkr=ts).cpu()
    assert tuple(y.shape) == (32, 1, 160000)
    assert torch.isfinite(y).all() and y.abs().max() <= 1.0
    worst = 0.0
    for b in (0, 3, 8, 13, 17, 22, 26, 31):  # the oracle on 8 of the 32 utterances (~1-2 s of CPU each)
        ref = gr.code_generator(env["folded"], synth.VCTK_CONFIG, code[b:b + 1], f0[b:b + 1], spkr[b:b + 1])
        e = (y[b:b + 1] - ref).numpy()
        assert _rms(e) <= NORTH_STAR_RMS and _rms(e) <= 1e-3 * _rms(ref.numpy()), (b, _rms(e))
        assert _rms(e) <= FP32_GUARD_RMS, (b, _rms(e))
        worst = max(worst, _rms(e))
    print(f"B=32 x T=500: worst RMS error vs the oracle over 8 utterances = {worst:.3e}")
    for b in (7, 19, 30):  # batch independence: an utterance on its own is bit-identical
        y1 = g(code=tc[b:b + 1], f0=tf[b:b + 1], spkr=ts[b:b + 1]).cpu()
        assert torch.equal(y1[0], y[b])
    # determinism: same launch twice -> identical bits
    y2 = g(code=tc, f0=tf, spkr=ts).cpu()
    assert torch.equal(y, y2)


def test_fp32_guard_rejects_split_bf16(env):
    """The regression guard does its job: the same comparison that passes for the exact-fp32 handle FAILS for a handle built with
    precision="split_bf16" (three bf16 products per fp32 product: ~10x the error, still 25x inside the north-star bar) -- so
    swapping the noisier arithmetic in by accident (DISSC_OPTIONS=precision=1, a changed default) cannot pass silently."""
    import dissc_amd
    g, gr, synth = env["g"], env["gr"], env["synth"]
    gs = dissc_amd.CodeGenerator(synth.VCTK_CONFIG, precision="split_bf16").to("cuda:0")
    gs.load_state_dict(synth.synth_generator_state_dict(seed=0))
    gs.eval().remove_weight_norm()
    for T, seed in ((99, 199), (500, 1234)):
        code, f0, spkr, _ = synth.synth_generator_inputs(2, T, seed=seed)
        tc, tf, ts = torch.from_numpy(code), torch.from_numpy(f0), torch.from_numpy(spkr)
        ref = gr.code_generator(env["folded"], synth.VCTK_CONFIG, code[1:2], f0[1:2], spkr[1:2]).numpy()
        e32 = _rms(g(code=tc, f0=tf, spkr=ts).cpu().numpy()[1:2] - ref)
        ebf = _rms(gs(code=tc, f0=tf, spkr=ts).cpu().numpy()[1:2] - ref)
        print(f"T={T}: fp32 rms {e32:.3e}, split-bf16 rms {ebf:.3e}, guard {FP32_GUARD_RMS:.0e}")
        assert e32 <= FP32_GUARD_RMS < ebf <= NORTH_STAR_RMS, (T, e32, ebf)
        assert FP32_GUARD_RMS <= 10 * e32, (T, e32)  # the guard stays within 10x of what the kernels deliver


def test_split_bf16_instance_next_to_fp32_instance(env):
    """CodeGenerator(h, precision="split_bf16") at the BASELINE size: within the 1e-4 RMS bar of the
    oracle, batch-independent and deterministic like the fp32 path -- and building it leaves the
    process default (exact fp32) untouched for instances created afterwards."""
    import dissc_amd
    g, gr, synth = env["g"], env["gr"], env["synth"]
    sd = synth.synth_generator_state_dict(seed=0)
    gs = dissc_amd.CodeGenerator(synth.VCTK_CONFIG, precision="split_bf16").to("cuda:0")
    gs.load_state_dict(sd)
    gs.eval().remove_weight_norm()
    code, f0, spkr, _ = synth.synth_generator_inputs(32, 500, seed=1234)
    tc, tf, ts = torch.from_numpy(code), torch.from_numpy(f0), torch.from_numpy(spkr)
    y32 = g(code=tc, f0=tf, spkr=ts).cpu()
    ys = gs(code=tc, f0=tf, spkr=ts).cpu()
    d = _rms((ys - y32).numpy())
    assert 0.0 < d <= 2e-5, d                      # really a different arithmetic, far inside the bar
    ref = gr.code_generator(env["folded"], synth.VCTK_CONFIG, code[3:4], f0[3:4], spkr[3:4])
    assert _rms((ys[3:4] - ref).numpy()) <= 1e-4   # north_star tolerance vs the reference CPU path
    assert torch.equal(gs(code=tc[7:8], f0=tf[7:8], spkr=ts[7:8]).cpu()[0], ys[7])
    assert torch.equal(gs(code=tc, f0=tf, spkr=ts).cpu(), ys)
    g2 = dissc_amd.CodeGenerator(synth.VCTK_CONFIG).to("cuda:0")  # default: exact fp32
    g2.load_state_dict(sd)
    g2.eval().remove_weight_norm()
    assert torch.equal(g2(code=tc[:4], f0=tf[:4], spkr=ts[:4]).cpu(), y32[:4])
    with pytest.raises(ValueError):
        dissc_amd.CodeGenerator(synth.VCTK_CONFIG, precision="fp8")


def test_wav_postprocess_matches_oracle(env):
    from dissc_amd.generator import wav_postprocess_
    rs = np.random.RandomState(0)
    y = np.tanh(rs.standard_normal((3, 1, 5000)).astype(np.float32) * 2)
    y[0, 0, :4] = [1.0, -1.0, 0.99999, 3.5 / 32768]
    n = np.array([5000, 1234, 1], dtype=np.int32)
    d = torch.from_numpy(y.copy()).cuda()
    wav_postprocess_(d, n)
    out = d.cpu().numpy()
    for b in range(3):
        want = env["gr"].wav_postprocess(y[b, 0, :n[b]])
        np.testing.assert_array_equal(out[b, 0, :n[b]], want)
        np.testing.assert_array_equal(out[b, 0, n[b]:], y[b, 0, n[b]:])


def test_split_bf16_precision_option_is_within_north_star_tolerance(golden_dir):
    """Opt-in DISSC_OPTIONS=precision=1 (split-bf16 products on the bf16 matrix cores, fp32
    accumulate): not bit-comparable with fp32, but must stay far inside the 1e-4 RMS bar."""
    import subprocess
    import sys
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DISSC_OPTIONS="precision=1")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "precision_check.py")], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines() if "rms_err" in ln]
    assert len(rows) == 4
    for row in rows:
        rms, ref_rms = float(row[2]), float(row[6])
        assert rms <= 2e-5 and rms <= 1e-4 * ref_rms * 10  # measured ~4e-6 (fp32 path: ~4e-7)
    # the same utterances as one ragged batch: bitwise the B=1 waveforms, silence after each end
    ragged = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("ragged")]
    assert len(ragged) == 4
    for row in ragged:
        assert row[3] == "1" and float(row[5]) == 0.0, row


def test_precision_option_leaves_predictors_and_units_exact():
    """precision=1 is a generator-only mode: durations, f0 and unit indices feed integer decisions
    and must stay on the exact fp32 kernels (the predictor/HuBERT parity tests pass unchanged)."""
    import subprocess
    import sys
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DISSC_OPTIONS="precision=1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu",
                        os.path.join(root, "tests", "test_gpu_predictors.py"),
                        os.path.join(root, "tests", "test_gpu_hubert.py")],
                       env=env, capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_fused_residual_pairs_are_bit_identical_to_separate_launches(env):
    """respair.hip (one launch per residual pair of the narrow stages, direct form) against the same generator with
    every conv as its own launch ("pair_max_c" = 0): identical bits, for a ragged batch (window edges,
    utterance ends inside a window, a 1-frame utterance) and at the BASELINE size."""
    lib, synth = env["lib"], env["synth"]
    g = _generator_with(lib, synth, pair_f23=0)  # (the default's k = 11 pairs of the 32-channel stage are F(2,3): next test)
    cur = ctypes.c_int(0)
    assert lib.dissc_get_option(b"pair_max_c", ctypes.byref(cur)) == 0 and cur.value >= 16
    g_sep = _generator_with(lib, synth, pair_f23=0, pair_max_c=0)  # every conv its own launch
    for code, f0, spkr, lengths in _pair_cases(synth):
        kw = dict(code=torch.from_numpy(code), f0=torch.from_numpy(f0), spkr=torch.from_numpy(spkr),
                  lengths=torch.from_numpy(lengths))
        y_pair = g(**kw).cpu()
        y_sep = g_sep(**kw).cpu()
        assert torch.isfinite(y_pair).all()
        assert torch.equal(y_pair, y_sep)


def test_f23_pairs_agree_with_the_direct_pairs(env):
    """the default instance (k = 11 pairs of the 32- and 16-channel stages on respair32/16_f23_kernel: register-only F(2,3)) against one
    built with "pair_f23" = 0 (the direct pairs): same waveform to fp32 rounding, ragged (incl. long utterances) and at the
    BASELINE size, fewer executed FLOPs, batch-independent samples"""
    lib, synth = env["lib"], env["synth"]
    gd = _generator_with(lib, synth, pair_f23=0)
    g = env["g"]
    assert g.flops_executed(1000) < gd.flops_executed(1000) and g.flops(1000) == gd.flops(1000)
    for code, f0, spkr, lengths in _pair_cases(synth) + [synth.synth_generator_inputs(3, 1203, seed=5, ragged=True)]:
        kw = dict(code=torch.from_numpy(code), f0=torch.from_numpy(f0), spkr=torch.from_numpy(spkr),
                  lengths=torch.from_numpy(lengths))
        y, yd = g(**kw).cpu(), gd(**kw).cpu()
        assert torch.isfinite(y).all() and not torch.equal(y, yd)
        e = (y - yd).double()
        rms = float(e.pow(2).mean().sqrt())
        print(f"B={code.shape[0]} T={code.shape[1]}: F(2,3) pairs vs direct pairs: rms {rms:.2e}, max {float(e.abs().max()):.2e}")
        assert rms <= 2e-6 and float(e.abs().max()) <= 5e-5
        one = g(code=kw["code"][:1], f0=kw["f0"][:1], spkr=kw["spkr"][:1], lengths=kw["lengths"][:1]).cpu()[0]
        assert torch.equal(one, y[0])


@pytest.mark.parametrize("C,k,d", [(64, 7, 1), (64, 11, 5), (128, 7, 3), (128, 11, 1), (256, 7, 5), (256, 11, 3), (64, 11, 3), (128, 7, 5)])
def test_f63_f54_conv_matches_torch_and_the_f43_form(env, C, k, d):
    """conv_wino8.hip (the eight Toom-Cook points on 8-wave workgroups as F(6,3), "wino8" = 2, and as F(5,4) with 4-tap
    sub-filters, "wino8_r4" = 2) through dissc_conv1d: against a float64 F.conv1d with ragged lengths (tiles of 300-384
    outputs, so 315 / 316 / 629 / 631 straddle the F(5,4) tiles whose 315 outputs are not a whole number of quads) and NaN
    beyond every utterance, next to the F(4,3) form -- error at most 3x the direct kernel's rms; an utterance alone gives the
    same bits as inside the batch."""
    lib = env["lib"]
    torch.manual_seed(C + k + d)
    lens = [1000, 1, 7, 315, 316, 359, 360, 361, 629, 631, 767, 769, 997]
    x = torch.rand(len(lens), C, 1000) * 2 - 1
    w = (torch.rand(C, C, k) * 2 - 1) * 0.025 * (256 / C) ** 0.5
    b = torch.rand(C) * 0.2 - 0.1
    errs = {}
    try:
        for form, (wo, w8, r4) in {"direct": (0, 0, 0), "f43": (2, 0, 0), "f63": (1, 2, 0), "f54": (1, 2, 2)}.items():
            assert lib.dissc_set_option(b"wino", wo) == 0 and lib.dissc_set_option(b"wino8", w8) == 0
            assert lib.dissc_set_option(b"wino8_r4", r4) == 0
            y = _run_conv(env, x, w, b, lens, k, d, 0.1)
            e2 = n2 = 0.0
            for i, n in enumerate(lens):
                ref = F.conv1d(F.leaky_relu(x[i:i + 1, :, :n].double(), 0.1), w.double(), b.double(), padding=(k - 1) * d // 2,
                               dilation=d)[0]
                e = y[i, :, :n].double() - ref
                e2 += float((e ** 2).sum())
                n2 += e.numel()
            errs[form] = (e2 / n2) ** 0.5
            if form in ("f63", "f54"):
                for j in (3, 8):
                    one = _run_conv(env, x[j:j + 1, :, :lens[j]], w, b, lens[j:j + 1], k, d, 0.1)
                    assert torch.equal(one[0, :, :lens[j]], y[j, :, :lens[j]])
    finally:
        lib.dissc_set_option(b"wino", 1)
        lib.dissc_set_option(b"wino8", 1)
        lib.dissc_set_option(b"wino8_r4", 1)
    print(f"C={C} k={k} d={d}: rms error direct {errs['direct']:.2e}, F(4,3) {errs['f43']:.2e}, F(6,3) {errs['f63']:.2e}, "
          f"F(5,4) {errs['f54']:.2e}")
    assert errs["f63"] <= 3.0 * errs["direct"] + 1e-8 and errs["f54"] <= 3.0 * errs["direct"] + 1e-8
    assert errs["f54"] != errs["f63"]  # (the two forms really ran)


def test_eight_point_generators_agree_with_the_f43_generator(env):
    """the default instance (per shape: F(5,4), F(6,3) or F(4,3) -- conv_wino8.hip's masks), one with EVERY k = 7 / 11 layer
    of the C >= 64 stages as F(5,4) and one with all of them (and the k = 3 layers) as F(6,3), against an instance built with
    "wino8" = 0 (F(4,3) everywhere): same waveform to fp32 rounding, fewer executed FLOPs, batch-independent samples"""
    lib, synth = env["lib"], env["synth"]
    gd = _generator_with(lib, synth, wino8=0)
    assert env["g"].flops_executed(1000) < gd.flops_executed(1000)
    g6 = _generator_with(lib, synth, wino8=1, wino8_r4=0, wino8_mask=0o777777777)
    g5 = _generator_with(lib, synth, wino8=1, wino8_r4=1, wino8_mask=0o777777777, wino8_r4_mask=0o777777777)
    assert g5.flops_executed(1000) < g6.flops_executed(1000) < gd.flops_executed(1000)
    assert g5.flops_executed(1000) < env["g"].flops_executed(1000) and g5.flops(1000) == gd.flops(1000) == g6.flops(1000)
    # + three long ragged utterances (63 / 62.6 / ... frames x 320: tens of tiles per row at every stage, tile ends that are
    # not whole output quads, utterance ends inside a tile)
    long_case = synth.synth_generator_inputs(3, 1203, seed=5, ragged=True)
    for code, f0, spkr, lengths in _pair_cases(synth) + [long_case]:
        kw = dict(code=torch.from_numpy(code), f0=torch.from_numpy(f0), spkr=torch.from_numpy(spkr),
                  lengths=torch.from_numpy(lengths))
        yd = gd(**kw).cpu()
        y1 = env["g"](**kw).cpu()
        assert not torch.equal(y1, yd) and float((y1 - yd).double().pow(2).mean().sqrt()) <= 5e-6
        for name, g8 in (("F(6,3)", g6), ("F(5,4)", g5)):
            y8 = g8(**kw).cpu()
            assert torch.isfinite(y8).all() and not torch.equal(y8, yd) and not torch.equal(y8, y1)
            e = (y8 - yd).double()
            rms = float(e.pow(2).mean().sqrt())
            print(f"B={code.shape[0]} T={code.shape[1]}: {name} layers vs F(4,3): rms {rms:.2e}, max {float(e.abs().max()):.2e}")
            assert rms <= 5e-6 and float(e.abs().max()) <= 1e-4
            one = g8(code=kw["code"][:1], f0=kw["f0"][:1], spkr=kw["spkr"][:1], lengths=kw["lengths"][:1]).cpu()[0]
            assert torch.equal(one, y8[0])


def test_generator_random_dispatch_fuzz(env):
    """Which kernel a layer runs on depends on (B, T, lengths): per-shape form masks, small_grid tile step-downs, two-per-CU
    tiles, exists-only tile enumeration on ragged batches.  25 seeded cases -- B in [1, 40], T in [1, 700], ragged rows incl.
    0- and 1-frame utterances, NaN-free poison beyond every length -- of the DEFAULT generator against
    oracle.generator_ref.code_generator (reference sr/models.py:98-114) at <= 1e-4 RMS / 1e-3 of the reference's RMS on up to
    three utterances per case, nothing written beyond an utterance, and batch independence: an utterance decoded alone is
    bit-identical to its row of the batch (tools/wino_fuzz.py one level up)."""
    g, gr, synth = env["g"], env["gr"], env["synth"]
    rs = np.random.RandomState(2025)
    worst = 0.0
    for case in range(25):
        B = int(rs.choice([1, 2, 3, 5, 8, 13, 21, 32, 40]))
        T = int(rs.choice([1, 2, 7, 33, 64, 99, 128, 250, 257, 500, 511, 700]))
        if B * T > 14000:  # keep a case within ~0.5 s of GPU and a few seconds of oracle
            B = max(1, 14000 // T)
        code, f0, spkr, _ = synth.synth_generator_inputs(B, T, seed=4000 + case)
        mode = case % 3  # 0: uniform, 1: ragged, 2: ragged with empty / one-frame rows
        lengths = np.full(B, T, np.int32)
        if mode >= 1:
            lengths = rs.randint(1, T + 1, size=B).astype(np.int32)
            lengths[rs.randint(B)] = T
        if mode == 2 and B >= 3:
            lengths[rs.randint(B)] = 0
            lengths[rs.randint(B)] = 1
            lengths[rs.randint(B)] = T if (lengths == T).sum() == 0 else lengths[rs.randint(B)]
        code2, f02 = code.copy(), f0.copy()
        for b in range(B):
            code2[b, lengths[b]:] = 99
            f02[b, 0, lengths[b]:] = 1e9
        tc, tf, ts, tl = torch.from_numpy(code2), torch.from_numpy(f02), torch.from_numpy(spkr), torch.from_numpy(lengths)
        y = g(code=tc, f0=tf, spkr=ts, lengths=tl if mode else None).cpu()
        assert tuple(y.shape) == (B, 1, 320 * T) and torch.isfinite(y).all()
        for b in range(B):
            assert not y[b, :, 320 * int(lengths[b]):].any(), (case, b)
        live = [b for b in range(B) if lengths[b] > 0]
        for b in list(rs.choice(live, size=min(3, len(live)), replace=False)):
            n = int(lengths[b])
            ref = gr.code_generator(env["folded"], synth.VCTK_CONFIG, code[b:b + 1, :n], f0[b:b + 1, :, :n], spkr[b:b + 1])
            e = (y[b:b + 1, :, :320 * n] - ref).numpy()
            assert _rms(e) <= NORTH_STAR_RMS and _rms(e) <= 1e-3 * max(_rms(ref.numpy()), 1e-3), (case, B, T, b, n, _rms(e))
            assert _rms(e) <= FP32_GUARD_RMS, (case, B, T, b, n, _rms(e))
            worst = max(worst, _rms(e))
        for b in list(rs.choice(live, size=min(2, len(live)), replace=False)):
            n = int(lengths[b])
            y1 = g(code=tc[b:b + 1, :n], f0=tf[b:b + 1, :, :n], spkr=ts[b:b + 1]).cpu()
            assert torch.equal(y1[0, :, :320 * n], y[b, :, :320 * n]), (case, B, T, b, n)
    print(f"generator dispatch fuzz: 25 cases, worst RMS error vs the oracle {worst:.3e}")


def test_options_are_frozen_into_the_handle(env):
    """"re-entrant per handle, no global state".  Two generators created under different options -- every ResBlock
    conv direct ("wino" = 0, residual pairs as separate launches) and the default transform-domain build -- run INTERLEAVED, with
    dissc_set_option calls in between (the defaults of handles created later): each one's output is bit-identical to its solo
    run, and the two really are different code paths (they differ in the last bits)."""
    lib, synth = env["lib"], env["synth"]
    g_direct = _generator_with(lib, synth, wino=0, pair_max_c=0, multistream=0)
    g_default = env["g"]
    code, f0, spkr, lengths = synth.synth_generator_inputs(5, 90, seed=31, ragged=True)
    kw = dict(code=torch.from_numpy(code), f0=torch.from_numpy(f0), spkr=torch.from_numpy(spkr), lengths=torch.from_numpy(lengths))
    solo_direct, solo_default = g_direct(**kw).cpu(), g_default(**kw).cpu()
    assert not torch.equal(solo_direct, solo_default) and float((solo_direct - solo_default).abs().max()) <= 1e-4
    saved = {}
    try:
        for i, (k, v) in enumerate([("wino", 0), ("pair_max_c", 0), ("small_grid", 0), ("ragged_enum", 0), ("wino_sv", 0),
                                    ("wino8", 0), ("multistream", 0), ("pair_f23", 0)]):
            cur = ctypes.c_int(0)
            assert lib.dissc_get_option(k.encode(), ctypes.byref(cur)) == 0
            saved[k] = cur.value
            assert lib.dissc_set_option(k.encode(), v) == 0   # changes what handles created LATER do -- not these two
            a, b = (g_direct, g_default) if i % 2 == 0 else (g_default, g_direct)
            ya, yb = a(**kw).cpu(), b(**kw).cpu()
            assert torch.equal(ya, solo_direct if a is g_direct else solo_default), k
            assert torch.equal(yb, solo_direct if b is g_direct else solo_default), k
    finally:
        for k, v in saved.items():
            lib.dissc_set_option(k.encode(), v)


def test_parallel_weight_packing_is_bit_identical(env, monkeypatch):
    """dissc_gen_create packs the layers' weights on a few host threads (DISSC_PACK_THREADS, default 8): the handle must not
    depend on how many -- same waveform, bit for bit, from handles built with 1, 3 and 16 packing threads."""
    import dissc_amd
    synth = env["synth"]
    code, f0, spkr, _ = synth.synth_generator_inputs(3, 37, seed=21)
    kw = dict(code=torch.from_numpy(code), f0=torch.from_numpy(f0), spkr=torch.from_numpy(spkr))
    outs = []
    for n in ("1", "3", "16"):
        monkeypatch.setenv("DISSC_PACK_THREADS", n)
        g = dissc_amd.CodeGenerator(synth.VCTK_CONFIG).to("cuda:0")
        g.load_state_dict(synth.synth_generator_state_dict(seed=0))
        g.eval().remove_weight_norm()
        outs.append(g(**kw).cpu())
        del g
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert torch.equal(outs[0], env["g"](**kw).cpu())
