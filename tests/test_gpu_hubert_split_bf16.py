"""The HuBERT encoder's opt-in split-bf16 mode (HubertEncoder(..., precision="split_bf16"); csrc/enc_bf3.hip) on the GPU.

Yardsticks, all computed here on the CPU against the float64 oracle on the same input, none of them on the device:
  * the fp32 oracle's own error (what the fp32 kernels are allowed TAP_RATIO x of, tests/test_gpu_hubert_trained_like.py);
  * the CPU model of the mode (tests/split_bf16_model.py): its arithmetic with an exact accumulator, i.e. the error the mode is
    ALLOWED to have.  The device adds fp32 accumulation of three times as many partial products and its summation order:
    MODEL_FACTOR = 2 on the model's figure (the failure this must catch, a dropped cross term, is hundreds of times larger:
    tests/test_split_bf16_model_cpu.py).
Feature bar per layer and utterance:  MODEL_FACTOR x model + TAP_RATIO x fp32 oracle  (worst frame l2, and worst channel).
The direct kernel tests compare one layer against float64 ON THE SPLIT OPERANDS: identical products, fp32 against exact
accumulation -- KERNEL_RATIO = 4 x torch fp32's error on the same unsplit operation (the allowance of a single fp32 kernel,
LN_RATIO).  Run with -s for one line per case; DISSC_SPLIT_BF16_TABLE=<file> writes the per-layer table
(profiles/hubert_split_bf16_error.md is a copy of it)."""
import ctypes
import importlib.util
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TAP_RATIO = 8.0         # the allowance of the fp32 kernels, as a ratio to the fp32 oracle's own error
MODEL_FACTOR = 2.0      # margin on the CPU model's error: fp32 instead of exact accumulation, summation order
KERNEL_RATIO = 4.0      # one kernel against float64 on the same split operands, as a ratio to torch fp32's error
FLOOR = 2.0 ** -24
CH_FLOOR = 1e-3         # worst-channel figure: a channel's RMS is floored at this fraction of the layer's RMS
SENT = 12345.0
IID_UTTS = (("iid_32000", 32000, 719), ("iid_16000", 16000, 7))
TL_UTTS = (("speech_like", 32000, 31), ("speech_dc", 16000, 32), ("dither", 8000, 33))


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, rel))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _tap_errs(x, ref):
    """(worst frame l2 relative, worst channel RMS / max(channel RMS, CH_FLOOR x the layer's RMS)) -- the two definitions of
    tests/test_gpu_hubert_trained_like.py::_tap_errs"""
    d = np.asarray(x, np.float64) - ref
    fr = (np.linalg.norm(d, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-300)).max()
    rms = np.sqrt((ref ** 2).mean(0))
    ch = (np.sqrt((d ** 2).mean(0)) / np.maximum(rms, CH_FLOOR * np.sqrt((ref ** 2).mean()))).max()
    return float(fr), float(ch)


class _Env:
    """one checkpoint + centres, and the three CPU computations of an utterance (cached: several tests share them)"""

    def __init__(self, sd, centers):
        from oracle import hubert_ref as hr
        self.hr, self.sd, self.sd64, self.centers = hr, sd, hr.to_double(sd), torch.as_tensor(centers)
        self._cache = {}

    def refs(self, key, wav):
        """-> dict(t64, t32, tm: per-layer [T,768] float64 arrays; u64, u32, um: units)"""
        if key not in self._cache:
            import split_bf16_model as sm
            w = torch.as_tensor(wav)[None]
            t64, t32, tm = [], [], []
            u64, _ = self.hr.encode(self.sd64, self.centers, w, taps=t64)
            u32, _ = self.hr.encode(self.sd, self.centers, w, taps=t32)
            um, _ = sm.encode(self.sd, self.centers, w, taps=tm)
            self._cache[key] = dict(t64=[t[0].numpy() for t in t64], t32=[t[0].double().numpy() for t in t32],
                                    tm=[t[0].double().numpy() for t in tm], u64=u64.numpy(), u32=u32.numpy(), um=um.numpy())
        return self._cache[key]

    def bars(self, key, wav, layer):
        """(frame bar, channel bar, model figures, fp32 oracle figures) of one layer (1-based)"""
        r = self.refs(key, wav)
        fm, cm = _tap_errs(r["tm"][layer - 1], r["t64"][layer - 1])
        fo, co = _tap_errs(r["t32"][layer - 1], r["t64"][layer - 1])
        return (MODEL_FACTOR * fm + TAP_RATIO * max(fo, FLOOR), MODEL_FACTOR * cm + TAP_RATIO * max(co, FLOOR), (fm, cm), (fo, co))

    def encoder(self, n_layers=6, precision="split_bf16"):
        from dissc_amd.hubert import HubertEncoder
        return HubertEncoder(self.sd, self.centers, n_layers=n_layers, precision=precision).to("cuda:0")


@pytest.fixture(scope="module")
def envs(golden_dir):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import synthdata as synth
    g = np.load(os.path.join(golden_dir, "hubert_trainedlike.npz"))
    iid = _Env(synth.synth_hubert_state_dict(6), synth.synth_kmeans_centers())
    tl = _Env(synth.synth_hubert_state_dict(6, kind="trained_like"), torch.from_numpy(g["centers"]))
    utts = [(iid, name, synth.synth_waveform(n, seed=s)) for name, n, s in IID_UTTS]
    utts += [(tl, name, synth.synth_waveform(n, seed=s, kind=name)) for name, n, s in TL_UTTS]
    return dict(iid=iid, tl=tl, utts=utts, synth=synth)


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dissc_amd._lib import check, lib
    return lib, check


def _ragged_batch(synth):
    """the B = 32 ragged 2 .. 10 s trained-like batch of test_encoder_batch32_ragged_2_to_10s (same seeds), NaN padding"""
    rs = np.random.RandomState(12)
    ns = [160000] + [int(v) for v in rs.randint(32000, 160001, size=30)] + [32000]
    wav = torch.full((32, 160000), float("nan"))
    for i, n in enumerate(ns):
        wav[i, :n] = torch.from_numpy(synth.synth_waveform(n, seed=800 + i, kind="speech_dc" if i % 5 == 0 else "speech_like"))
    return wav, ns


# ---------------------------------------------------------------------------------------------------------------------------
# 1. features against float64
# ---------------------------------------------------------------------------------------------------------------------------
def test_per_layer_features_against_float64(envs):
    """handles of n_layers = 1 .. 6 in split-bf16 on the two iid and the three trained-like utterances: worst frame (l2,
    relative) and worst channel <= MODEL_FACTOR x the CPU model's figure + TAP_RATIO x the fp32 oracle's"""
    rows = []
    for env in (envs["iid"], envs["tl"]):
        for layer in range(1, 7):
            enc = env.encoder(layer)
            for e, name, w in envs["utts"]:
                if e is not env:
                    continue
                x = enc(torch.from_numpy(w)[None])["dense"][0].cpu().numpy()
                t64 = env.refs(name, w)["t64"][layer - 1]
                assert x.shape == t64.shape and np.isfinite(x).all(), (name, layer)
                bf, bc, (fm, cm), (fo, co) = env.bars(name, w, layer)
                fk, ck = _tap_errs(x, t64)
                rows.append((name, layer, fk, fm, fo, fk / bf, ck, cm, co, ck / bc))
                print(f"layer {layer} {name:12s}: frame l2 {fk:.2e} (model {fm:.2e}, fp32 oracle {fo:.2e}, bar {bf:.2e}, used"
                      f" {fk / bf:.2f})  channel {ck:.2e} (model {cm:.2e}, fp32 oracle {co:.2e}, bar {bc:.2e}, used {ck / bc:.2f})")
            del enc
    path = os.environ.get("DISSC_SPLIT_BF16_TABLE")
    if path:
        with open(path, "w") as f:
            f.write("| utterance | layer | frame l2: device | model | fp32 oracle | device / bar | channel: device | model | fp32 oracle |"
                    " device / bar |\n|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                f.write("| %s | %d | %.2e | %.2e | %.2e | %.2f | %.2e | %.2e | %.2e | %.2f |\n" % r)
    bad = [(r[0], r[1], round(r[5], 2), round(r[9], 2)) for r in rows if r[5] > 1.0 or r[9] > 1.0]
    assert not bad, f"(utterance, layer, frame / bar, channel / bar) above the bar: {bad}"


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the mode is really on, and only where asked
# ---------------------------------------------------------------------------------------------------------------------------
def _dense(enc, w):
    return enc(torch.from_numpy(w)[None])["dense"][0].cpu()


def test_mode_is_on_only_where_asked(envs, L):
    lib, _ = L
    env, (_, name, w) = envs["iid"], envs["utts"][0]
    t64 = env.refs(name, w)["t64"][5]
    split, fp32, default = env.encoder(6), env.encoder(6, "fp32"), env.encoder(6, None)
    ds, df, dd = _dense(split, w), _dense(fp32, w), _dense(default, w)
    assert lib.dissc_hubert_precision(split._handle) == 1
    assert lib.dissc_hubert_precision(fp32._handle) == 0 and lib.dissc_hubert_precision(default._handle) == 0
    assert torch.equal(df, dd)
    assert not torch.equal(ds, df)
    es, ef = _tap_errs(ds.numpy(), t64)[0], _tap_errs(df.numpy(), t64)[0]
    print(f"worst frame vs float64: split {es:.2e}, fp32 handle {ef:.2e} ({es / ef:.1f} x)")
    assert es > 2 * ef, (es, ef)
    # the process option: a default handle follows it, an explicit "fp32" does not
    try:
        assert lib.dissc_set_option(b"enc_precision", 1) == 0
        opt_default, opt_fp32 = env.encoder(6, None), env.encoder(6, "fp32")
        d1, d2 = _dense(opt_default, w), _dense(opt_fp32, w)
    finally:
        lib.dissc_set_option(b"enc_precision", 0)
    assert lib.dissc_hubert_precision(opt_default._handle) == 1 and torch.equal(d1, ds)
    assert lib.dissc_hubert_precision(opt_fp32._handle) == 0 and torch.equal(d2, df)
    assert torch.equal(_dense(opt_default, w), ds)  # frozen into the handle: the option is 0 again
    # the generator's option does not reach the encoder (a fresh process, as the existing option tests do)
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"dissc_split_bf16_{os.getpid()}.npy")
    code = ("import sys, numpy as np, torch; sys.path.insert(0, %r); import synthdata as synth\n"
            "from dissc_amd.hubert import HubertEncoder\n"
            "enc = HubertEncoder(synth.synth_hubert_state_dict(6), synth.synth_kmeans_centers(), n_layers=6).to('cuda:0')\n"
            "w = torch.from_numpy(synth.synth_waveform(%d, seed=%d))[None]\n"
            "np.save(%r, enc(w)['dense'][0].cpu().numpy())\n" % (ROOT, IID_UTTS[0][1], IID_UTTS[0][2], out))
    try:
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DISSC_OPTIONS="precision=1"), capture_output=True,
                           text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        np.testing.assert_array_equal(np.load(out), df.numpy())
    finally:
        if os.path.exists(out):
            os.remove(out)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. units
# ---------------------------------------------------------------------------------------------------------------------------
def _check_units_split(env, key, wav, units, dense):
    """every flip against the float64 oracle explained by the MEASURED feature error (which must be inside test 1's bar for
    this utterance), and flips <= 2 x the CPU model's + 2 (the rule _check_units_tl applies to the fp32 path)"""
    r = env.refs(key, wav)
    eps_rel = env.bars(key, wav, 6)[0]
    mism, amb = env.hr.check_units(units, r["u64"], r["t64"][5], env.centers.double(), x_dev=dense, tag=key, max_mismatch=None,
                                   eps_rel=eps_rel)
    fm, f32 = int((r["um"] != r["u64"]).sum()), int((r["u32"] != r["u64"]).sum())
    print(f"{key}: eps_rel {eps_rel:.2e}; flips vs float64: device {mism}, model {fm}, fp32 oracle {f32}, of {len(r['u64'])} frames"
          f" ({amb} ambiguous)")
    assert mism <= 2 * fm + 2, (key, mism, fm)


def test_units_on_fixture_utterances(envs):
    encs = {id(envs["iid"]): (envs["iid"].encoder(6), envs["iid"].encoder(6, "fp32")), id(envs["tl"]): (envs["tl"].encoder(6), None)}
    for env, name, w in envs["utts"]:
        split, fp32 = encs[id(env)]
        out = split(torch.from_numpy(w)[None])
        units = out["units"][0].cpu().numpy()
        _check_units_split(env, name, w, units, out["dense"][0].cpu().numpy())
        if fp32 is not None:  # the goldens' rule: at most 1 unit per utterance away from the fp32 handle's
            uf = fp32(torch.from_numpy(w)[None])["units"][0].cpu().numpy()
            assert int((units != uf).sum()) <= 1, (name, int((units != uf).sum()))


def test_units_on_the_ragged_batch(envs):
    env = envs["tl"]
    wav, ns = _ragged_batch(envs["synth"])
    out = env.encoder(6)(wav, n_samples=torch.tensor(ns))
    units, dense = out["units"].cpu().numpy(), out["dense"].cpu().numpy()
    order = np.argsort(ns)
    for i in (0, 31, int(order[10]), int(order[21])):
        T = env.hr.num_frames(ns[i])
        assert int(out["frames"][i]) == T
        _check_units_split(env, f"ragged utt {i} ({ns[i]} samples)", wav[i, :ns[i]].numpy(), units[i, :T], dense[i, :T])


# ---------------------------------------------------------------------------------------------------------------------------
# 4. ragged batches: the guarantees of the fp32 path, for the new kernels
# ---------------------------------------------------------------------------------------------------------------------------
def test_ragged_batch_is_bitwise_batch_independent(envs, L):
    lib, _ = L
    env = envs["tl"]
    wav, ns = _ragged_batch(envs["synth"])
    enc = env.encoder(6)
    out = enc(wav, n_samples=torch.tensor(ns))
    units, dense = out["units"].cpu().numpy(), out["dense"].cpu().numpy()
    assert np.isfinite(np.concatenate([dense[i, :int(out["frames"][i])].ravel() for i in range(32)])).all()
    for i in range(32):
        T = int(out["frames"][i])
        one = enc(wav[i:i + 1, :ns[i]])
        np.testing.assert_array_equal(one["units"][0].cpu().numpy(), units[i, :T])
        np.testing.assert_array_equal(one["dense"][0].cpu().numpy(), dense[i, :T])
    outs = []
    try:
        for mode in (0, 2, 4, 1):
            assert lib.dissc_set_option(b"hubert_split", mode) == 0
            e = env.encoder(6)
            o = e(wav, n_samples=torch.tensor(ns))
            outs.append((o["units"].cpu(), o["dense"].cpu()))
            del e
    finally:
        lib.dissc_set_option(b"hubert_split", 1)
    for u, d in outs:
        for i in range(32):
            T = int(out["frames"][i])
            assert np.array_equal(u[i, :T].numpy(), units[i, :T]) and np.array_equal(d[i, :T].numpy(), dense[i, :T]), i


# ---------------------------------------------------------------------------------------------------------------------------
# 5. tile boundaries of the new kernels, directly
# ---------------------------------------------------------------------------------------------------------------------------
def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / np.sqrt(2.0)))


def _frame_errs(y, ref):
    """y, ref [C, T] -> per frame l2 relative"""
    d = y.double() - ref
    return d.norm(dim=0) / ref.norm(dim=0).clamp_min(1e-300)


def _assert_kernel_bar(tag, ek, et):
    ratio = ek / max(et, FLOOR)
    print(f"{tag}: kernel {ek:.2e} vs float64 on the split operands, torch fp32 {et:.2e} vs float64, ratio {ratio:.2f} (bar {KERNEL_RATIO})")
    assert ratio <= KERNEL_RATIO, (tag, ek, et, ratio)


def _with_small_grid(lib, value, fn):
    cur = ctypes.c_int(0)
    assert lib.dissc_get_option(b"small_grid", ctypes.byref(cur)) == 0
    try:
        assert lib.dissc_set_option(b"small_grid", value) == 0
        return fn()
    finally:
        lib.dissc_set_option(b"small_grid", cur.value)


S2_LMAX = [3, 4, 5, 255, 256, 257, 513, 1023, 31999]


@pytest.mark.parametrize("small_grid", [1, 0])  # 1: short rows step down to 64 x 128 tiles; 0: 256 x 128 tiles everywhere
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("k", [3, 2])
def test_stride2_conv_tile_boundaries(L, k, act, small_grid):
    """dissc_conv1d_s2_prec(prec = 1): 512 -> 512 channels, ragged lengths including 0 and < k, NaN beyond every length;
    sentinel-filled output outside [0, len_out) untouched"""
    import torch.nn.functional as F
    import split_bf16_model as sm
    lib, check = L
    rs = np.random.RandomState(100 * k + act)
    C = 512
    w = torch.from_numpy((rs.standard_normal((C, C, k)) / np.sqrt(C * k)).astype(np.float32))
    for Lmax in S2_LMAX:
        lens = [Lmax, 0, k - 1, max(k, Lmax // 2 + 1), max(k, Lmax - 1)]
        if Lmax == 31999:
            lens = [Lmax, 0, 17001]  # (the float64 reference of 5 such rows would take minutes)
        B, ldx = len(lens), (Lmax + 3) // 4 * 4
        Lo = (Lmax - k) // 2 + 1
        ldo = (Lo + 3) // 4 * 4
        x = torch.full((B, C, ldx), float("nan"))
        for b, n in enumerate(lens):
            x[b, :, :n] = torch.from_numpy((rs.standard_normal((C, n)) * np.exp(rs.standard_normal((C, 1)))).astype(np.float32))
        xd, ld = x.cuda(), torch.tensor(lens, dtype=torch.int32).cuda()
        y = torch.full((B, C, ldo), SENT, dtype=torch.float32, device="cuda")
        _with_small_grid(lib, small_grid, lambda: check(lib.dissc_conv1d_s2_prec(
            xd.data_ptr(), w.data_ptr(), None, y.data_ptr(), ld.data_ptr(), B, C, C, k, ldx, ldo, Lmax, act, 1, None),
            "dissc_conv1d_s2_prec"))
        y = y.cpu()
        ek = et = 0.0
        for b, n in enumerate(lens):
            lo = (n - k) // 2 + 1 if n >= k else 0
            assert (y[b, :, lo:] == SENT).all(), f"k={k} Lmax={Lmax} utterance {b}: output beyond its length written"
            if lo == 0:
                continue
            xb = x[b:b + 1, :, :n]
            ref, r64, r32 = sm.conv1d_s2_ref(xb, w)[0], F.conv1d(xb.double(), w.double(), stride=2)[0], F.conv1d(xb, w, stride=2)[0]
            if act:
                ref, r64, r32 = _gelu64(ref), _gelu64(r64), F.gelu(r32)
            assert torch.isfinite(y[b, :, :lo]).all()
            ek = max(ek, float(_frame_errs(y[b, :, :lo], ref).max()))
            et = max(et, float(_frame_errs(r32, r64).max()))
        _assert_kernel_bar(f"stride-2 k={k} act={act} small_grid={small_grid} Lmax_in={Lmax}", ek, et)


LIN_TS = [1, 63, 64, 65, 127, 129, 499]


@pytest.mark.parametrize("small_grid", [1, 0])
@pytest.mark.parametrize("epi", ["bias", "gelu", "residual"])
@pytest.mark.parametrize("K,M", [(512, 768), (768, 2304), (3072, 768)])
def test_linear_tile_boundaries(L, K, M, epi, small_grid):
    """dissc_linear_prec(prec = 1): one ragged batch with T = 1 .. 499 (+ an empty utterance), NaN beyond every length"""
    import torch.nn.functional as F
    import split_bf16_model as sm
    lib, check = L
    rs = np.random.RandomState(K + len(epi))
    lens = LIN_TS + [0]
    B, ld = len(lens), 500
    w = torch.from_numpy((rs.standard_normal((M, K)) / np.sqrt(K)).astype(np.float32))
    bias = torch.from_numpy(rs.standard_normal(M).astype(np.float32))
    x = torch.full((B, K, ld), float("nan"))
    res = torch.full((B, M, ld), float("nan"))
    for b, n in enumerate(lens):
        x[b, :, :n] = torch.from_numpy((rs.standard_normal((K, n)) * np.exp(rs.standard_normal((K, 1)))).astype(np.float32))
        res[b, :, :n] = torch.from_numpy(rs.standard_normal((M, n)).astype(np.float32))
    xd, rd, ldv = x.cuda(), res.cuda(), torch.tensor(lens, dtype=torch.int32).cuda()
    y = torch.full((B, M, ld), SENT, dtype=torch.float32, device="cuda")
    _with_small_grid(lib, small_grid, lambda: check(lib.dissc_linear_prec(
        xd.data_ptr(), w.data_ptr(), bias.data_ptr(), rd.data_ptr() if epi == "residual" else None, y.data_ptr(), ldv.data_ptr(),
        B, K, M, ld, max(lens), 1 if epi == "gelu" else 0, 1, None), "dissc_linear_prec"))
    y = y.cpu()
    for b, n in enumerate(lens):
        assert (y[b, :, n:] == SENT).all(), f"T={n}: output beyond the length written"
        if n == 0:
            continue
        xb = x[b, :, :n].t()
        ref, r64, r32 = sm.linear_ref(xb, w, bias).t(), F.linear(xb.double(), w.double(), bias.double()).t(), F.linear(xb, w, bias).t()
        if epi == "gelu":
            ref, r64, r32 = _gelu64(ref), _gelu64(r64), F.gelu(r32)
        if epi == "residual":
            ref, r64, r32 = ref + res[b, :, :n].double(), r64 + res[b, :, :n].double(), r32 + res[b, :, :n]
        assert torch.isfinite(y[b, :, :n]).all()
        _assert_kernel_bar(f"linear K={K} M={M} {epi} small_grid={small_grid} T={n}", float(_frame_errs(y[b, :, :n], ref).max()),
                           float(_frame_errs(r32, r64).max()))


def test_diagnostic_entries_refuse_what_the_kernel_does_not_take(L):
    lib, _ = L
    x = torch.zeros(1, 32, 8, device="cuda")
    y = torch.zeros(1, 32, 8, device="cuda")
    w = torch.zeros(32, 32, 3)
    assert lib.dissc_conv1d_s2_prec(x.data_ptr(), w.data_ptr(), None, y.data_ptr(), None, 1, 32, 32, 3, 8, 8, 8, 0, 1, None) != 0  # < 64 rows
    assert lib.dissc_conv1d_s2_prec(x.data_ptr(), w.data_ptr(), None, y.data_ptr(), None, 1, 32, 32, 3, 8, 8, 8, 0, 2, None) != 0  # prec
    assert lib.dissc_linear_prec(x.data_ptr(), w.data_ptr(), None, None, y.data_ptr(), None, 1, 32, 32, 8, 8, 0, 1, None) != 0


# ---------------------------------------------------------------------------------------------------------------------------
# 6. command line and the whole conversion
# ---------------------------------------------------------------------------------------------------------------------------
def test_encode_cli_precision_flag(envs, golden_dir, tmp_path):
    """data/encode.py --precision split_bf16 on the CLI fixture of tests/test_gpu_cli.py: at most 1 unit per utterance away
    from the fp32 run's manifest"""
    td = str(tmp_path)
    os.makedirs(f"{td}/ckpt")
    os.makedirs(f"{td}/wav")
    torch.save({"model": envs["iid"].sd}, f"{td}/ckpt/hubert-base-ls960.pt")
    np.save(f"{td}/ckpt/kmeans_100.npy", envs["iid"].centers.numpy())
    for i in (1, 2):
        shutil.copy(os.path.join(golden_dir, f"s1_{i}.wav"), f"{td}/wav/s1_{i}.wav")
    cli = _load("dissc_encode_cli_split", "data/encode.py")
    base = ["--base_dir", f"{td}/wav", "--checkpoint_dir", f"{td}/ckpt", "--f0", "zeros"]
    cli.main(base + ["--out_file", f"{td}/fp32.txt"])
    cli.main(base + ["--out_file", f"{td}/split.txt", "--precision", "split_bf16"])
    a, b = ({d["audio"]: d for d in map(json.loads, open(f"{td}/{fn}.txt").read().strip().split("\n"))} for fn in ("fp32", "split"))
    assert sorted(a) == sorted(b) == ["s1_1.wav", "s1_2.wav"]
    for name in a:
        ua, ub = np.array(a[name]["units"]), np.array(b[name]["units"])
        assert ua.shape == ub.shape == (99,)
        assert int((ua != ub).sum()) <= 1, (name, int((ua != ub).sum()))


def test_converter_with_split_encoder_and_generator_runs_cfg2(envs):
    """8 x 10 s through encode -> predictors (fp32) -> generator, encoder and generator both split-bf16: finite waveforms of
    320 samples per predicted frame"""
    import dissc_amd
    from dissc_amd import predictors as P
    from dissc_amd.pipeline import Converter
    synth = envs["synth"]
    enc = envs["iid"].encoder(6)
    lm = P.LenPredictor(100, 108).to("cuda:0")
    lm.load_state_dict(synth.synth_len_state_dict(100, 108))
    lm.norm_mean, lm.norm_std = synth.synth_len_norm_stats()
    pm = P.PitchPredictor(100, 108).to("cuda:0")
    pm.load_state_dict(synth.synth_pitch_state_dict("new", 100, 108))
    g = dissc_amd.CodeGenerator(synth.VCTK_CONFIG, precision="split_bf16").to("cuda:0")
    g.load_state_dict(synth.synth_generator_state_dict(seed=0))
    g.eval().remove_weight_norm()
    tgt = 6
    waves = [synth.synth_waveform(160000, seed=100 + i) for i in range(8)]
    raw = Converter(enc, lm, pm, g, postprocess=False)(waves, [tgt])
    assert sorted(raw) == [(i, tgt) for i in range(8)]
    units = enc(torch.from_numpy(np.stack(waves)), want_dense=False)["units"].cpu()
    assert units.shape == (8, 499)
    for i in range(8):
        hu, _, _ = P.infer_samples([units[i]], [tgt], lm, pm, norm_pitch=True, device="cuda:0")[0]
        r = raw[(i, tgt)]
        assert r.shape == (320 * len(hu),) and r.size > 0 and np.isfinite(r).all(), i
