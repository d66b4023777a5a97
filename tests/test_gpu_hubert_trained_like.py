"""The HuBERT encoder on trained-like weights and inputs (synthdata kind="trained_like" / "speech_like"), against float64.

Every error is measured against a float64 computation on the same fp32 inputs, and every bar is a RATIO to the error of the
fp32 CPU computation of the same operation (torch fp32, or the fp32 oracle), so a bar holds on any conditioning.  The direct
kernel tests feed the fused attention (csrc/attn.hip) and the channels-first LayerNorm (csrc/hubert.hip ln_cf_kernel) through
their diagnostic entries, dissc_attention / dissc_layernorm_cf; the encoder tests tap every layer (handles of n_layers = 1..6)
and check the units against the float64 oracle's.  Run with -s for one line per case; the measured table is
profiles/hubert_trained_like_error.md."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# Bars: ratio of the kernel's error to the fp32 CPU computation's own error (ceilings; profiles/hubert_trained_like_error.md)
ATTN_RATIO = 6.0        # per (utterance, head): max over queries of the l2 relative error of the output row
LN_RATIO = 4.0          # per row kind: max over rows of the l2 relative error of the normalised row
TAP_RATIO = 8.0         # per layer and utterance: worst frame (l2, relative) and worst channel (RMS / RMS, floored)
FLOOR = 2.0 ** -24      # denominators of the ratios are floored here: an fp32 computation that happens to be exact
CH_FLOOR = 1e-3         # worst-channel figure: a channel's RMS is floored at this fraction of the layer's RMS
SENT = 12345.0


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def lib():
    _need_gpu()
    from dissc_amd._lib import check, lib
    return lib, check


# ---------------------------------------------------------------------------------------------------------------------------
# fused attention, direct
# ---------------------------------------------------------------------------------------------------------------------------
ATT_TS = [1, 2, 63, 64, 65, 127, 128, 129, 499]
ATT_SCALES = [1.0, 10.0, 30.0, 80.0]     # one head each: the largest |logit| of a row


def _attention_case(seed=0):
    """qkv [B][3D][ld] with NaN beyond every length: utterance i of ATT_TS has one dominant key, placed in key tile 0, 1, 2 or the
    last (the partly masked one) by turns; two more utterances of T = 499: all keys equal, and logits that grow with the key
    index (the running maximum changes in every tile: a rescale per tile).  Head h: logits of size ATT_SCALES[h]."""
    rs = np.random.RandomState(seed)
    H, D = len(ATT_SCALES), 64 * len(ATT_SCALES)
    Ts = ATT_TS + [499, 499]
    B, ld = len(Ts), 500
    qkv = np.full((B, 3 * D, ld), np.nan, np.float64)
    kinds = []
    for b, T in enumerate(Ts):
        kind = "equal" if b == len(ATT_TS) else "growing" if b == len(ATT_TS) + 1 else f"tile{('0', '1', '2', 'last')[b % 4]}"
        kinds.append(kind)
        for h, sc in enumerate(ATT_SCALES):
            u = rs.standard_normal(64)
            u /= np.linalg.norm(u)
            q = u[:, None] + 0.3 * rs.standard_normal((64, T)) / 8.0           # queries share a direction u
            k = rs.standard_normal((64, T)) / 8.0 * (sc / 3.0)                 # background logits ~ sc / 3
            if kind == "equal":
                k[:] = (sc * u)[:, None]
            elif kind == "growing":
                k = u[:, None] * (sc * np.arange(1, T + 1) / T)[None, :] + 0.1 * k
            else:
                n_tiles = (T + 63) // 64
                tile = {"tile0": 0, "tile1": 1, "tile2": 2, "tilelast": n_tiles - 1}[kind]
                tile = min(tile, n_tiles - 1)
                j = min(64 * tile + rs.randint(0, 64), T - 1)
                k[:, j] = sc * u
            qkv[b, h * 64:(h + 1) * 64, :T] = q
            qkv[b, D + h * 64:D + (h + 1) * 64, :T] = k
            qkv[b, 2 * D + h * 64:2 * D + (h + 1) * 64, :T] = rs.standard_normal((64, T))
    return qkv.astype(np.float32), np.array(Ts, np.int32), kinds, H, D, ld


def _attention_ref(qkv, Ts, H, D, dtype):
    """softmax(Q^T K) V per (utterance, head) in ``dtype`` -> list of [B] arrays [D, T] (float64)"""
    out = []
    for b, T in enumerate(Ts):
        x = torch.from_numpy(qkv[b, :, :T]).to(dtype)
        o = torch.empty(D, T, dtype=torch.float64)
        for h in range(H):
            q, k, v = (x[i * D + h * 64:i * D + (h + 1) * 64] for i in range(3))
            p = torch.softmax(q.t() @ k, dim=-1)                               # [Tq, Tk]
            o[h * 64:(h + 1) * 64] = (v @ p.t()).double()
        out.append(o.numpy())
    return out


def _row_err(got, ref):
    """[D, T] -> per (head, query): ||got - ref||_2 / ||ref||_2 over the head's 64 outputs -> [H, T]"""
    D, T = ref.shape
    d = (got.astype(np.float64) - ref).reshape(D // 64, 64, T)
    r = ref.reshape(D // 64, 64, T)
    return np.linalg.norm(d, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-300)


@pytest.mark.parametrize("xcd", [11, 3])
def test_attention_direct_against_float64(lib, xcd):
    """csrc/attn.hip on constructed Q / K / V: logit scales 1 .. 80, the dominant key in key tiles 0 / 1 / 2 / the last (partly
    masked), equal keys, a running maximum that grows in every tile; T = 1 .. 499 in one ragged batch, NaN beyond every length;
    both grid orders (xcd_order bit 3).  Per (utterance, head): the worst query's error <= ATTN_RATIO x torch fp32's, finite,
    and the output beyond T untouched."""
    L, check = lib
    qkv, Ts, kinds, H, D, ld = _attention_case()
    B = len(Ts)
    r64 = _attention_ref(qkv, Ts, H, D, torch.float64)
    r32 = _attention_ref(qkv, Ts, H, D, torch.float32)
    x = torch.from_numpy(qkv).cuda()
    lens = torch.from_numpy(Ts).cuda()
    out = torch.full((B, D, ld), SENT, dtype=torch.float32, device="cuda")
    try:
        assert L.dissc_set_option(b"xcd_order", xcd) == 0
        check(L.dissc_attention(x.data_ptr(), lens.data_ptr(), B, int(Ts.max()), D, ld, out.data_ptr(), None), "dissc_attention")
        torch.cuda.synchronize()
    finally:
        L.dissc_set_option(b"xcd_order", 11)
    o = out.cpu().numpy()
    worst = 0.0
    for b, T in enumerate(Ts):
        got = o[b, :, :T]
        assert np.isfinite(got).all(), (b, T)
        assert (o[b, :, T:] == SENT).all(), f"T={T}: output beyond the length written"
        ek, et = _row_err(got, r64[b]), _row_err(r32[b], r64[b])
        for h, sc in enumerate(ATT_SCALES):
            ratio = ek[h].max() / max(et[h].max(), FLOOR)
            worst = max(worst, ratio)
            print(f"attention xcd={xcd} T={T:3d} {kinds[b]:8s} logit {sc:4.0f}: kernel {ek[h].max():.2e} torch fp32 {et[h].max():.2e}"
                  f" ratio {ratio:.2f}")
            assert ratio <= ATTN_RATIO, (T, kinds[b], sc, ratio)
    print(f"attention xcd={xcd}: worst ratio {worst:.2f} (bar {ATTN_RATIO})")


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm, direct
# ---------------------------------------------------------------------------------------------------------------------------
LN_KINDS = ("massive", "offset", "constant", "tiny_std", "plain")


def _ln_case(C, seed=0):
    """x [B][C][ld], column t of utterance b is a row of kind LN_KINDS[t % 5]: N(0,1) with 4 channels at +-1e3 (one of them channel
    0, C/2 or C-1 in three rows of four); a common offset
    of 1e3 .. 1e4 with std 1; a constant row; std ~ sqrt(eps); plain N(0,1).  Ragged lengths, NaN beyond them."""
    rs = np.random.RandomState(seed + C)
    lens = np.array([200, 137, 1, 64], np.int32)
    B, ld = len(lens), 200
    x = np.full((B, C, ld), np.nan, np.float32)
    for b, T in enumerate(lens):
        for t in range(T):
            kind = LN_KINDS[t % 5]
            if kind == "massive":
                r = rs.standard_normal(C)
                idx = rs.choice(np.arange(1, C), 4, replace=False)
                idx[0] = (0, C // 2, C - 1, idx[0])[(t // 5) % 4]    # the LayerNorm's pivot candidates among the massive channels
                r[idx] = 1e3 * rs.choice([-1.0, 1.0], 4) * (1 + rs.rand(4))
            elif kind == "offset":
                r = 10.0 ** rs.uniform(3, 4) + rs.standard_normal(C)
            elif kind == "constant":
                r = np.full(C, 10.0 ** rs.uniform(-2, 4) * rs.choice([-1.0, 1.0]))
            elif kind == "tiny_std":
                r = rs.standard_normal() + np.sqrt(1e-5) * rs.uniform(0.3, 3) * rs.standard_normal(C)
            else:
                r = rs.standard_normal(C)
            x[b, :, t] = r
    gamma = np.exp(0.5 * rs.standard_normal(C)).astype(np.float32)
    gamma[:3] = [1e-3, 30.0, 1.0]
    beta = rs.standard_normal(C).astype(np.float32)
    return x, gamma, beta, lens, ld


@pytest.mark.parametrize("C", [512, 768])
def test_layernorm_direct_against_float64(lib, C):
    """ln_cf_kernel on rows where a two-pass fp32 LayerNorm can go wrong: per row kind, the worst row's error of the normalised
    row (y - beta, l2 relative) <= LN_RATIO x torch fp32 F.layer_norm's; constant rows give beta exactly; ragged lengths with
    NaN padding, nothing written beyond a length."""
    import torch.nn.functional as F
    L, check = lib
    x, gamma, beta, lens, ld = _ln_case(C)
    B = len(lens)
    xd = torch.from_numpy(x).cuda()
    g, bt, ln = (torch.from_numpy(a).cuda() for a in (gamma, beta, lens))
    y = torch.full((B, C, ld), SENT, dtype=torch.float32, device="cuda")
    check(L.dissc_layernorm_cf(xd.data_ptr(), g.data_ptr(), bt.data_ptr(), ln.data_ptr(), B, C, ld, 1e-5, y.data_ptr(), None),
          "dissc_layernorm_cf")
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    errs = {k: ([], []) for k in LN_KINDS}
    for b, T in enumerate(lens):
        assert (y[b, :, T:] == SENT).all(), f"utterance {b}: output beyond the length written"
        rows = torch.from_numpy(x[b, :, :T].T.copy())
        r64 = F.layer_norm(rows.double(), (C,), torch.from_numpy(gamma).double(), torch.from_numpy(beta).double(), 1e-5).numpy()
        r32 = F.layer_norm(rows, (C,), torch.from_numpy(gamma), torch.from_numpy(beta), 1e-5).double().numpy()
        got = y[b, :, :T].T.astype(np.float64)
        assert np.isfinite(got).all()
        n64 = r64 - beta
        for t in range(T):
            kind = LN_KINDS[t % 5]
            if kind == "constant":
                np.testing.assert_array_equal(y[b, :, t], beta, err_msg=f"constant row {t} of utterance {b}: y != beta")
                continue
            den = max(np.linalg.norm(n64[t]), 1e-300)
            errs[kind][0].append(np.linalg.norm(got[t] - r64[t]) / den)
            errs[kind][1].append(np.linalg.norm(r32[t] - r64[t]) / den)
    for kind, (ek, et) in errs.items():
        if not ek:
            continue
        ratio = max(ek) / max(max(et), FLOOR)
        print(f"layernorm C={C} {kind:8s}: kernel {max(ek):.2e} torch fp32 {max(et):.2e} ratio {ratio:.2f} (bar {LN_RATIO})")
        assert ratio <= LN_RATIO, (C, kind, ratio)


# ---------------------------------------------------------------------------------------------------------------------------
# the encoder: per-layer taps, units
# ---------------------------------------------------------------------------------------------------------------------------
FIXTURE_UTTS = (("speech_like", 32000, 31), ("speech_dc", 16000, 32), ("dither", 8000, 33))


def _edge_waves():
    import synthdata as synth
    w = {f"{k}_{n}": synth.synth_waveform(n, seed=s, kind=k) for k, n, s in FIXTURE_UTTS}
    w["zeros_400"] = np.zeros(400, np.float32)
    w["zeros_4000"] = np.zeros(4000, np.float32)
    clip = np.clip(np.round(synth.synth_waveform(24000, seed=34, kind="speech_like").astype(np.float64) * 32768 * 60), -32767, 32767)
    w["clipped_24000"] = (clip / 32768).astype(np.float32)
    return w


@pytest.fixture(scope="module")
def tl(golden_dir):
    _need_gpu()
    import synthdata as synth
    from oracle import hubert_ref as hr
    g = np.load(os.path.join(golden_dir, "hubert_trainedlike.npz"))
    sd = synth.synth_hubert_state_dict(6, kind="trained_like")
    centers = torch.from_numpy(g["centers"])
    return dict(hr=hr, synth=synth, sd=sd, sd64=hr.to_double(sd), centers=centers, g=g)


def _oracles(tl, wav):
    """float64 and fp32 oracle on one utterance: (taps64, taps32, units64, units32), taps [T, 768] per layer"""
    hr = tl["hr"]
    t64, t32 = [], []
    u64, _ = hr.encode(tl["sd64"], tl["centers"], torch.from_numpy(wav)[None], taps=t64)
    u32, _ = hr.encode(tl["sd"], tl["centers"], torch.from_numpy(wav)[None], taps=t32)
    return [t[0].numpy() for t in t64], [t[0].double().numpy() for t in t32], u64.numpy(), u32.numpy()


def _tap_errs(x, ref):
    """(worst frame l2 relative, worst channel RMS / max(channel RMS, CH_FLOOR x the layer's RMS))"""
    d = x.astype(np.float64) - ref
    fr = (np.linalg.norm(d, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-300)).max()
    rms = np.sqrt((ref ** 2).mean(0))
    ch = (np.sqrt((d ** 2).mean(0)) / np.maximum(rms, CH_FLOOR * np.sqrt((ref ** 2).mean()))).max()
    return fr, ch


def test_per_layer_taps_against_float64(tl):
    """Handles of n_layers = 1..6 on the fixture's utterances and the edge waveforms (all-zero n = 400 / 4000, DC offset,
    1-LSB dither, clipping): per layer, the worst frame's l2 relative error and the worst channel's RMS error (over the channel's
    RMS, floored) <= TAP_RATIO x the fp32 oracle's own figure."""
    from dissc_amd.hubert import HubertEncoder
    waves = _edge_waves()
    ref = {name: _oracles(tl, w) for name, w in waves.items()}
    worst = {}
    for L in range(1, 7):
        enc = HubertEncoder(tl["sd"], tl["centers"], n_layers=L).to("cuda:0")
        for name, w in waves.items():
            out = enc(torch.from_numpy(w)[None])
            x = out["dense"][0].cpu().numpy()
            t64, t32 = ref[name][0][L - 1], ref[name][1][L - 1]
            assert x.shape == t64.shape and np.isfinite(x).all(), (name, L)
            fk, ck = _tap_errs(x, t64)
            fo, co = _tap_errs(t32, t64)
            rf, rc = fk / max(fo, FLOOR), ck / max(co, FLOOR)
            worst[L] = max(worst.get(L, 0.0), rf, rc)
            print(f"layer {L} {name:18s}: frame l2 {fk:.2e} (fp32 oracle {fo:.2e}, ratio {rf:.2f})  channel {ck:.2e}"
                  f" (fp32 oracle {co:.2e}, ratio {rc:.2f})")
            assert rf <= TAP_RATIO and rc <= TAP_RATIO, (name, L, rf, rc)
        del enc
    print("per-layer worst ratio:", {L: round(v, 2) for L, v in worst.items()}, f"(bar {TAP_RATIO})")


def _check_units_tl(hr, units, u64, u32, d64, d32, centers, dense, tag):
    """every flip against the float64 oracle explicable by the measured feature error; flips <= 2 x the fp32 oracle's + 2.
    eps_rel: TAP_RATIO x the fp32 oracle's own worst per-frame error (floored at 1e-7), printed"""
    e32 = float((np.linalg.norm(d32 - d64, axis=1) / np.linalg.norm(d64, axis=1)).max())
    eps_rel = TAP_RATIO * max(e32, 1e-7)
    mism, amb = hr.check_units(units, u64, d64, centers, x_dev=dense, tag=tag, max_mismatch=None, eps_rel=eps_rel)
    f32 = int((u32 != u64).sum())
    print(f"{tag}: eps_rel {eps_rel:.2e}; flips: device {mism}, fp32 oracle {f32}, of {len(u64)} frames ({amb} ambiguous)")
    assert mism <= 2 * f32 + 2, (tag, mism, f32)


def test_encoder_units_on_fixture_utterances(tl):
    """the whole 6-layer encoder with the fixture's centres on the fixture's utterances and the edge waveforms"""
    from dissc_amd.hubert import HubertEncoder
    hr = tl["hr"]
    enc = HubertEncoder(tl["sd"], tl["centers"], n_layers=6).to("cuda:0")
    for name, w in _edge_waves().items():
        t64, t32, u64, u32 = _oracles(tl, w)
        out = enc(torch.from_numpy(w)[None])
        _check_units_tl(hr, out["units"][0].cpu().numpy(), u64, u32, t64[5], t32[5], tl["centers"].double(),
                        out["dense"][0].cpu().numpy(), name)


def test_encoder_batch32_ragged_2_to_10s(tl):
    """B = 32 ragged 2 .. 10 s speech-like batch, NaN padding: 4 utterances against the float64 oracle, B = 1 bit-identity of the
    units and dense features on all 32, and every hubert_split mode bitwise equal on this batch"""
    from dissc_amd import _lib
    from dissc_amd.hubert import HubertEncoder
    hr, synth = tl["hr"], tl["synth"]
    rs = np.random.RandomState(12)
    ns = [160000] + [int(v) for v in rs.randint(32000, 160001, size=30)] + [32000]
    wav = torch.full((32, 160000), float("nan"))
    for i, n in enumerate(ns):
        wav[i, :n] = torch.from_numpy(synth.synth_waveform(n, seed=800 + i, kind="speech_dc" if i % 5 == 0 else "speech_like"))
    enc = HubertEncoder(tl["sd"], tl["centers"], n_layers=6).to("cuda:0")
    out = enc(wav, n_samples=torch.tensor(ns))
    units, dense = out["units"].cpu().numpy(), out["dense"].cpu().numpy()
    order = np.argsort(ns)
    for i in (0, 31, int(order[10]), int(order[21])):
        T = hr.num_frames(ns[i])
        assert int(out["frames"][i]) == T
        t64, t32, u64, u32 = _oracles(tl, wav[i, :ns[i]].numpy())
        _check_units_tl(hr, units[i, :T], u64, u32, t64[5], t32[5], tl["centers"].double(), dense[i, :T],
                        f"utt {i} ({ns[i]} samples)")
    for i in range(32):
        T = int(out["frames"][i])
        one = enc(wav[i:i + 1, :ns[i]])
        np.testing.assert_array_equal(one["units"][0].cpu().numpy(), units[i, :T])
        np.testing.assert_array_equal(one["dense"][0].cpu().numpy(), dense[i, :T])
    outs = []
    try:
        for mode in (0, 2, 4, 1):
            assert _lib.lib.dissc_set_option(b"hubert_split", mode) == 0
            e = HubertEncoder(tl["sd"], tl["centers"], n_layers=6).to("cuda:0")
            o = e(wav, n_samples=torch.tensor(ns))
            outs.append((o["units"].cpu(), o["dense"].cpu()))
            del e
    finally:
        _lib.lib.dissc_set_option(b"hubert_split", 1)
    for u, d in outs[1:]:
        for i in range(32):
            T = int(out["frames"][i])
            assert torch.equal(u[i, :T], outs[0][0][i, :T]) and torch.equal(d[i, :T], outs[0][1][i, :T])
