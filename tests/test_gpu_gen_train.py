"""csrc/gen_train.hip and nn.CodeGenerator on the GPU: the multi-tensor weight norm on both sides of its wave / workgroup
threshold and of the 128-tensor pointer slice, the embeddings' forward and dense gradient, the MRF mean and the tanh tail bit
for bit or under the bars of tests/conv_grad_ref.check (e <= K max(e_cpu, 2^-24 rms(R64)), K = 4 unless an exception is
written next to its measured figure), then the whole generator: every entry of named_grads() against the float64 reference
evaluated with the engine's own leaky-ReLU decisions, the mel loss on top, one AdamW step.
Measured ratios: profiles/gen_train.md."""
import ctypes

import numpy as np
import pytest
import torch

import conv_grad_ref as R
import gen_train_ref as GT
import mel_ref
import synthdata as synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 12345.0


@pytest.fixture(scope="module")
def nn():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import nn
    return nn


def _i32(a):
    return torch.tensor(list(a), dtype=torch.int32, device=DEV)


# ---------------------------------------------------------------------------------------------------------
# 1. weight norm
# ---------------------------------------------------------------------------------------------------------
def _wn_data(shapes, seed):
    rs = np.random.RandomState(seed)
    f = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32))
    return [f(r, c) for r, c in shapes], [f(r).abs() + 0.25 for r, _ in shapes], [f(r, c) for r, c in shapes]


def _wn_run(nn, shapes, vs, gs, gws):
    """forward + backward of one handle into sentinel-filled buffers -> per tensor (w, gv, gg), and the two flat buffers"""
    wn = nn.WeightNorm(shapes)
    v_flat, g_flat = torch.zeros(wn.total), torch.zeros(wn.total_rows)
    for (r, c), o, ro, v, g in zip(shapes, wn.off, wn.row_off, vs, gs):
        v_flat[o:o + r * c], g_flat[ro:ro + r] = v.reshape(-1), g
    v_flat, g_flat = v_flat.to(DEV), g_flat.to(DEV)
    w_flat = torch.full((wn.total,), SENT, device=DEV)
    gv_flat = torch.full((wn.total,), SENT, device=DEV)
    _, inv = wn.forward(v_flat, g_flat, out=w_flat)
    _, gg, _ = wn.backward(v_flat, g_flat, [None if t is None else t.to(DEV) for t in gws], gv_out=gv_flat)
    torch.cuda.synchronize()
    w_flat, gv_flat, gg, inv = w_flat.cpu(), gv_flat.cpu(), gg.cpu(), inv.cpu()
    for (r, c), ro, v in zip(shapes, wn.row_off, vs):  # the kept 1 / ||v||: within 1 ulp
        want = 1.0 / v.double().norm(dim=1)
        assert ((inv[ro:ro + r].double() - want).abs() <= 2.0 ** -23 * want).all()
    out = [(w_flat[o:o + r * c].view(r, c), gv_flat[o:o + r * c].view(r, c), gg[ro:ro + r])
           for (r, c), o, ro in zip(shapes, wn.off, wn.row_off)]
    return wn, out, w_flat, gv_flat


def test_weight_norm(nn):
    W = nn.WNORM_WAVE_COLS
    shapes = [(1, 112), (3, 1), (2, 3), (16, 48), (16, 176), (5, W - 1), (5, W), (5, W + 1), (7, 1799), (4, 2816), (2, 4097)]
    vs, gs, gws = _wn_data(shapes, seed=11)
    null = 4
    given = [None if i == null else t for i, t in enumerate(gws)]
    wn, out, w_flat, gv_flat = _wn_run(nn, shapes, vs, gs, given)
    assert wn.has_gaps
    bad = []
    for i, ((r, c), v, g, gw, (w, gv, gg)) in enumerate(zip(shapes, vs, gs, given, out)):
        r64, r32 = GT.weight_norm_ref(v, g, gw, torch.float64), GT.weight_norm_ref(v, g, gw, torch.float32)
        bad += R.check(f"wnorm {r} x {c} w", "weight", w, r64[0], r32[0])
        if i == null:  # a null gradient: exact zeros
            assert not gv.any() and not gg.any()
            continue
        bad += R.check(f"wnorm {r} x {c} gv", "weight", gv, r64[1], r32[1])
        bad += R.check(f"wnorm {r} x {c} gg", "vec", gg, r64[2], r32[2])
    assert not bad, bad
    # the alignment gaps keep the sentinel
    gap = torch.ones(wn.total, dtype=torch.bool)
    for (r, c), o in zip(shapes, wn.off):
        gap[o:o + r * c] = False
    assert gap.sum() > 0 and (w_flat[gap] == SENT).all() and (gv_flat[gap] == SENT).all()
    assert not (w_flat[~gap] == SENT).any() and not (gv_flat[~gap] == SENT).any()
    # two calls: the same bits; a tensor in a handle of its own: the same bits
    _, again, _, _ = _wn_run(nn, shapes, vs, gs, given)
    for a, b in zip(out, again):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    for i in (2, 5, 6, 7, 8, 10):
        _, alone, _, _ = _wn_run(nn, shapes[i:i + 1], vs[i:i + 1], gs[i:i + 1], gws[i:i + 1])
        assert all(torch.equal(x, y) for x, y in zip(out[i], alone[0])), shapes[i]


def test_weight_norm_two_pointer_slices_and_bias_gather(nn):
    W = nn.WNORM_WAVE_COLS
    shapes = [(2, 5 + i % 7) for i in range(128)] + [(2, 37), (3, W + 188)]
    vs, gs, gws = _wn_data(shapes, seed=12)
    gws[3] = gws[128] = None
    _, out, _, _ = _wn_run(nn, shapes, vs, gs, gws)
    for i in (0, 127, 129):
        _, alone, _, _ = _wn_run(nn, shapes[i:i + 1], vs[i:i + 1], gs[i:i + 1], gws[i:i + 1])
        assert all(torch.equal(x, y) for x, y in zip(out[i], alone[0])), i
    r64, r32 = (GT.weight_norm_ref(vs[129], gs[129], gws[129], d) for d in (torch.float64, torch.float32))
    assert not R.check("slot 129 gv", "weight", out[129][1], r64[1], r32[1])
    assert not out[128][1].any() and not out[3][2].any() and out[127][1].any()
    # the bias gradients of both slices, gathered by the same launches: copies, each at the next multiple of 4 floats
    sizes = [1 + i % 5 for i in range(130)]
    wn = nn.WeightNorm(shapes, sizes)
    rs = np.random.RandomState(3)
    gbs = [torch.from_numpy(rs.randn(n).astype(np.float32)).to(DEV) for n in sizes]
    gbs[1] = gbs[129] = None
    v_flat, g_flat = torch.ones(wn.total, device=DEV), torch.ones(wn.total_rows, device=DEV)
    buf, _ = wn.forward(v_flat, g_flat, torch.arange(wn.bias_total, dtype=torch.float32, device=DEV))
    assert torch.equal(buf[wn.total:].cpu(), torch.arange(wn.bias_total, dtype=torch.float32))
    _, _, gb = wn.backward(v_flat, g_flat, [None] * 130, gbs)
    want = torch.zeros(wn.bias_total)
    for o, t in zip(wn.bias_off, gbs):
        assert o % 4 == 0
        if t is not None:
            want[o:o + t.numel()] = t.cpu()
    assert torch.equal(gb.cpu(), want) and wn.bias_off[129] > wn.bias_off[128] > 0


# ---------------------------------------------------------------------------------------------------------
# 2. embeddings
# ---------------------------------------------------------------------------------------------------------
E, N_CODES, N_SPK = 16, 20, 200


def _embed_tables(seed=0):
    rs = np.random.RandomState(seed)
    return (torch.from_numpy(rs.randn(N_CODES, E).astype(np.float32)), torch.from_numpy(rs.randn(N_SPK, E).astype(np.float32)))


def _embed_run(nn, dw, sw, code, f0, spkr, lengths, gx):
    d, s = dw.to(DEV).requires_grad_(True), sw.to(DEV).requires_grad_(True)
    x = nn.embed_concat(d, s, code.to(DEV), f0.to(DEV), spkr.to(DEV), _i32(lengths), gx.shape[2])
    x.backward(gx.to(DEV))
    torch.cuda.synchronize()
    return x.detach().cpu(), d.grad.cpu(), s.grad.cpu()


def _embed_raw_fwd(lib, dw, sw, code, f0, spkr, lengths, ld):
    """the forward into a sentinel-filled buffer: what it does not write stays"""
    B, T = code.shape
    x = torch.full((B, 2 * E + 1, ld), SENT, device=DEV)
    args = [t.to(DEV).contiguous() for t in (code, f0, spkr, dw, sw)] + [_i32(lengths)]
    rc = lib.dissc_embed_concat_fwd(*[ctypes.c_void_p(t.data_ptr()) for t in args], B, T, E, N_CODES, N_SPK,
                                    ctypes.c_void_p(x.data_ptr()), ld, None)
    assert rc == 0
    torch.cuda.synchronize()
    return x.cpu()


@pytest.mark.parametrize("B,T,lengths,same_id", [(4, 130, [130, 64, 1, 0], False), (4, 130, [130, 64, 1, 0], True), (1, 1, [1], False),
                                                 (2, 9, [9, 4], False)])
def test_embeddings(nn, B, T, lengths, same_id):
    from dissc_amd import lib
    rs = np.random.RandomState(B * T + same_id)
    dw, sw = _embed_tables()
    ld = (T + 3) // 4 * 4
    code = torch.from_numpy(rs.randint(0, 17, (B, T)))  # ids 17, 18, 19 stay unused
    if same_id:
        code[:] = 3  # every position the same id: the longest chain
    f0 = torch.from_numpy(rs.randn(B, T).astype(np.float32))
    spkr = torch.tensor([5, 5, 9, 100][:B])  # two utterances of one speaker
    gx = torch.from_numpy(rs.randn(B, 2 * E + 1, ld).astype(np.float32))
    x, gd, gs = _embed_run(nn, dw, sw, code, f0, spkr, lengths, gx)
    r64 = GT.embed_ref(dw, sw, code, f0, spkr, lengths, gx, torch.float64)
    r32 = GT.embed_ref(dw, sw, code, f0, spkr, lengths, gx, torch.float32)
    # forward: torch's indexing bit for bit; nothing written at or beyond lengths
    raw = _embed_raw_fwd(lib, dw, sw, code, f0, spkr, lengths, ld)
    for b, n in enumerate(lengths):
        assert torch.equal(raw[b, :, :n], r32[0][b, :, :n]) and (raw[b, :, n:] == SENT).all()
    assert torch.equal(x[:, :, :T], r32[0]) and not x[:, :, T:].any()
    bad = R.check(f"embed B {B} T {T} g_dict", "weight", gd, r64[1], r32[1])
    bad += R.check(f"embed B {B} T {T} g_spkr", "weight", gs, r64[2], r32[2])
    assert not bad, bad
    used, used_s = set(int(c) for b, n in enumerate(lengths) for c in code[b, :n]), set(int(s) for s, n in zip(spkr, lengths) if n)
    for i in range(N_CODES):
        assert bool(gd[i].any()) == (i in used), i
    for i in range(N_SPK):
        assert bool(gs[i].any()) == (i in used_s), i
    # two calls: the same bits; 1e30 beyond lengths (and in the row's padding) changes nothing
    poisoned = gx.clone()
    for b, n in enumerate(lengths):
        poisoned[b, :, n:] = 1e30
    _, gd2, gs2 = _embed_run(nn, dw, sw, code, f0, spkr, lengths, poisoned)
    assert torch.equal(gd2, gd) and torch.equal(gs2, gs)
    # ids outside the tables behave as the forward clamps them
    wild, wild_s = code.clone(), spkr.clone()
    wild[0, 0], wild_s[0] = -3, 1000
    if T > 1:
        wild[0, 1] = 25
    xw, gdw, gsw = _embed_run(nn, dw, sw, wild, f0, wild_s, lengths, gx)
    xc, gdc, gsc = _embed_run(nn, dw, sw, wild.clamp(0, N_CODES - 1), f0, wild_s.clamp(0, N_SPK - 1), lengths, gx)
    assert torch.equal(xw, xc) and torch.equal(gdw, gdc) and torch.equal(gsw, gsc) and gdc[0].any() and gsc[N_SPK - 1].any()


def test_embeddings_code_stream_repeated(nn):
    """a code stream at half the f0 rate: the Python side repeats the ids (generator.py's _upsample), the scatter sees T ids"""
    from dissc_amd.generator import CodeGenerator as Inference
    rs = np.random.RandomState(4)
    dw, sw = _embed_tables(1)
    B, T, lengths = 2, 10, [10, 6]
    half = torch.from_numpy(rs.randint(0, N_CODES, (B, T // 2)))
    code = Inference._upsample(half.unsqueeze(1), T).squeeze(1).contiguous()
    assert torch.equal(code, torch.from_numpy(np.repeat(half.numpy(), 2, axis=1)))
    f0 = torch.from_numpy(rs.randn(B, T).astype(np.float32))
    spkr, gx = torch.tensor([1, 2]), torch.from_numpy(rs.randn(B, 2 * E + 1, 12).astype(np.float32))
    x, gd, gs = _embed_run(nn, dw, sw, code, f0, spkr, lengths, gx)
    r64 = GT.embed_ref(dw, sw, code, f0, spkr, lengths, gx, torch.float64)
    r32 = GT.embed_ref(dw, sw, code, f0, spkr, lengths, gx, torch.float32)
    assert torch.equal(x[:, :, :T], r32[0])
    assert not R.check("repeated g_dict", "weight", gd, r64[1], r32[1]) + R.check("repeated g_spkr", "weight", gs, r64[2], r32[2])


# ---------------------------------------------------------------------------------------------------------
# 3. MRF mean, 4. tanh
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nk", [1, 2, 3])
def test_mrf_mean_bit_for_bit(nn, nk):
    from dissc_amd import lib
    rs = np.random.RandomState(nk)
    B, C, ld, lengths = 3, 16, 12, [12, 5, 0]
    rs_ = [torch.from_numpy(rs.randn(B, C, ld).astype(np.float32)) for _ in range(nk)]
    g = torch.from_numpy(rs.randn(B, C, ld).astype(np.float32))
    valid = torch.zeros(B, 1, ld, dtype=torch.bool)
    for b, n in enumerate(lengths):
        valid[b, :, :n] = True
    want = rs_[0]
    for r in rs_[1:]:
        want = want + r
    want = want / nk  # ((a + b) + c) / nk on the CPU in fp32
    dev = [r.to(DEV).requires_grad_(True) for r in rs_]
    y = nn.mrf_mean(dev, _i32(lengths))
    y.backward(g.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(y.detach().cpu(), torch.where(valid, want, torch.zeros(())))
    for r in dev:
        assert torch.equal(r.grad.cpu(), torch.where(valid, g / nk, torch.zeros(())))
    # into a sentinel-filled buffer: nothing is written at or beyond lengths
    raw = torch.full((B, C, ld), SENT, device=DEV)
    ptrs = (ctypes.c_void_p * nk)(*[r.data_ptr() for r in dev])
    assert lib.dissc_mrf_mean_fwd(ptrs, nk, ctypes.c_void_p(raw.data_ptr()), ctypes.c_void_p(_i32(lengths).data_ptr()), B, C, ld, ld,
                                  None) == 0
    torch.cuda.synchronize()
    assert torch.equal(raw.cpu(), torch.where(valid, want, torch.full((), SENT)))


def test_tanh(nn):
    B, C, ld, cols, lengths = 2, 1, 1032, 1030, [1030, 517]
    rs = np.random.RandomState(5)
    x = torch.from_numpy(np.stack([np.linspace(-12, 12, ld), 3 * rs.randn(ld)]).astype(np.float32)).view(B, C, ld)
    gy = torch.from_numpy(rs.randn(B, C, cols).astype(np.float32))
    xd = x.to(DEV).requires_grad_(True)
    y = nn.tanh(xd, _i32(lengths), cols)
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    y, gx = y.detach().cpu(), xd.grad.cpu()
    valid = torch.zeros(B, C, ld, dtype=torch.bool)
    for b, n in enumerate(lengths):
        valid[b, :, :n] = True

    def ref(dtype):
        xx = x.to(dtype).requires_grad_(True)
        yy = torch.tanh(xx) * valid
        (yy[:, :, :cols] * gy.to(dtype)).sum().backward()
        return yy.detach()[:, :, :cols], xx.grad

    r64, r32 = ref(torch.float64), ref(torch.float32)
    assert y.shape == (B, C, cols) and gx.shape == (B, C, ld)
    bad = R.check("tanh y", "act", y, r64[0], r32[0]) + R.check("tanh gx", "act", gx, r64[1], r32[1])
    assert not bad, bad
    assert not y[~valid[:, :, :cols]].any() and not gx[~valid].any()
    sat = y.abs() == 1
    assert sat.sum() >= 20 and not gx[:, :, :cols][sat].any()  # y = +-1: exactly no gradient


# ---------------------------------------------------------------------------------------------------------
# 5 - 7. the whole generator
# ---------------------------------------------------------------------------------------------------------
def _kind(key, t):
    return "weight" if t.dim() >= 2 and not key.endswith(".weight_g") else "vec"


# Every tensor below is held to K = 4, whole and worst row: the worst ratios measured on an MI355X over both configs are
# 2.16 (whole: a ResBlock bias of the VCTK config) and 2.19 (worst row: a ResBlock weight_v); profiles/gen_train.md has the table.
def _check_grads(tag, named, g64, g32):
    bad = []
    for key, t in named.items():
        kind = _kind(key, t)
        flat = (lambda a: a.reshape(-1)) if kind == "vec" else (lambda a: a)
        bad += R.check(f"{tag} {key}", kind, flat(t.detach().cpu()), flat(g64[key]), flat(g32[key]))
    return bad


def _gen_inputs(h, B, T, seed):
    code, f0, spkr, _ = synth.synth_generator_inputs(B, T, seed=seed, n_spk=200, n_codes=h["num_embeddings"])
    return torch.from_numpy(code), torch.from_numpy(f0), torch.from_numpy(spkr)


def _valid_cols(lengths, rate, shape):
    m = torch.zeros(shape, dtype=torch.bool)
    for b, n in enumerate(lengths):
        m[b, :, :rate * n] = True
    return m


@pytest.fixture(scope="module")
def small(nn):
    """the small config, loaded once; its batch, cotangent, one forward + backward and both references"""
    h = GT.SMALL_CONFIG
    sd = synth.synth_generator_state_dict(h, seed=3)
    G = nn.CodeGenerator(h).to(DEV)
    G.load_state_dict(sd)
    B, T, lengths = 3, 13, [13, 7, 1]
    code, f0, spkr = _gen_inputs(h, B, T, seed=5)
    gwav = torch.from_numpy(np.random.RandomState(6).randn(B, 1, 8 * T).astype(np.float32))
    taps = []
    wav = G(code=code, f0=f0, spkr=spkr, lengths=lengths, taps=taps)
    wav.backward(gwav.to(DEV))
    torch.cuda.synchronize()
    grads = {k: t.clone() for k, t in G.named_grads().items()}
    return dict(h=h, sd=sd, G=G, B=B, T=T, lengths=lengths, code=code, f0=f0, spkr=spkr, gwav=gwav, wav=wav.detach().cpu(),
                taps=[t.detach().cpu() for t in taps], grads=grads)


def test_generator_small_config(nn, small):
    s = small
    h, G, lengths = s["h"], s["G"], s["lengths"]
    assert s["wav"].shape == (3, 1, 104) and len(s["taps"]) == len(GT.conv_input_rates(h))
    masks = [t > 0 for t in s["taps"]]
    args = (s["sd"], h, s["code"], s["f0"], s["spkr"], lengths)
    w64, g64 = GT.generator_ref(*args, torch.float64, gwav=s["gwav"], masks=masks)
    w32, g32 = GT.generator_ref(*args, torch.float32, gwav=s["gwav"], masks=masks)
    assert set(s["grads"]) == set(s["sd"]) == set(g64)
    bad = R.check("small wav", "act", s["wav"], w64, w32)
    bad += _check_grads("small", s["grads"], g64, g32)
    # the reference on its OWN branch decisions: only a count of how many differ from the engine's
    own = []
    GT.generator_ref(*args, torch.float64, taps=own)
    differ = total = 0
    for rate, e, r in zip(GT.conv_input_rates(h), s["taps"], own):
        v = _valid_cols(lengths, rate, r.shape).expand_as(r)
        differ += int(((e[:, :, :r.shape[2]] > 0) != (r > 0))[v].sum())
        total += int(v.sum())
    print(f"GT small: {differ} of {total} leaky-ReLU decisions differ between the engine and the float64 reference")
    assert not bad, bad
    # nothing beyond lengths
    assert not s["wav"][~_valid_cols(lengths, 8, s["wav"].shape)].any()


def test_generator_small_reproducible_ragged_and_alone(nn, small):
    s = small
    G, lengths = s["G"], s["lengths"]

    def run(code, f0, spkr, lengths, gwav, poison=False):
        G.zero_grad()
        taps = []
        wav = G(code=code, f0=f0, spkr=spkr, lengths=lengths, taps=taps)
        if poison:  # 1e30 in every activation row beyond its utterance's length, before the backward reads them
            for rate, t in zip(GT.conv_input_rates(s["h"]), taps):
                t.data[~_valid_cols(lengths, rate, t.shape).expand_as(t).to(DEV)] = 1e30
        wav.backward(gwav.to(DEV))
        torch.cuda.synchronize()
        return wav.detach().cpu(), {k: t.clone() for k, t in G.named_grads().items()}

    wav, grads = run(s["code"], s["f0"], s["spkr"], lengths, s["gwav"])
    assert torch.equal(wav, s["wav"]) and all(torch.equal(grads[k], s["grads"][k]) for k in grads)
    # poison beyond lengths: ids and f0 of the padding, the cotangent, the saved activations
    code, f0, gwav = s["code"].clone(), s["f0"].clone(), s["gwav"].clone()
    for b, n in enumerate(lengths):
        code[b, n:], f0[b, :, n:], gwav[b, :, 8 * n:] = 19, 1e30, 1e30
    wav2, grads2 = run(code, f0, s["spkr"], lengths, gwav, poison=True)
    assert torch.equal(wav2, wav) and all(torch.equal(grads2[k], grads[k]) for k in grads)
    # an utterance alone: the same wav bits as in the batch
    for b, n in enumerate(lengths):
        alone, _ = run(s["code"][b:b + 1, :n], s["f0"][b:b + 1, :, :n], s["spkr"][b:b + 1], [n], s["gwav"][b:b + 1, :, :8 * n])
        assert torch.equal(alone[0], wav[b, :, :8 * n]), (b, n)


def test_generator_state_dict_round_trip_and_inference_twin(nn, small):
    import dissc_amd
    s = small
    sd, out = s["sd"], s["G"].state_dict()
    assert set(out) == set(sd) and all(out[k].shape == sd[k].shape and torch.equal(out[k], sd[k]) for k in sd)
    inf = dissc_amd.CodeGenerator(s["h"]).to(DEV)
    inf.load_state_dict(out)
    y = inf(code=s["code"], f0=s["f0"], spkr=s["spkr"], lengths=torch.tensor(s["lengths"])).cpu()
    e = (y - s["wav"]).double()
    rms = float(e.pow(2).mean().sqrt())
    print(f"GT inference twin vs trainable forward: rms {rms:.3e}, max {float(e.abs().max()):.3e}")
    # tests/test_gpu_generator.py's bars: the acceptance bar, and the one between two forms of the engine's own forward
    assert rms <= 1e-4 and rms <= 5e-6 and float(e.abs().max()) <= 1e-4


def test_generator_vctk_mel_loss(nn):
    """the shipped config with the mel loss on top: the loss value against the float64 mel of the engine's wav, every
    parameter gradient against the float64 generator fed the engine's own wav cotangent and branch decisions (the
    discontinuous sign(a - b) of the L1 stays outside: tests/test_gpu_mel_grad.py)"""
    import dissc_amd
    h = synth.VCTK_CONFIG
    sd = synth.synth_generator_state_dict(h, seed=0)
    G = nn.CodeGenerator(h).to(DEV)
    G.load_state_dict(sd)
    B, T, lengths = 2, 6, [6, 3]
    code, f0, spkr = _gen_inputs(h, B, T, seed=8)
    ns = [320 * n for n in lengths]
    target = torch.from_numpy(0.3 * np.random.RandomState(9).randn(B, 320 * T).astype(np.float32))
    ms = dissc_amd.MelSpectrogram().to(DEV)
    taps = []
    wav = G(code=code, f0=f0, spkr=spkr, lengths=lengths, taps=taps)
    wav.retain_grad()
    loss = 45 * ms.l1_loss(target.to(DEV), wav, n_samples=ns)
    loss.backward()
    torch.cuda.synchronize()
    w = wav.detach().cpu()
    num = sum(float((mel_ref.mel(target[b, :n].numpy()) - mel_ref.mel(w[b, 0, :n].numpy())).abs().sum()) for b, n in enumerate(ns))
    v64 = 45 * num / sum(80 * (n // 256) for n in ns)
    print(f"GT vctk loss {float(loss.detach()):.6f}, float64 mel of the engine's wav {v64:.6f}")
    assert abs(float(loss.detach()) - v64) <= 1e-5 * v64  # tests/test_gpu_mel_grad.py's bar for the loss
    gwav, masks = wav.grad.cpu(), [t.detach().cpu() > 0 for t in taps]
    assert gwav.abs().sum() > 0 and not gwav[~_valid_cols(lengths, 320, gwav.shape)].any()
    w64, g64 = GT.generator_ref(sd, h, code, f0, spkr, lengths, torch.float64, gwav=gwav, masks=masks)
    w32, g32 = GT.generator_ref(sd, h, code, f0, spkr, lengths, torch.float32, gwav=gwav, masks=masks)
    bad = R.check("vctk wav", "act", w, w64, w32) + _check_grads("vctk", G.named_grads(), g64, g32)
    assert not bad, bad


def test_one_optimiser_step(nn, small):
    import dissc_amd
    s = small
    G = nn.CodeGenerator(s["h"]).to(DEV)
    G.load_state_dict(s["sd"])
    assert len(G.parameters()) == 5 and all(p.is_leaf and p.requires_grad for p in G.parameters())
    opt = torch.optim.AdamW(G.parameters(), 2e-4, betas=(0.8, 0.99))
    ms = dissc_amd.MelSpectrogram(n_fft=64, num_mels=20, hop_size=16, win_size=64).to(DEV)
    target = torch.from_numpy(0.3 * np.random.RandomState(2).randn(3, 104).astype(np.float32)).to(DEV)
    lengths, ns = [13, 7, 4], [104, 56, 32]

    def loss_of():
        return 45 * ms.l1_loss(target, G(code=s["code"], f0=s["f0"], spkr=s["spkr"], lengths=lengths), n_samples=ns)

    first = loss_of()
    first.backward()
    nonzero = {k for k, t in G.named_grads().items() if t.any()}
    opt.step()
    with torch.no_grad():
        second = float(loss_of())
    print(f"GT one AdamW step: loss {float(first.detach()):.6f} -> {second:.6f}")
    assert np.isfinite(second) and second != float(first.detach())
    after = G.state_dict()
    assert nonzero == set(s["sd"])
    for k in nonzero:  # every tensor that had a gradient moved
        assert not torch.equal(after[k], s["sd"][k]), k
