"""dissc_amd.nn.conv1d_grouped, nn.mean_pool and nn.discriminator_s on the GPU: the device-side packings bit for bit against a host
packing, every gradient of the layer against torch in float64 under the bars of tests/train_stage_cases.py (ragged INPUT lengths
around the stride, the halo, the chunk and a partial boundary; the six grouped layers of DiscriminatorS at full channel count and
three small shapes), the layers at the trainer's row lengths, the pool against its stated fp32 expression, and DiscriminatorS end
to end against its float64 restatement.  Measured ratios: profiles/conv_grouped_grad.md."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_grouped_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def nn():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import nn
    return nn


def case(cin, cout, k, s, g, B, ld, seed, bias=True):
    rs = np.random.RandomState(seed)
    x = torch.from_numpy(rs.randn(B, cin, ld).astype(np.float32))
    x[torch.from_numpy(rs.rand(B, cin, ld) < 0.02)] = 0.0  # exact zeros: the x = 0 branch is the slope
    w = torch.from_numpy((rs.uniform(-1, 1, (cout, cin // g, k)) / np.sqrt(cin // g * k)).astype(np.float32))
    b = torch.from_numpy(rs.uniform(-1, 1, cout).astype(np.float32)) if bias else None
    gy = torch.from_numpy(rs.randn(B, cout, R.out_ld(ld, s)).astype(np.float32))
    return x, w, b, gy


def run(nn, s, g, x, w, b, gy, lengths, slope, need=(True, True, True), nan_workspace=False):
    """one forward + backward of nn.conv1d_grouped on the device; returns [y, gx, gw, gb], None where there is none"""
    xd = x.to(DEV).requires_grad_(need[0])
    wd = w.to(DEV).requires_grad_(need[1])
    bd = None if b is None else b.to(DEV).requires_grad_(need[2])
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV)
    y = nn.conv1d_grouped(xd, wd, bd, stride=s, groups=g, lengths=ln, in_slope=slope)
    if nan_workspace:
        for ws in nn._workspaces.values():
            ws.fill_(255)  # every float of the workspace a NaN
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    return [y.detach().cpu()] + [None if t is None or t.grad is None else t.grad.cpu() for t in (xd, wd, bd)]


# ---- the packings -------------------------------------------------------------------------------------------------------
def _host_packing(w, g, which):
    """include/dissc_hip.h, dissc_convggrad_packed"""
    cout, cig, k = w.shape
    cog, pad = cout // g, (k - 1) // 2
    po = R.ceil4(pad)
    k4n = (po + pad) // 4 + 1
    wg = w.numpy().reshape(g, cog, cig, k)
    rows, red = (cog, cig) if which == 0 else (cig, cog)
    rtn, c4n = R.cdiv(rows, 16), R.cdiv(red, 4)
    wp = np.zeros((g, rtn * 16, c4n * 4, 4 * k4n), dtype=np.float32)  # [group][row][reduction channel][o']
    wp[:, :rows, :red, po - pad:po - pad + k] = wg if which == 0 else wg.transpose(0, 2, 1, 3)
    grp, rt, c4, k4, lane, e = np.meshgrid(*(np.arange(n) for n in (g, rtn, c4n, k4n, 64, 4)), indexing="ij")
    return wp[grp, 16 * rt + lane % 16, 4 * c4 + lane // 16, 4 * k4 + e]


@pytest.mark.parametrize("cin,cout,k,s,g", R.DISC_S[:4] + R.SMALL + [(40, 96, 5, 2, 1)])
def test_device_packing_bit_for_bit(nn, cin, cout, k, s, g):
    from dissc_amd import _lib
    lib = _lib.lib
    lib.dissc_convggrad_packed.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.dissc_convggrad_packed.restype = ctypes.c_longlong
    x, w, b, gy = case(cin, cout, k, s, g, 1, 16, seed=cin + k)
    h = nn._handle(nn.CONV1D_GROUPED, cin, cout, k, s, torch.device(DEV), g)
    wd = w.to(DEV)
    _lib.check(nn.CONV1D_GROUPED.set_weights(h, wd.data_ptr(), None, None), "dissc_convggrad_set_weights")
    for which in (0, 1):
        host = _host_packing(w, g, which)
        n = lib.dissc_convggrad_packed(h, which, None, None)
        assert n == host.size
        dst = torch.full((n,), float("nan"), device=DEV)
        assert lib.dissc_convggrad_packed(h, which, dst.data_ptr(), None) == n
        torch.cuda.synchronize()
        assert np.array_equal(dst.cpu().numpy().view(np.uint32), host.reshape(-1).view(np.uint32))


# ---- the layer ----------------------------------------------------------------------------------------------------------
# Exceptions to K = 4 (tests/train_stage_cases.py's rule, as tests/test_gpu_conv_strided_grad.py's K_EXC: only for y or gx, only
# where one output is ONE sequential fp32 chain of n >= 1 024 products in a matrix-core accumulator; K = 2 x the measured worst
# ratio over every case of this file, rounded up, never above min(32, max(4, sqrt(n)))).  (tensor, Cin, Cout, k, s, g) -> (whole,
# worst channel).  The weight and bias gradients get none.
# None is needed: the kernels keep four accumulators per output and add them in a fixed order, so the longest chain of one
# output is 2 624 / 4 = 656 products (convs.5, y and gx), below the rule's 1 024; every measured ratio is in
# profiles/conv_grouped_grad.md.
K_EXC = {}


def _k(tensor, cin, cout, k, s, g):
    kw, kc = K_EXC.get((tensor, cin, cout, k, s, g), (R.K_WHOLE, R.K_CH))
    n = cin // g * k if tensor == "y" else cout // g * R.cdiv(k, s)
    assert tensor in ("y", "gx") and (max(kw, kc) <= 4 or (n >= 1024 and max(kw, kc) <= R.k_cap(n)))
    return kw, kc


def lengths_for(nn, cin, cout, k, s, g, max_b=None):
    """INPUT lengths with T = 64 s (one chunk of the weight gradient): 1, 2, s, s + 1, 20, 21, 41 (the halo and the kernel), T - 1,
    T, T + 1, 2 T + 1, one of each residue mod s next to 2 T, and, where the plan has one inside an utterance, a length on either
    side of a partial boundary (placed in the utterance the boundary falls in), as test_gpu_conv_strided_grad.lengths_for does.
    max_b = 4 (the two widest layers): s + 1, 2 T - 1 and the last two of the list."""
    T = nn.WGRAD_CHUNK * s
    lengths = [1, 2, s, s + 1, 20, 21, 41, T - 1, T, T + 1, 2 * T + 1] + [2 * T - r for r in range(s)] + [T, 2 * T + 1]
    if max_b is not None:
        assert max_b == 4
        lengths = [s + 1, 2 * T - 1, T, 2 * T + 1]
    B, ld = len(lengths), R.ceil4(2 * T + 1)
    P, pairs = nn.wgrad_partials_grouped(B, ld, cin, cout, k, s, g)
    nch = R.cdiv(R.cdiv(ld, s), nn.WGRAD_CHUNK)
    inside = [divmod(p * pairs, nch) for p in range(1, P) if (p * pairs) % nch]
    if inside:
        b, c = inside[len(inside) // 2]
        lengths[-2], lengths[-1] = c * T, c * T + 1  # c chunks of outputs exactly, and one output more
        lengths[b], lengths[-1] = lengths[-1], lengths[b]  # this utterance's chunk c belongs to the next partial
    return lengths, ld, (P, pairs)


def assert_layer_gradients(run, cin, cout, k, s, g, lengths, ld, seed, k_y, k_gx, slope=0.1):
    """the four bars on a ragged batch; nothing beyond the lengths; every result bit-reproducible, also behind a workspace full of
    NaNs; poison beyond the lengths changes nothing; the five needs_input_grad combinations keep the others' bits; every utterance
    alone has the batch's y and gx bits."""
    B = len(lengths)
    x, w, b, gy = case(cin, cout, k, s, g, B, ld, seed)
    vi, vo = R.valid_masks(lengths, ld, s)
    run = functools.partial(run, lengths=lengths, slope=slope)
    y, gx, gw, gb = run(x, w, b, gy)
    r64 = R.layer_ref(x, w, b, gy, lengths, s, g, slope, torch.float64)
    r32 = R.layer_ref(x, w, b, gy, lengths, s, g, slope, torch.float32)
    bad = R.check("batch y", "act", y, r64[0], r32[0], *k_y)
    bad += R.check("batch gx", "act", gx, r64[1], r32[1], *k_gx)
    bad += R.check("batch gw", "weight", gw, r64[2], r32[2])
    bad += R.check("batch gb", "vec", gb, r64[3], r32[3])
    assert not gx[(vi == 0).expand_as(gx)].any() and not y[(vo == 0).expand_as(y)].any(), "written or propagated beyond the lengths"
    for name, t, q in zip(("y", "gx", "gw", "gb"), (y, gx, gw, gb), run(x, w, b, gy)):
        assert torch.equal(q, t), f"{name} is not bit-reproducible"
    for name, t, q in zip(("y", "gx", "gw", "gb"), (y, gx, gw, gb), run(x, w, b, gy, nan_workspace=True)):
        assert torch.equal(q, t), f"a workspace full of NaNs changes {name}"
    xp, gyp = x.clone(), gy.clone()
    xp[(vi == 0).expand_as(x)] = 1e30
    gyp[(vo == 0).expand_as(gy)] = 1e30
    for name, t, q in zip(("y", "gx", "gw", "gb"), (y, gx, gw, gb), run(xp, w, b, gyp)):
        assert torch.equal(q, t), f"poison beyond the lengths changes {name}"
    for need in ((False, True, True), (True, False, True), (True, True, False), (True, False, False), (False, False, True)):
        for name, t, q, on in zip(("gx", "gw", "gb"), (gx, gw, gb), run(x, w, b, gy, need=need)[1:4], need):
            assert (torch.equal(q, t) if on else q is None), f"needs_input_grad {need}: {name}"
    for i, n in enumerate(lengths):
        sl = slice(i, i + 1)
        yi, gxi, _, _ = run(x[sl], w, b, gy[sl], lengths=[n])
        assert torch.equal(gxi, gx[sl]), ("alone gx differs from the batch's", i, n)
        assert torch.equal(yi, y[sl]), ("alone y differs from the batch's", i, n)
    assert not bad, bad


@pytest.mark.parametrize("cin,cout,k,s,g", R.DISC_S + R.SMALL)
def test_layer_gradients_against_float64(nn, cin, cout, k, s, g):
    lengths, ld, plan = lengths_for(nn, cin, cout, k, s, g, max_b=4 if cout >= 1024 else None)
    print(f"\nlayer {cin} -> {cout} k {k} s {s} g {g}: lengths {lengths}, ld {ld}, (P, pairs) {plan}")
    assert_layer_gradients(functools.partial(run, nn, s, g), cin, cout, k, s, g, lengths, ld, 7 * cin + k + s,
                           _k("y", cin, cout, k, s, g), _k("gx", cin, cout, k, s, g))


@pytest.mark.parametrize("layer", range(6))
def test_training_shape(nn, layer):
    """2 x 2 rows at the layer's own scale-0 row length, two rows shorter: the kernels' tile walk over a long row; the four bars,
    every result bit-reproducible"""
    (cin, cout, k, s, g), L = R.DISC_S[layer], R.TRAIN_L[layer]
    B, ld, slope = 4, R.ceil4(L), 0.1
    lengths = [L, L // 2 + 1, L, max(1, L // 3)]
    x, w, b, gy = case(cin, cout, k, s, g, B, ld, seed=L + k)
    y, gx, gw, gb = run(nn, s, g, x, w, b, gy, lengths, slope)
    r64 = R.layer_ref(x, w, b, gy, lengths, s, g, slope, torch.float64)
    r32 = R.layer_ref(x, w, b, gy, lengths, s, g, slope, torch.float32)
    print(f"\ntraining shape {cin} -> {cout} L {L}: plan {nn.wgrad_partials_grouped(B, ld, cin, cout, k, s, g)}")
    bad = R.check("train y", "act", y, r64[0], r32[0], *_k("y", cin, cout, k, s, g))
    bad += R.check("train gx", "act", gx, r64[1], r32[1], *_k("gx", cin, cout, k, s, g))
    bad += R.check("train gw", "weight", gw, r64[2], r32[2])
    bad += R.check("train gb", "vec", gb, r64[3], r32[3])
    for name, t, q in zip(("y", "gx", "gw", "gb"), (y, gx, gw, gb), run(nn, s, g, x, w, b, gy, lengths, slope)):
        assert torch.equal(q, t), f"{name} is not bit-reproducible"
    assert not bad, bad


# ---- the pool -----------------------------------------------------------------------------------------------------------
POOL_N = [0, 1, 2, 3, 4, 5, 8, 9, 513]


def test_mean_pool(nn):
    T, B = 513, len(POOL_N)
    rs = np.random.RandomState(4)
    wav = torch.from_numpy(rs.randn(B, 1, T).astype(np.float32))
    g = torch.from_numpy(rs.randn(B, 1, R.ceil4(T // 2 + 1)).astype(np.float32))
    ref32, gx32 = R.pool_ref(wav, POOL_N, g)           # the stated fp32 expression, by torch on the CPU
    ref64, gx64 = R.pool_ref(wav.double(), POOL_N, g.double())
    vo = torch.zeros_like(ref32)
    for i, n in enumerate(POOL_N):
        vo[i, :, :R.pool_len(n)] = 1

    def go(wav_, g_, lengths):
        wd = wav_.to(DEV).requires_grad_(True)
        out, olen = nn.mean_pool(wd, lengths)
        out.backward(g_.to(DEV))
        torch.cuda.synchronize()
        return out.detach().cpu(), wd.grad.cpu(), olen

    out, gx, olen = go(wav, g, POOL_N)
    assert list(olen) == [R.pool_len(n) for n in POOL_N]
    assert out.shape == ref32.shape and torch.equal(out, ref32), "the forward is not the stated fp32 expression"
    assert gx.shape == wav.shape and torch.equal(gx, gx32), "the backward is not the stated fp32 expression"
    bad = R.check("pool", "act", out, ref64, ref32) + R.check("pool gx", "act", gx, gx64, gx32)
    assert not out[vo == 0].any()
    for i, n in enumerate(POOL_N):
        assert not gx[i, :, n:].any()
    # poison beyond the lengths, in the waveform and in the incoming gradient
    wp, gp = wav.clone(), g.clone()
    for i, n in enumerate(POOL_N):
        wp[i, :, n:] = 1e30
    gp[vo == 0] = 1e30
    outp, gxp, _ = go(wp, gp, torch.tensor(POOL_N, dtype=torch.int32, device=DEV))  # lengths already on the device
    assert torch.equal(outp, out) and torch.equal(gxp, gx)
    # no lengths, [B, T] input
    out2, gx2, olen2 = go(wav[:, 0], g, None)
    r2, g2 = R.pool_ref(wav, None, g)
    assert torch.equal(out2, r2) and torch.equal(gx2.reshape(B, 1, T), g2) and list(olen2) == [T // 2 + 1] * B
    # the C entry with row strides larger than the row: ldx = 520, ldo = 264
    from dissc_amd import _lib
    xs = torch.full((B, 1, 520), 1e30)
    xs[:, :, :T] = wav
    xd, od = xs.to(DEV), torch.zeros(B, 1, 264, device=DEV)
    ln = torch.tensor(POOL_N, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib.dissc_mean_pool_fwd(xd.data_ptr(), od.data_ptr(), ln.data_ptr(), B, 1, T, 520, 264, None), "dissc_mean_pool_fwd")
    gd, gxd = torch.full((B, 1, 264), 1e30), torch.full((B, 1, 520), float("nan"), device=DEV)
    gd[:, :, :g.shape[2]] = gp
    gd = gd.to(DEV)
    _lib.check(_lib.lib.dissc_mean_pool_bwd(gd.data_ptr(), gxd.data_ptr(), ln.data_ptr(), B, 1, T, 520, 264, None), "dissc_mean_pool_bwd")
    torch.cuda.synchronize()
    assert torch.equal(od.cpu()[:, :, :260], ref32) and not od.cpu()[:, :, 260:].any()
    assert torch.equal(gxd.cpu()[:, :, :T], gx32) and not gxd.cpu()[:, :, T:].any()
    assert not bad, bad


# ---- DiscriminatorS end to end ------------------------------------------------------------------------------------------
def _loss(maps, hats, mask):
    """mean((1 - score)^2) over the valid scores + 2 sum_l mean |lrelu(f_l) - lrelu(fhat_l)| (the score map as it is), torch ops"""
    score = maps[7]
    loss = (((1 - score) ** 2) * mask[7]).sum() / mask[7].sum()
    for j, (f, fh) in enumerate(zip(maps, hats)):
        a, c = (f, fh) if j == 7 else (F.leaky_relu(f, R.SLOPE), F.leaky_relu(fh, R.SLOPE))
        loss = loss + 2 * (a - c).abs().sum() / (mask[j].sum() * f.shape[1])
    return loss


def test_discriminator_s_end_to_end(nn):
    B, T, lengths = 2, 1028, [1028, 771]
    rs = np.random.RandomState(11)
    w = R.disc_s_weights(seed=3)
    wav = torch.from_numpy(rs.uniform(-1, 1, (B, 1, T)).astype(np.float32))
    masks = R.map_masks(T, lengths, B)
    hats = [torch.from_numpy(rs.randn(B, c, m.shape[2]).astype(np.float32)) * 0.3 * m for c, m in zip(R.DISC_S_CHANNELS, masks)]

    wd = {n: t.to(DEV).requires_grad_(True) for n, t in w.items()}
    wavd = wav.to(DEV).requires_grad_(True)
    score, fmaps, lens = nn.discriminator_s(wavd, wd, lengths)
    assert score is fmaps[7] and len(fmaps) == 8 and len(lens) == 8
    _loss(fmaps, [h.to(DEV) for h in hats], [m.to(DEV) for m in masks]).backward()
    torch.cuda.synchronize()
    for j, (ln, m) in enumerate(zip(lens, masks)):
        assert ln.cpu().tolist() == [R.map_lengths(n)[j] for n in lengths] == m[:, 0].sum(1).long().tolist()

    ref = {}
    for dtype in (torch.float64, torch.float32):
        wr = {n: t.to(dtype).requires_grad_(True) for n, t in w.items()}
        wavr = wav.to(dtype).requires_grad_(True)
        maps = R.disc_s_ragged(wr, wavr, lengths)
        _loss(maps, [h.to(dtype) for h in hats], [m.to(dtype) for m in masks]).backward()
        ref[dtype] = ([m.detach() for m in maps], wavr.grad, {n: t.grad for n, t in wr.items()})
    m64, gwav64, g64 = ref[torch.float64]
    m32, gwav32, g32 = ref[torch.float32]
    bad = []
    for j in range(8):
        bad += R.check(f"map {j}" + (" (score)" if j == 7 else ""), "act", fmaps[j].detach(), m64[j], m32[j])
        assert fmaps[j].shape == m64[j].shape and not fmaps[j].detach().cpu()[(masks[j] == 0).expand_as(m64[j])].any()
    bad += R.check("grad wav", "act", wavd.grad, gwav64, gwav32)
    for n in sorted(wd):
        bad += R.check(f"grad {n}", "weight" if n.endswith("weight") else "vec", wd[n].grad, g64[n], g32[n])
    wdet = {k: t.detach() for k, t in wd.items()}
    for i, n in enumerate(lengths):
        assert not wavd.grad[i, :, n:].any()
        with torch.no_grad():  # alone, on its own samples only: 771 is no multiple of 4, the row is copied into a zeroed one
            alone = nn.discriminator_s(wav[i:i + 1, :, :n].contiguous().to(DEV), wdet, [n])[1]
        for j, (a, f) in enumerate(zip(alone, fmaps)):
            m = R.map_lengths(n)[j]
            assert torch.equal(a[:, :, :m], f.detach()[i:i + 1, :, :m]), ("alone map differs from the batch's", i, j)
    # the second scale: through nn.mean_pool, equal to the composition of its parts
    with torch.no_grad():
        pooled, olen = nn.mean_pool(wav.to(DEV), lengths)
        assert list(olen) == [515, 386] and pooled.shape == (B, 1, 516)
        score2, fmaps2, lens2 = nn.discriminator_s(pooled, wdet, olen)
        x, n_in = pooled, np.asarray(olen)
        for j, (name, (s, g, k)) in enumerate(zip(R.layer_names(), R.layer_params())):
            ln = torch.from_numpy(n_in.astype(np.int32)).to(DEV)
            args = (wdet[name + ".weight"], wdet[name + ".bias"])
            x = nn.conv1d_grouped(x, *args, stride=s, groups=g, lengths=ln, in_slope=R.SLOPE if j else 1.0) if j < 6 else \
                nn.conv1d(x, *args, lengths=ln, in_slope=R.SLOPE)
            n_in = -(-n_in // s)
            assert torch.equal(x, fmaps2[j]) and lens2[j].cpu().tolist() == n_in.tolist(), j
        p64 = R.disc_s_ragged({n: t.double() for n, t in w.items()}, R.pool_ref(wav.double(), lengths)[0], list(olen))
        p32 = R.disc_s_ragged(w, R.pool_ref(wav, lengths)[0], list(olen))
        bad += R.check("scale 1 score", "act", score2, p64[7], p32[7])
    assert not bad, bad
