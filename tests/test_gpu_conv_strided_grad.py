"""dissc_amd.nn.conv1d_strided, nn.period_fold and nn.discriminator_p on the GPU: the device-side packings bit for bit against a
host packing, every gradient of the layer against torch in float64 under the bars of tests/train_stage_cases.py (ragged INPUT
lengths around the stride, the chunk and a partial boundary; the four strided layers of DiscriminatorP and two other (k, stride)),
the discriminator's own row lengths at 22 rows, the fold against torch's reflect pad and view, and DiscriminatorP end to end
against its float64 Conv2d restatement.  Measured ratios: profiles/conv_strided_grad.md."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_strided_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def nn():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import nn
    return nn


def case(cin, cout, k, s, B, ld, seed, bias=True):
    rs = np.random.RandomState(seed)
    x = torch.from_numpy(rs.randn(B, cin, ld).astype(np.float32))
    x[torch.from_numpy(rs.rand(B, cin, ld) < 0.02)] = 0.0  # exact zeros: the x = 0 branch is the slope
    w = torch.from_numpy((rs.uniform(-1, 1, (cout, cin, k)) / np.sqrt(cin * k)).astype(np.float32))
    b = torch.from_numpy(rs.uniform(-1, 1, cout).astype(np.float32)) if bias else None
    gy = torch.from_numpy(rs.randn(B, cout, R.out_ld(ld, s)).astype(np.float32))
    return x, w, b, gy


def run(nn, s, x, w, b, gy, lengths, slope, need=(True, True, True)):
    """one forward + backward of nn.conv1d_strided on the device; returns [y, gx, gw, gb], None where there is none"""
    xd = x.to(DEV).requires_grad_(need[0])
    wd = w.to(DEV).requires_grad_(need[1])
    bd = None if b is None else b.to(DEV).requires_grad_(need[2])
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV)
    y = nn.conv1d_strided(xd, wd, bd, stride=s, lengths=ln, in_slope=slope)
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    return [y.detach().cpu()] + [None if t is None or t.grad is None else t.grad.cpu() for t in (xd, wd, bd)]


# ---- the packings -------------------------------------------------------------------------------------------------------
def _host_packing(w, which):
    """include/dissc_hip.h, dissc_convsgrad_packed"""
    cout, cin, k = w.shape
    rows, red = (cout, cin) if which == 0 else (cin, cout)
    nblk, c8n = R.cdiv(rows, 32), R.cdiv(red, 32) * 4
    wp = np.zeros((nblk * 32, c8n * 8, k), dtype=np.float32)  # [row][reduction channel][kk]
    wp[:rows, :red] = w.numpy() if which == 0 else w.numpy().transpose(1, 0, 2)
    blk, kk, c8, lane, e = np.meshgrid(*(np.arange(n) for n in (nblk, k, c8n, 64, 4)), indexing="ij")
    return wp[32 * blk + lane % 32, 8 * c8 + 2 * e + lane // 32, kk]


@pytest.mark.parametrize("cin,cout,k,s", R.DISC_P[:3] + R.TAP_TABLE + [(40, 33, 3, 2)])
def test_device_packing_bit_for_bit(nn, cin, cout, k, s):
    from dissc_amd import _lib
    lib = _lib.lib
    lib.dissc_convsgrad_packed.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.dissc_convsgrad_packed.restype = ctypes.c_longlong
    x, w, b, gy = case(cin, cout, k, s, 1, 16, seed=cin + k)
    h = nn._handle(nn.CONV1D_STRIDED, cin, cout, k, s, torch.device(DEV))
    wd = w.to(DEV)
    _lib.check(nn.CONV1D_STRIDED.set_weights(h, wd.data_ptr(), None, None), "dissc_convsgrad_set_weights")
    for which in (0, 1):
        host = _host_packing(w, which)
        n = lib.dissc_convsgrad_packed(h, which, None, None)
        assert n == host.size
        dst = torch.full((n,), float("nan"), device=DEV)
        assert lib.dissc_convsgrad_packed(h, which, dst.data_ptr(), None) == n
        torch.cuda.synchronize()
        assert np.array_equal(dst.cpu().numpy().view(np.uint32), host.reshape(-1).view(np.uint32))


# ---- the layer ----------------------------------------------------------------------------------------------------------
# Exceptions to K = 4 (tests/train_stage_cases.py's rule, as tests/test_gpu_conv_transpose_grad.py's K_EXC: only where one output
# is ONE sequential fp32 chain of n >= 1 024 products in a matrix-core accumulator; never above min(32, max(4, sqrt(n)))).
# (tensor, Cin, Cout, k, s) -> (whole, worst channel); K = 2 x the measured worst ratio over every case of this file, rounded up;
# measured on an MI355X (profiles/conv_strided_grad.md).  The weight and bias gradients get no exception.
#   forward of convs.3, n = 512 x 5 = 2 560 in one chain: 2.95 / 4.88 (ragged batch)  ->  6 / 10 (cap 32)
# The other candidates stay at 4: the data gradients of convs.3 (n = 1 024 x 2) and convs.2 (n = 512 x 2) measured 1.05 / 1.03
# and 1.02 / 1.02.
K_EXC = {("y", 512, 1024, 5, 3): (6.0, 10.0)}


def _k(tensor, cin, cout, k, s):
    kw, kc = K_EXC.get((tensor, cin, cout, k, s), (R.K_WHOLE, R.K_CH))
    n = cin * k if tensor == "y" else cout * R.cdiv(k, s)
    assert tensor in ("y", "gx") and (max(kw, kc) <= 4 or (n >= 1024 and max(kw, kc) <= R.k_cap(n)))
    return kw, kc


def lengths_for(nn, cin, cout, k, s, max_b=None):
    """INPUT lengths with T = 64 s (one chunk of the weight gradient): 1, 2, s, s + 1, T - 1, T, T + 1, 2 T + 1, one of each residue
    mod s next to 2 T, and, where the plan has one inside an utterance, a length on either side of a partial boundary (placed in
    the utterance the boundary falls in), as conv_grad_harness.lengths_for does.  max_b = 4 (the widest layer): s + 1, 2 T - 1
    and the last two of the list."""
    T = nn.WGRAD_CHUNK * s
    lengths = [1, 2, s, s + 1, T - 1, T, T + 1, 2 * T + 1] + [2 * T - r for r in range(s)] + [T, 2 * T + 1]
    if max_b is not None:
        assert max_b == 4
        lengths = [s + 1, 2 * T - 1, T, 2 * T + 1]
    B, ld = len(lengths), R.ceil4(2 * T + 1)
    P, pairs = nn.wgrad_partials_strided(B, ld, cin, cout, k, s)
    nch = R.cdiv(R.cdiv(ld, s), nn.WGRAD_CHUNK)
    inside = [divmod(p * pairs, nch) for p in range(1, P) if (p * pairs) % nch]
    if inside:
        b, c = inside[len(inside) // 2]
        lengths[-2], lengths[-1] = c * T, c * T + 1  # c chunks of outputs exactly, and one output more
        lengths[b], lengths[-1] = lengths[-1], lengths[b]  # this utterance's chunk c belongs to the next partial
    return lengths, ld, (P, pairs)


def assert_layer_gradients(run, cin, cout, k, s, lengths, ld, seed, k_y, k_gx, slope=0.1):
    """conv_grad_harness.assert_layer_gradients for the strided layer: the four bars on a ragged batch; nothing beyond the lengths;
    every result bit-reproducible; poison beyond the lengths changes nothing; the five needs_input_grad combinations keep the
    others' bits; every utterance alone has the batch's y and gx bits."""
    B = len(lengths)
    x, w, b, gy = case(cin, cout, k, s, B, ld, seed)
    vi, vo = R.valid_masks(lengths, ld, s)
    run = functools.partial(run, lengths=lengths, slope=slope)
    y, gx, gw, gb = run(x, w, b, gy)
    r64 = R.layer_ref(x, w, b, gy, lengths, s, slope, torch.float64)
    r32 = R.layer_ref(x, w, b, gy, lengths, s, slope, torch.float32)
    bad = R.check("batch y", "act", y, r64[0], r32[0], *k_y)
    bad += R.check("batch gx", "act", gx, r64[1], r32[1], *k_gx)
    bad += R.check("batch gw", "weight", gw, r64[2], r32[2])
    bad += R.check("batch gb", "vec", gb, r64[3], r32[3])
    assert not gx[(vi == 0).expand_as(gx)].any() and not y[(vo == 0).expand_as(y)].any(), "written or propagated beyond the lengths"
    for name, t, q in zip(("y", "gx", "gw", "gb"), (y, gx, gw, gb), run(x, w, b, gy)):
        assert torch.equal(q, t), f"{name} is not bit-reproducible"
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


@pytest.mark.parametrize("cin,cout,k,s", R.DISC_P + R.TAP_TABLE)
def test_layer_gradients_against_float64(nn, cin, cout, k, s):
    lengths, ld, plan = lengths_for(nn, cin, cout, k, s, max_b=4 if cin * cout >= 512 * 1024 else None)
    print(f"\nlayer {cin} -> {cout} k {k} s {s}: lengths {lengths}, ld {ld}, (P, pairs) {plan}")
    assert_layer_gradients(functools.partial(run, nn, s), cin, cout, k, s, lengths, ld, 7 * cin + k + s, _k("y", cin, cout, k, s),
                           _k("gx", cin, cout, k, s))


TRAIN_L = [815, 272, 91, 31]  # the rows of DiscriminatorP(11) on 8 960 samples, layer by layer


@pytest.mark.parametrize("layer", range(4))
def test_training_shape(nn, layer):
    """22 rows (B = 2, period 11) at the discriminator's own row lengths, one layer each, two rows shorter: the four bars, every
    result bit-reproducible"""
    (cin, cout, k, s), L = R.DISC_P[layer], TRAIN_L[layer]
    assert L == (R.cdiv(8960, 11) if layer == 0 else R.cdiv(TRAIN_L[layer - 1], 3))
    B, ld, slope = 22, R.ceil4(L), 0.1
    lengths = [L] * B
    lengths[3], lengths[20] = L // 2 + 1, max(1, L // 3)
    x, w, b, gy = case(cin, cout, k, s, B, ld, seed=L + k)
    y, gx, gw, gb = run(nn, s, x, w, b, gy, lengths, slope)
    r64 = R.layer_ref(x, w, b, gy, lengths, s, slope, torch.float64)
    r32 = R.layer_ref(x, w, b, gy, lengths, s, slope, torch.float32)
    print(f"\ntraining shape {cin} -> {cout} L {L}: plan {nn.wgrad_partials_strided(B, ld, cin, cout, k, s)}")
    bad = R.check("train y", "act", y, r64[0], r32[0], *_k("y", cin, cout, k, s))
    bad += R.check("train gx", "act", gx, r64[1], r32[1], *_k("gx", cin, cout, k, s))
    bad += R.check("train gw", "weight", gw, r64[2], r32[2])
    bad += R.check("train gb", "vec", gb, r64[3], r32[3])
    for name, t, q in zip(("y", "gx", "gw", "gb"), (y, gx, gw, gb), run(nn, s, x, w, b, gy, lengths, slope)):
        assert torch.equal(q, t), f"{name} is not bit-reproducible"
    assert not bad, bad


# ---- the fold -----------------------------------------------------------------------------------------------------------
def _fold(nn, wav, p, lengths, g=None):
    wd = wav.to(DEV).requires_grad_(g is not None)
    x0 = nn.period_fold(wd, p, lengths)
    if g is not None:
        x0.backward(g.to(DEV))
    torch.cuda.synchronize()
    return x0.detach().cpu(), None if g is None else wd.grad.cpu()


def _fold_grad_ref(wav, p, lengths, g):
    """the gradient of sum(fold(wav) g) by torch autograd in float64, every utterance alone, and the two terms' magnitudes"""
    B, T = wav.shape[0], wav.shape[-1]
    gw, mag = torch.zeros(B, T, dtype=torch.float64), torch.zeros(B, T, dtype=torch.float64)
    for i, n in enumerate([T] * B if lengths is None else lengths):
        if n <= 0:
            continue
        for out, gg in ((gw, g.double()), (mag, g.double().abs())):
            y = wav.reshape(B, 1, T)[i:i + 1, :, :n].double().clone().requires_grad_(True)
            v = R.fold_one(y, p)  # [1, 1, H, p]
            (v[0, 0].t() * gg[i * p:(i + 1) * p, 0, :v.shape[2]]).sum().backward()
            out[i, :n] = y.grad[0, 0]
    return gw, mag


@pytest.mark.parametrize("p", R.PERIODS)
def test_fold_against_torch(nn, p):
    rs = np.random.RandomState(p)
    T = 20 * p + 3
    cases = [(T, None), (T, [T, T - 1, p + 1, 0])]
    if p == 5:
        cases += [(T, [T - r for r in range(p)] + [7, 5, 4, 3])]  # every residue; 3 = the shortest torch pads to 5
    for T, lengths in cases:
        B = 4 if lengths is None else len(lengths)
        for shape in ((B, 1, T), (B, T)):
            wav = torch.from_numpy(rs.randn(*shape).astype(np.float32))
            ref = R.fold_ref(wav, p, lengths)
            g = torch.from_numpy(rs.randn(*ref.shape).astype(np.float32))
            x0, gwav = _fold(nn, wav, p, lengths, g)
            assert x0.shape == ref.shape and torch.equal(x0, ref), (p, lengths)  # bits, and nothing beyond the rows' lengths
            assert gwav.shape == wav.shape
            g64, mag = _fold_grad_ref(wav, p, lengths, g)
            # a sample's one or two contributions, added in either order: within 1 ulp (2^-23 relative) of the two-term sum
            assert bool(((gwav.reshape(B, T).double() - g64).abs() <= 2.0 ** -23 * mag).all()), (p, lengths)
            for i, n in enumerate([T] * B if lengths is None else lengths):
                assert not gwav.reshape(B, T)[i, n:].any()
    dev_len = torch.tensor([T, T - 1, p + 1, 0], dtype=torch.int32, device=DEV)  # lengths already on the device
    wav = torch.from_numpy(rs.randn(4, 1, T).astype(np.float32))
    assert torch.equal(nn.period_fold(wav.to(DEV), p, dev_len).cpu(), R.fold_ref(wav, p, [T, T - 1, p + 1, 0]))


@pytest.mark.parametrize("p", R.PERIODS)
def test_fold_raises_where_torch_raises(nn, p):
    wav = torch.zeros(1, 1, 4 * p, device=DEV)
    for n in range(1, 2 * p + 2):
        try:
            R.fold_one(torch.zeros(1, 1, n), p)
            raises = False
        except RuntimeError:
            raises = True
        if raises:
            with pytest.raises(ValueError):
                nn.period_fold(wav, p, [n])
            with pytest.raises(ValueError):
                nn.discriminator_p(wav, {}, p, [n])
        else:
            assert nn.period_fold(wav, p, [n]).shape == (p, 1, 4)
    assert not nn.period_fold(wav + 1, p, [0]).any()


# ---- DiscriminatorP end to end ------------------------------------------------------------------------------------------
def _loss(maps, hats, mask):
    """mean((1 - score)^2) over the valid scores + 2 sum_l mean |lrelu(f_l) - lrelu(fhat_l)| (the score map as it is), torch ops"""
    score = maps[5]
    loss = (((1 - score) ** 2) * mask[5]).sum() / mask[5].sum()
    for j, (f, fh) in enumerate(zip(maps, hats)):
        a, c = (f, fh) if j == 5 else (F.leaky_relu(f, R.SLOPE), F.leaky_relu(fh, R.SLOPE))
        loss = loss + 2 * (a - c).abs().sum() / (mask[j].sum() * f.shape[1])
    return loss


@pytest.mark.parametrize("p", [2, 11])
def test_discriminator_p_end_to_end(nn, p):
    B, T, lengths = 3, 1920, [1920, 1601, 640]
    rs = np.random.RandomState(100 + p)
    w = R.disc_p_weights(seed=p)
    wav = torch.from_numpy(rs.uniform(-1, 1, (B, 1, T)).astype(np.float32))
    masks = R.map_masks(T, p, lengths, B)
    hats = [torch.from_numpy(rs.randn(B * p, c, m.shape[2]).astype(np.float32)) * 0.3 * m for c, m in zip(R.DISC_P_CHANNELS[1:], masks)]

    wd = {n: t.to(DEV).requires_grad_(True) for n, t in w.items()}
    wavd = wav.to(DEV).requires_grad_(True)
    score, fmaps, lens = nn.discriminator_p(wavd, wd, p, lengths)
    assert score is fmaps[5] and len(fmaps) == 6 and len(lens) == 6
    _loss(fmaps, [h.to(DEV) for h in hats], [m.to(DEV) for m in masks]).backward()
    torch.cuda.synchronize()
    for ln, m in zip(lens, masks):
        assert torch.equal(ln.cpu().long(), m[:, 0].sum(1).long())

    ref = {}
    for dtype in (torch.float64, torch.float32):
        wr = {n: t.to(dtype).requires_grad_(True) for n, t in w.items()}
        wavr = wav.to(dtype).requires_grad_(True)
        maps = R.disc_p_conv2d(wr, wavr, p, lengths)
        _loss(maps, [h.to(dtype) for h in hats], [m.to(dtype) for m in masks]).backward()
        ref[dtype] = ([m.detach() for m in maps], wavr.grad, {n: t.grad for n, t in wr.items()})
    m64, gwav64, g64 = ref[torch.float64]
    m32, gwav32, g32 = ref[torch.float32]
    bad = []
    for j in range(6):
        bad += R.check(f"p {p} map {j}" + (" (score)" if j == 5 else ""), "act", fmaps[j].detach(), m64[j], m32[j])
        assert not fmaps[j].detach().cpu()[(masks[j] == 0).expand_as(m64[j])].any()
    bad += R.check(f"p {p} grad wav", "act", wavd.grad, gwav64, gwav32)
    for n in sorted(wd):
        weight = n.endswith("weight")
        got, a, c = wd[n].grad, g64[n], g32[n]
        if weight:
            got, a, c = got[:, :, :, 0], a[:, :, :, 0], c[:, :, :, 0]
        bad += R.check(f"p {p} grad {n}", "weight" if weight else "vec", got, a, c)
    for i, n in enumerate(lengths):
        assert not wavd.grad[i, :, n:].any()
        with torch.no_grad():
            alone = nn.discriminator_p(wav[i:i + 1].to(DEV), {k: t.detach() for k, t in wd.items()}, p, [n])[0]
        assert torch.equal(alone, score.detach()[i * p:(i + 1) * p]), ("alone score differs from the batch's", i)
    assert not bad, bad
