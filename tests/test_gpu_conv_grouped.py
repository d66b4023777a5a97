"""dissc_amd.nn.conv1d_grouped, nn.mean_pool and nn.discriminator_s on the GPU: the device-side packings bit for bit against a host
packing, every gradient of the layer against torch in float64 under the bars of tests/train_stage_cases.py (ragged INPUT lengths
around the stride, the halo, the chunk and a partial boundary; the six grouped layers of DiscriminatorS at full channel count and
three small shapes), the layers at the trainer's row lengths, the pool against its stated fp32 expression, and DiscriminatorS end
to end against its float64 restatement.  Measured ratios: profiles/conv_grouped_grad.md."""
import functools

import numpy as np
import pytest
import torch

import conv_grad_harness as H
import conv_grouped_ref as R

pytestmark = pytest.mark.gpu
DEV = H.DEV


@pytest.fixture(scope="module")
def nn():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import nn
    return nn


# ---- the packings -------------------------------------------------------------------------------------------------------
def _host_packing(w, which, g):
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
    H.assert_device_packing(nn, H.Spec("grouped", cin, cout, k, s, g), functools.partial(_host_packing, g=g))


# ---- the layer ----------------------------------------------------------------------------------------------------------
# Exceptions to K = 4 (tests/train_stage_cases.py's rule, as tests/test_gpu_conv_strided_grad.py's K_EXC: only for y or gx, only
# where one output is ONE sequential fp32 chain of n >= 1 024 products in a matrix-core accumulator; K = 2 x the measured worst
# ratio over every case of this file, rounded up, never above min(32, max(4, sqrt(n)))).  (tensor, Cin, Cout, k, s, g) -> (whole,
# worst channel).  The weight and bias gradients get none.
# None is needed: the kernels keep four accumulators per output and add them in a fixed order, so the longest chain of one
# output is 2 624 / 4 = 656 products (convs.5, y and gx), below the rule's 1 024; every measured ratio is in
# profiles/conv_grouped_grad.md.
K_EXC = {}  # the rule: H.k_bars


@pytest.mark.parametrize("cin,cout,k,s,g", R.DISC_S + R.SMALL)
def test_layer_gradients_against_float64(nn, cin, cout, k, s, g):
    spec = H.Spec("grouped", cin, cout, k, s, g)
    lengths, ld, plan = H.lengths_for(nn, spec, max_b=4 if cout >= 1024 else None)
    print(f"\nlayer {spec}: lengths {lengths}, ld {ld}, (P, pairs) {plan}")
    H.assert_layer_gradients(H.gpu_run(nn, spec), spec, lengths, ld, 7 * cin + k + s, H.k_bars(K_EXC, "y", spec),
                             H.k_bars(K_EXC, "gx", spec))


@pytest.mark.parametrize("layer", range(6))
def test_training_shape(nn, layer):
    """2 x 2 rows at the layer's own scale-0 row length, two rows shorter: the kernels' tile walk over a long row; the four bars,
    every result bit-reproducible"""
    (cin, cout, k, s, g), L = R.DISC_S[layer], R.TRAIN_L[layer]
    spec, lengths = H.Spec("grouped", cin, cout, k, s, g), [L, L // 2 + 1, L, max(1, L // 3)]
    print(f"\ntraining shape {cin} -> {cout} L {L}: plan {spec.partials(nn, 4, R.ceil4(L))}")
    H.assert_training_shape(H.gpu_run(nn, spec), spec, lengths, R.ceil4(L), L + k, H.k_bars(K_EXC, "y", spec),
                            H.k_bars(K_EXC, "gx", spec))


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
    H.disc_loss(fmaps, [h.to(DEV) for h in hats], [m.to(DEV) for m in masks]).backward()
    torch.cuda.synchronize()
    for j, (ln, m) in enumerate(zip(lens, masks)):
        assert ln.cpu().tolist() == [R.map_lengths(n)[j] for n in lengths] == m[:, 0].sum(1).long().tolist()

    ref = {}
    for dtype in (torch.float64, torch.float32):
        wr = {n: t.to(dtype).requires_grad_(True) for n, t in w.items()}
        wavr = wav.to(dtype).requires_grad_(True)
        maps = R.disc_s_ragged(wr, wavr, lengths)
        H.disc_loss(maps, [h.to(dtype) for h in hats], [m.to(dtype) for m in masks]).backward()
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
