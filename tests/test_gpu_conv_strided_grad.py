"""dissc_amd.nn.conv1d_strided, nn.period_fold and nn.discriminator_p on the GPU: the device-side packings bit for bit against a
host packing, every gradient of the layer against torch in float64 under the bars of tests/train_stage_cases.py (ragged INPUT
lengths around the stride, the chunk and a partial boundary; the four strided layers of DiscriminatorP and two other (k, stride)),
the discriminator's own row lengths at 22 rows, the fold against torch's reflect pad and view, and DiscriminatorP end to end
against its float64 Conv2d restatement.  Measured ratios: profiles/conv_strided_grad.md."""
import numpy as np
import pytest
import torch

import conv_grad_harness as H
import conv_strided_ref as R

pytestmark = pytest.mark.gpu
DEV = H.DEV


@pytest.fixture(scope="module")
def nn():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import nn
    return nn


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
    H.assert_device_packing(nn, H.Spec("strided", cin, cout, k, s), _host_packing)


# ---- the layer ----------------------------------------------------------------------------------------------------------
# Exceptions to K = 4 (tests/train_stage_cases.py's rule, as tests/test_gpu_conv_transpose_grad.py's K_EXC: only where one output
# is ONE sequential fp32 chain of n >= 1 024 products in a matrix-core accumulator; never above min(32, max(4, sqrt(n)))).
# (tensor, Cin, Cout, k, s) -> (whole, worst channel); K = 2 x the measured worst ratio over every case of this file, rounded up;
# measured on an MI355X (profiles/conv_strided_grad.md).  The weight and bias gradients get no exception.
#   forward of convs.3, n = 512 x 5 = 2 560 in one chain: 2.95 / 4.88 (ragged batch)  ->  6 / 10 (cap 32)
# The other candidates stay at 4: the data gradients of convs.3 (n = 1 024 x 2) and convs.2 (n = 512 x 2) measured 1.05 / 1.03
# and 1.02 / 1.02.
K_EXC = {("y", 512, 1024, 5, 3): (6.0, 10.0)}  # the rule: H.k_bars


@pytest.mark.parametrize("cin,cout,k,s", R.DISC_P + R.TAP_TABLE)
def test_layer_gradients_against_float64(nn, cin, cout, k, s):
    spec = H.Spec("strided", cin, cout, k, s)
    lengths, ld, plan = H.lengths_for(nn, spec, max_b=4 if cin * cout >= 512 * 1024 else None)
    print(f"\nlayer {spec}: lengths {lengths}, ld {ld}, (P, pairs) {plan}")
    H.assert_layer_gradients(H.gpu_run(nn, spec), spec, lengths, ld, 7 * cin + k + s, H.k_bars(K_EXC, "y", spec),
                             H.k_bars(K_EXC, "gx", spec))


TRAIN_L = [815, 272, 91, 31]  # the rows of DiscriminatorP(11) on 8 960 samples, layer by layer


@pytest.mark.parametrize("layer", range(4))
def test_training_shape(nn, layer):
    """22 rows (B = 2, period 11) at the discriminator's own row lengths, one layer each, two rows shorter: the four bars, every
    result bit-reproducible"""
    (cin, cout, k, s), L = R.DISC_P[layer], TRAIN_L[layer]
    assert L == (R.cdiv(8960, 11) if layer == 0 else R.cdiv(TRAIN_L[layer - 1], 3))
    spec, lengths = H.Spec("strided", cin, cout, k, s), [L] * 22
    lengths[3], lengths[20] = L // 2 + 1, max(1, L // 3)
    print(f"\ntraining shape {cin} -> {cout} L {L}: plan {spec.partials(nn, 22, R.ceil4(L))}")
    H.assert_training_shape(H.gpu_run(nn, spec), spec, lengths, R.ceil4(L), L + k, H.k_bars(K_EXC, "y", spec),
                            H.k_bars(K_EXC, "gx", spec))


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
    H.disc_loss(fmaps, [h.to(DEV) for h in hats], [m.to(DEV) for m in masks]).backward()
    torch.cuda.synchronize()
    for ln, m in zip(lens, masks):
        assert torch.equal(ln.cpu().long(), m[:, 0].sum(1).long())

    ref = {}
    for dtype in (torch.float64, torch.float32):
        wr = {n: t.to(dtype).requires_grad_(True) for n, t in w.items()}
        wavr = wav.to(dtype).requires_grad_(True)
        maps = R.disc_p_conv2d(wr, wavr, p, lengths)
        H.disc_loss(maps, [h.to(dtype) for h in hats], [m.to(dtype) for m in masks]).backward()
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
