"""nn.conv1d(..., precision="split_bf16") on the GPU: the handle of dissc_convgrad_create_prec(prec = 1) through the C ABI with
tests/conv_grad_harness.py's conventions (x NaN beyond every length, y a sentinel, the workspace NaN; gy is NaN beyond the
lengths too), held to the float64 split model of tests/conv_split_ref.py.

Per layer, on one ragged batch: which arithmetic ran (the forward's bits are dissc_conv1d_prec's with the HOST packing, so the
device repack is proven; gx is that conv on the transposed, flipped weights times the mask; every result differs from the fp32
handle's and is at least half as far from unsplit float64 as the model is); the error against the model inside the bar of one
split launch (sm.launch_bar: 4 x torch fp32's own error, whole tensor and worst channel / weight row; gb at the fp32 layer's
bar); raggedness; determinism.  Then the layers that fall back per direction, the untouched default, and one ResBlock."""
import ctypes
import types

import numpy as np
import pytest
import torch

import conv_grad_harness as H
import conv_grad_ref as R
import conv_split_ref as cs
import split_bf16_model as sm
from tile_harness import SENTINEL, lib, run_conv  # noqa: F401  (lib: the module fixture that builds the library)

pytestmark = pytest.mark.gpu
DEV = H.DEV
NAMES = ("y", "gx", "gw", "gb")


@pytest.fixture(scope="module")
def nn(lib):
    from dissc_amd import nn
    return nn


# K exceptions by the rule of tests/train_stage_cases.py: K = 2 x the measured worst ratio, rounded up, never above
# min(32, max(4, sqrt(n))), n the chain length of one output, and only for y or gx with n >= 1 024.  (tensor, layer) -> (K whole,
# K worst channel).  Measured on an MI355X (profiles/conv1d_split_bf16.md):
#   gx of 1024 -> 1024 k 5, n = 5 120: whole 2.878, worst channel 5.604 -> 12 (cap 32).  conv_bf3_kernel sums one output's 5 120
#   products (x 3) in ONE fp32 matrix-core chain where torch sums in blocks; the fp32 handle's own gx stands at 4.7 x torch's error.
K_EXCEPTIONS = {("gx", (1024, 1024, 5, 1)): (sm.KERNEL_RATIO, 12.0)}


def k_bars(name, layer):
    cin, cout, k, _ = layer
    kw, kr = K_EXCEPTIONS.get((name, layer), (sm.KERNEL_RATIO, sm.KERNEL_RATIO))
    n = {"y": cin * k, "gx": cout * k}.get(name, 0)
    assert max(kw, kr) <= sm.KERNEL_RATIO or (name in ("y", "gx") and n >= 1024 and max(kw, kr) <= R.k_cap(n)), (name, layer)
    return kw, kr


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def run_abi(nn, layer, x, w, b, gy, lengths, prec, slope=cs.SLOPE):
    """set_weights, forward and backward of the (prec) handle of ``layer`` on device tensors; y starts as the sentinel, gx as
    NaN, the workspace as NaN bytes.  -> (y, gx, gw, gb) on the device, (P, pairs, workspace bytes)"""
    cin, cout, k, d = layer
    B, _, ld = x.shape
    h = nn._handle(nn.CONV1D, cin, cout, k, d, torch.device(DEV), prec=prec)
    ln = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    K = nn.CONV1D
    nn.check(K.set_weights(h, _ptr(w), _ptr(b), None), "set_weights")
    y = torch.full((B, cout, ld), SENTINEL, device=DEV)
    nn.check(K.forward(h, _ptr(x), None, _ptr(y), _ptr(ln), B, ld, ld, ld, slope, None), "forward")
    P, pairs = ctypes.c_int(0), ctypes.c_int(0)
    nn.check(K.partials(h, B, ld, ctypes.byref(P), ctypes.byref(pairs)), "partials")
    nws = int(K.workspace_bytes(h, B, ld))
    ws = torch.full((nws,), 255, dtype=torch.uint8, device=DEV)
    gx = torch.full((B, cin, ld), float("nan"), device=DEV)
    gw = torch.full((cout, cin, k), float("nan"), device=DEV)
    gb = torch.full((cout,), float("nan"), device=DEV)
    nn.check(K.backward(h, _ptr(x), _ptr(gy), _ptr(ln), B, ld, ld, ld, slope, _ptr(gx), _ptr(gw), _ptr(gb), _ptr(ws), nws, None), "backward")
    torch.cuda.synchronize()
    return (y, gx, gw, gb), (P.value, pairs.value, nws)


def _beyond(lengths, ld):
    m = torch.zeros(len(lengths), 1, ld, dtype=torch.bool)
    for i, n in enumerate(lengths):
        m[i, :, n:] = True
    return m


@pytest.mark.parametrize("layer", cs.LAYERS, ids=lambda l: "%d-%d-k%d-d%d" % l)
def test_split_layer(lib, nn, layer):
    cin, cout, k, d = layer
    x, w, b, gy, lengths, ld = cs.inputs(lib, layer)
    model, r64, r32 = cs.references(x, w, b, gy, lengths, d)
    dev = [t.to(DEV) for t in (x, w, b, gy)]
    got_dev, plan = run_abi(nn, layer, *dev, lengths, prec=1)
    got = [t.cpu() for t in got_dev]
    beyond = _beyond(lengths, ld)
    print(f"\nCSB {layer}: lengths {lengths}, ld {ld}, tile widths {cs.tile_widths(lib, *layer, len(lengths), ld)}, plan {plan}")

    # 3. raggedness: the sentinel survives, gx is zero from lengths[b] on, no NaN anywhere in the gradients
    assert (got[0][beyond.expand_as(got[0])] == SENTINEL).all(), "the forward wrote beyond a length"
    assert not got[1][beyond.expand_as(got[1])].any(), "gx is not zero beyond a length"
    for name, t in zip(NAMES[1:], got[1:]):
        assert torch.isfinite(t).all(), name
    y = torch.where(beyond.expand_as(got[0]), torch.zeros(()), got[0])
    assert torch.isfinite(y).all()
    held = [y] + got[1:]

    # 1. which arithmetic ran
    assert nn.conv1d_precision(*layer) == (True, True, True)
    y_diag = run_conv(lib, dev[0], w, b, lengths, k, d, cs.SLOPE, Lmax=ld, prec=1).cpu()
    assert torch.equal(got[0], y_diag), "the forward is not dissc_conv1d_prec(prec = 1) on the host packing"
    wt = w.transpose(0, 1).flip(2).contiguous()
    gx_raw = run_conv(lib, dev[3], wt, torch.zeros(cin), lengths, k, d, 1.0, Lmax=ld, prec=1).cpu()
    xz = torch.nan_to_num(x)
    gx_want = torch.where(beyond.expand_as(gx_raw), torch.zeros(()), torch.where(xz > 0, gx_raw, gx_raw * torch.tensor(cs.SLOPE)))
    assert torch.equal(got[1], gx_want), "gx is not the split conv of gy on the transposed, flipped weights, masked"
    fp32 = [t.cpu() for t in run_abi(nn, layer, *dev, lengths, prec=0)[0]]
    fp32[0] = torch.where(beyond.expand_as(fp32[0]), torch.zeros(()), fp32[0])
    for j, name in enumerate(NAMES[:3]):
        assert not torch.equal(held[j], fp32[j]), f"{name} has the fp32 handle's bits"
        e_model, e_got = cs.rel_rms(model[j], r64[j]), cs.rel_rms(held[j], r64[j])
        print(f"CSB {layer} {name}: to unsplit float64 {e_got:.3e}, the model's {e_model:.3e}, the fp32 handle's {cs.rel_rms(fp32[j], r64[j]):.3e}")
        assert e_got >= 0.5 * e_model, (name, e_got, e_model)
    assert torch.equal(held[3], fp32[3]), "the bias gradient is the fp32 layer's"

    # 2. error against the split model
    bad = []
    for j, name in enumerate(NAMES[:3]):
        kw, kr = k_bars(name, layer)
        v, fig = cs.bars(name, held[j], model[j], r64[j], r32[j], kw, kr)
        print(f"CSB {layer} {name}: e {fig['e']:.3e} against the model, torch fp32 {fig['e_fp32']:.3e}, ratio {fig['ratio']:.3f} (bar {kw:g}) | "
              f"worst channel / row {fig['worst_row_ratio']:.3f} (bar {kr:g})")
        bad += v
    bad += R.check(f"{layer} gb", "vec", held[3], r64[3], r32[3])
    assert not bad, bad

    # 4. determinism: equal bits again; every utterance's gx alone; P and the workspace do not depend on lengths
    again, plan2 = run_abi(nn, layer, *dev, lengths, prec=1)
    for name, t, q in zip(NAMES, got, again):
        assert torch.equal(t, q.cpu()), f"{name} is not bit-reproducible"
    shorter = [min(n, 3) for n in lengths]
    assert run_abi(nn, layer, *dev, shorter, prec=1)[1] == plan == plan2
    for i, n in enumerate(lengths):
        if n > 0:
            sl = slice(i, i + 1)
            alone = run_abi(nn, layer, dev[0][sl].contiguous(), dev[1], dev[2], dev[3][sl].contiguous(), [n], prec=1)[0]
            assert torch.equal(alone[1].cpu(), got[1][sl]), ("alone gx differs from the batch's", i, n)


class _Split:
    """dissc_amd.nn with conv1d at precision="split_bf16", for conv_grad_harness.run"""

    def __init__(self, nn):
        self._nn = nn

    def __getattr__(self, name):
        return getattr(self._nn, name)

    def conv1d(self, *a, **kw):
        return self._nn.conv1d(*a, precision="split_bf16", **kw)


MIXED = [(16, 16, 3, 1), (32, 1, 7, 1), (32, 32, 7, 12)]


@pytest.mark.parametrize("layer", MIXED, ids=lambda l: "%d-%d-k%d-d%d" % l)
def test_fp32_directions_keep_the_default_bits(nn, layer):
    cin, cout, k, d = layer
    spec = H.Spec("conv1d", cin, cout, k, d)
    lengths = [0, 1, (k - 1) * d // 2 + 1, 63, 64, 65, 129, 132]
    x, w, b, gy = H.case(spec, len(lengths), 132, seed=7)
    fwd, dgrad, wgrad = nn.conv1d_precision(*layer)
    assert (fwd, dgrad, wgrad) != (True, True, True)
    default = H.run(nn, spec, x, w, b, gy, lengths, cs.SLOPE)
    split = H.run(_Split(nn), spec, x, w, b, gy, lengths, cs.SLOPE)
    for name, is_split, a, c in zip(NAMES, (fwd, dgrad, wgrad, False), default, split):
        print(f"CSB mixed {layer} {name}: {'split' if is_split else 'fp32'}, bits {'differ' if not torch.equal(a, c) else 'equal'}")
        if not is_split:
            assert torch.equal(a, c), f"{name} runs fp32 and must have the default call's bits"
        else:
            assert not torch.equal(a, c), f"{name} is reported split but has the fp32 bits"


def test_default_untouched_beside_a_split_handle(nn):
    spec = H.Spec("conv1d", 32, 32, 3, 1)
    lengths = [1, 17, 64, 65, 129, 132]
    x, w, b, gy = H.case(spec, len(lengths), 132, seed=11)
    before = H.run(nn, spec, x, w, b, gy, lengths, cs.SLOPE)
    split = H.run(_Split(nn), spec, x, w, b, gy, lengths, cs.SLOPE)
    explicit = H.run(types.SimpleNamespace(conv1d=lambda *a, **kw: nn.conv1d(*a, precision="fp32", **kw), conv_transpose1d=None,
                                           conv1d_strided=None, conv1d_grouped=None), spec, x, w, b, gy, lengths, cs.SLOPE)
    after = H.run(nn, spec, x, w, b, gy, lengths, cs.SLOPE)
    for name, a, e, c, s in zip(NAMES, before, explicit, after, split):
        assert torch.equal(a, e) and torch.equal(a, c), f'{name}: precision="fp32" / the default after a split call changed bits'
        assert name == "gb" or not torch.equal(a, s), f"{name}: the split call has the default's bits (one handle for both?)"


def test_resblock1_split(nn):
    """nn.resblock1 at C = 32, k = 7 on 3 utterances of 40, 64 and 65 columns against float64 autograd on the unsplit operands:
    sm.block_bar(chained model's error, torch fp32's error) for y, gx and the twelve parameter gradients; the leaky-ReLU masks are
    the engine's own, as tests/conv_grad_ref.py takes them."""
    C, k, dil, lengths, ld = 32, 7, (1, 3, 5), [40, 64, 65], 68
    rs = np.random.RandomState(5)
    x = torch.from_numpy(rs.randn(3, C, ld).astype(np.float32))
    gy = torch.from_numpy(rs.randn(3, C, ld).astype(np.float32))
    for i, n in enumerate(lengths):
        x[i, :, n:] = 0.0
        gy[i, :, n:] = 0.0
    w = {}
    for m in range(3):
        for grp in ("convs1", "convs2"):
            w[f"{grp}.{m}.weight"] = torch.from_numpy((rs.uniform(-1, 1, (C, C, k)) / np.sqrt(C * k)).astype(np.float32))
            w[f"{grp}.{m}.bias"] = torch.from_numpy(rs.uniform(-0.1, 0.1, C).astype(np.float32))
    assert all(nn.conv1d_precision(C, C, k, d) == (True, True, True) for d in dil + (1,))
    xd = x.to(DEV).requires_grad_(True)
    wd = {n: t.to(DEV).requires_grad_(True) for n, t in w.items()}
    ln = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    taps = []
    y = nn.resblock1(xd, wd, k, dil, lengths=ln, taps=taps, precision="split_bf16")
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    masks = [t.detach() > 0 for t in taps]
    own = []
    R.resblock1_ref(w, x, k, dil, torch.float64, lengths=lengths, taps=own)
    valid = ~_beyond(lengths, ld)
    flips = [int((((o > 0) != m.cpu()) & valid).sum()) for o, m in zip(own, masks)]
    print(f"\nCSB resblock1: positions where float64's own sign differs from the engine's, per conv input: {flips}")
    y64, gx64, g64 = R.resblock1_ref(w, x, k, dil, torch.float64, masks=masks, lengths=lengths, gy=gy)
    y32, gx32, g32 = R.resblock1_ref(w, x, k, dil, torch.float32, masks=masks, lengths=lengths, gy=gy)
    ym, gxm, gm = cs.resblock1(x, w, k, dil, gy, lengths, masks)
    bad = []
    cases = [("y", y.detach().cpu(), ym, y64, y32), ("gx", xd.grad.cpu(), gxm, gx64, gx32)]
    cases += [(n, wd[n].grad.cpu(), gm[n], g64[n], g32[n]) for n in w]
    assert len(cases) == 14
    for name, got, mod, r64, r32 in cases:
        e, em, e32 = cs.rel_rms(got, r64), cs.rel_rms(mod, r64), cs.rel_rms(r32, r64)
        bar = sm.block_bar(em, e32)
        print(f"CSB resblock1 {name:16s}: {e:.3e} to float64, model {em:.3e}, torch fp32 {e32:.3e}, {e / bar:.2f} of the bar")
        assert torch.isfinite(got).all()
        if not e <= bar:
            bad.append((name, e, em, e32))
    assert not bad, bad
