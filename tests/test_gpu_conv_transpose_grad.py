"""dissc_amd.nn.conv_transpose1d on the GPU: the device-side packings bit for bit against dissc_conv_transpose1d on host
weights, every gradient of the layer against torch in float64 under the bars of tests/train_stage_cases.py (ragged input
lengths around the chunk and a partial boundary; the five upsamplers, shapes off the 32 grid and the strides 1, 3 and 8 that
no generator layer has; the training shapes at B = 32), and one generator stage (the upsampler
followed by resblock1) against the float64 stage evaluated with the engine's own branch decisions.  Measured ratios:
profiles/conv_transpose_grad.md."""
import ctypes

import numpy as np
import pytest
import torch

import conv_grad_harness as H
import conv_transpose_grad_ref as R

pytestmark = pytest.mark.gpu
DEV = H.DEV


@pytest.fixture(scope="module")
def nn():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import nn
    return nn


def _conv_transpose1d_host(x, w, b, lengths, s, slope):
    """dissc_conv_transpose1d: host weights packed on the host"""
    from dissc_amd import _lib
    B, cin, ld = x.shape
    _, cout, k = w.shape
    xd, y = x.to(DEV), torch.zeros(B, cout, s * ld, device=DEV)
    wc = w.contiguous()
    ln = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib.dissc_conv_transpose1d(xd.data_ptr(), wc.data_ptr(), None if b is None else b.data_ptr(), y.data_ptr(),
                                               ln.data_ptr(), B, cin, cout, k, s, ld, s * ld, ld, ctypes.c_float(slope), None),
               "dissc_conv_transpose1d")
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("cin,cout,k,s", R.UPS + R.OFF_GRID + R.OTHER_STRIDES)
def test_device_packing_bit_for_bit(nn, cin, cout, k, s):
    B, ld, lengths, slope = 3, 100, [100, 37, 3], 0.1
    spec = H.Spec("transposed", cin, cout, k, s)
    x, w, b, gy = H.case(spec, B, ld, seed=cin + k)
    y = H.gpu_run(nn, spec)(x, w, b, gy, lengths, slope)[0]
    host = _conv_transpose1d_host(x, w, b, lengths, s, slope)
    assert torch.equal(y, host)
    assert host[0].abs().min() > 0 and not host[2, :, s * 3:].any()
    # without a bias: the replicated bias rows are rewritten as zeros, not left over from the call above
    y0 = H.gpu_run(nn, spec)(x, w, None, gy, lengths, slope)[0]
    assert torch.equal(y0, _conv_transpose1d_host(x, w, None, lengths, s, slope))


# Exceptions to K = 4 (tests/train_stage_cases.py's rule: only where one output is ONE sequential fp32 chain of n >= 1 024
# products in a matrix-core accumulator while torch sums in SIMD-wide blocks; K = 2 x the measured worst ratio, rounded up,
# never above min(32, max(4, sqrt(n)))).  (tensor, Cin, Cout, k, s) -> (whole, worst channel); measured on an MI355X over
# every case of this file (profiles/conv_transpose_grad.md).  The weight and bias gradients get no exception.
#   data gradient of ups.0, n = 256 x 11 = 2 816: 3.66 / 3.30 (ragged batch, one chain), 2.30 / 1.61 (B = 32 at 28 columns,
#   two chains of 1 408)  ->  8 / 7 (cap 32)
# The other candidates stay at 4: the forward of ups.0 (n = 1 536) measured 1.12 / 1.09 and 2.41 / 2.53, the data gradients
# of ups.1 (n = 1 024) 2.52 / 2.40 and of 257 -> 130, k = 11 (n = 1 430) 2.68 / 2.64.
K_EXC = {("gx", 512, 256, 11, 5): (8.0, 7.0)}  # the rule: H.k_bars


@pytest.mark.parametrize("cin,cout,k,s", R.UPS + R.OFF_GRID + R.OTHER_STRIDES)
def test_layer_gradients_against_float64(nn, cin, cout, k, s):
    spec = H.Spec("transposed", cin, cout, k, s)
    lengths, ld, plan = H.lengths_for(nn, spec)
    print(f"\nlayer {spec}: lengths {lengths}, ld {ld}, (P, pairs) {plan}")
    H.assert_layer_gradients(H.gpu_run(nn, spec), spec, lengths, ld, 7 * cin + k + s, H.k_bars(K_EXC, "y", spec),
                             H.k_bars(K_EXC, "gx", spec))


TRAIN = [(512, 256, 11, 5, 28), (32, 16, 4, 2, 4480)]


@pytest.mark.parametrize("cin,cout,k,s,L", TRAIN)
def test_training_shapes(nn, cin, cout, k, s, L):
    """B = 32 at the generator's own lengths (28 frames): the widest upsampler at 28 input positions, and the longest
    reduction, 32 x 4 480, of the narrowest"""
    spec = H.Spec("transposed", cin, cout, k, s)
    print(f"\ntraining shape {spec} L {L}: plan {spec.partials(nn, 32, L)}")
    H.assert_training_shape(H.gpu_run(nn, spec), spec, H.training_lengths(32, L, (1, 5, 17, 31)), L, L + k,
                            H.k_bars(K_EXC, "y", spec), H.k_bars(K_EXC, "gx", spec))


def test_stage_against_float64_with_the_engines_masks(nn):
    """one generator stage: conv_transpose1d (64 -> 32, k 4, s 2) followed by resblock1 (C 32, k 7), ragged, the gradient
    taken through both"""
    cin, C, kt, s, k, dil = 64, 32, 4, 2, 7, (1, 3, 5)
    lengths, ld = [1, 5, 31, 32, 33, 66], 68
    B = len(lengths)
    rs = np.random.RandomState(11)
    w = {}
    for m in range(3):
        for c in ("convs1", "convs2"):
            w[f"{c}.{m}.weight"] = torch.from_numpy((rs.uniform(-1, 1, (C, C, k)) / np.sqrt(C * k)).astype(np.float32))
            w[f"{c}.{m}.bias"] = torch.from_numpy((rs.uniform(-1, 1, C) / np.sqrt(C * k)).astype(np.float32))
    wt = torch.from_numpy((rs.uniform(-1, 1, (cin, C, kt)) / np.sqrt(cin * kt / s)).astype(np.float32))
    bt = torch.from_numpy((rs.uniform(-1, 1, C) / np.sqrt(cin * kt)).astype(np.float32))
    x = torch.from_numpy(rs.randn(B, cin, ld).astype(np.float32))
    vi, vo = R.valid_masks(lengths, ld, R.conv_transpose_op(s))
    # the cotangent of an output that is never written: zero (the residual hands it through unmasked)
    gy = torch.from_numpy(rs.randn(B, C, s * ld).astype(np.float32)) * vo
    wd = {n: t.to(DEV).requires_grad_(True) for n, t in w.items()}
    wtd, btd = wt.to(DEV).requires_grad_(True), bt.to(DEV).requires_grad_(True)
    xd = x.to(DEV).requires_grad_(True)
    ln = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    ln_out = torch.tensor([s * n for n in lengths], dtype=torch.int32, device=DEV)
    taps = []
    up = nn.conv_transpose1d(xd, wtd, btd, stride=s, lengths=ln, in_slope=R.SLOPE)
    y = nn.resblock1(up, wd, k, dil, lengths=ln_out, taps=taps)
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    assert len(taps) == 6
    masks = [t.detach().cpu() > 0 for t in taps]
    y64, gx64, g64 = R.stage_ref(wt, bt, s, w, x, k, dil, torch.float64, masks, lengths, gy)
    y32, gx32, g32 = R.stage_ref(wt, bt, s, w, x, k, dil, torch.float32, masks, lengths, gy)
    bad = R.check("stage y", "act", y.detach(), y64, y32)
    bad += R.check("stage gx", "act", xd.grad, gx64, gx32)
    got = dict(wd, **{"ups.weight": wtd, "ups.bias": btd})
    for n in sorted(got):
        bad += R.check("stage grad " + n, "weight" if n.endswith("weight") else "vec", got[n].grad, g64[n], g32[n])
    assert not bad, bad
    assert not xd.grad.cpu()[(vi == 0).expand(B, cin, ld)].any()
    assert not y.detach().cpu()[(vo == 0).expand(B, C, s * ld)].any()
