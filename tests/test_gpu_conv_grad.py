"""dissc_amd.nn on the GPU: the device-side packings bit for bit against dissc_conv1d on host weights, every gradient of
the layer against torch in float64 under the bars of tests/train_stage_cases.py (ragged lengths around the padding, the
chunk and a partial boundary; the training shapes at B = 32), and resblock1 against the float64 block evaluated with
the engine's own branch decisions.  Measured ratios: profiles/conv_grad.md."""
import ctypes

import numpy as np
import pytest
import torch

import conv_grad_harness as H
import conv_grad_ref as R

pytestmark = pytest.mark.gpu
DEV = H.DEV


@pytest.fixture(scope="module")
def nn():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import nn
    return nn


def _conv1d_host(x, w, b, lengths, d, slope):
    """dissc_conv1d: host weights packed on the host"""
    from dissc_amd import _lib
    B, cin, ld = x.shape
    cout, _, k = w.shape
    xd, y = x.to(DEV), torch.zeros(B, cout, ld, device=DEV)
    wc = w.contiguous()
    ln = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib.dissc_conv1d(xd.data_ptr(), wc.data_ptr(), None if b is None else b.data_ptr(), y.data_ptr(), ln.data_ptr(),
                                     B, cin, cout, k, d, ld, ld, ld, ctypes.c_float(slope), None), "dissc_conv1d")
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("cin,cout,k,d,slope", [(16, 16, 11, 5, 0.1), (32, 32, 7, 3, 0.1), (64, 64, 3, 1, 0.1), (257, 512, 7, 1, 1.0),
                                                (16, 1, 7, 1, 0.01)])
def test_device_packing_bit_for_bit(nn, cin, cout, k, d, slope):
    B, ld, lengths = 3, 100, [100, 37, 3]
    spec = H.Spec("conv1d", cin, cout, k, d)
    x, w, b, gy = H.case(spec, B, ld, seed=cin + k)
    y, gx, _, _, _ = H.gpu_run(nn, spec)(x, w, b, gy, lengths, slope)
    assert torch.equal(y, _conv1d_host(x, w, b, lengths, d, slope))
    wt = w.transpose(0, 1).flip(2).contiguous()  # [Cin][Cout][k], taps flipped
    plain = _conv1d_host(gy, wt, None, lengths, d, 1.0)  # the data gradient before the mask
    assert torch.equal(gx, plain * torch.where(x > 0, torch.tensor(1.0), torch.tensor(np.float32(slope))))
    assert plain.abs().sum() > 0


LAYERS = [(16, 16, 3, 1), (16, 16, 11, 5), (32, 32, 7, 3), (64, 64, 11, 5), (128, 128, 3, 3), (256, 256, 7, 1), (257, 512, 7, 1),
          (16, 1, 7, 1)]


@pytest.mark.parametrize("cin,cout,k,d", LAYERS)
def test_layer_gradients_against_float64(nn, cin, cout, k, d):
    spec = H.Spec("conv1d", cin, cout, k, d)
    lengths, ld, plan = H.lengths_for(nn, spec)
    print(f"\nlayer {spec}: lengths {lengths}, ld {ld}, (P, pairs) {plan}")
    H.assert_layer_gradients(H.gpu_run(nn, spec), spec, lengths, ld, 7 * cin + k + d, H.k_bars(K_DIRECT, "y", spec),
                             H.k_bars(K_DIRECT, "gx", spec))


# The one exception to K = 4 (tests/train_stage_cases.py's rule): the forward and the data gradient are the direct conv
# kernels (conv_mfma32_kernel / conv_mfma_kernel), where every output is ONE fp32 chain of n = Cin k (forward) or Cout k
# (data gradient) products in a matrix-core accumulator and torch sums in SIMD-wide blocks -- the exception that file
# records for conv_fwd.  K = 2 x the measured worst ratio, rounded up, never above min(32, max(4, sqrt(n))); measured on
# an MI355X over every case of this file (profiles/conv_grad.md).  Chains below 1 024 products, the weight and bias
# gradients and the whole of resblock1 stay at 4.
# Measured worst ratios (whole / worst channel) and the K they give:
#   n = 3 584 (data gradient of 257 -> 512, k = 7): 4.55 / 4.77 (ragged batch), 4.14 / 4.31 (B = 32)  -> 10 / 10 (cap 32)
#   n = 2 816 (256 -> 256, k = 11, B = 32):          forward 3.11 / 4.70, data gradient 3.78 / 3.81  ->  4 / 10 (cap 32)
#   n = 1 799 (forward of 257 -> 512, k = 7):        2.40 / 3.54 (ragged batch), 2.03 / 4.06 (B = 32) ->  4 / 9  (cap 32)
K_DIRECT = {3584: (10.0, 10.0), 2816: (4.0, 10.0), 1799: (4.0, 9.0)}  # n -> (whole, worst channel); the rule: H.k_bars

TRAIN = [(16, 16, 11, 5, 8960), (256, 256, 11, 5, 140), (257, 512, 7, 1, 28)]


@pytest.mark.parametrize("cin,cout,k,d,L", TRAIN)
def test_training_shapes(nn, cin, cout, k, d, L):
    """B = 32 at the generator's own lengths (28 frames): the 286 720-long reduction of the narrowest stage, the widest
    ResBlock layer, conv_pre"""
    spec = H.Spec("conv1d", cin, cout, k, d)
    print(f"\ntraining shape {spec} L {L}: plan {spec.partials(nn, 32, L)}")
    H.assert_training_shape(H.gpu_run(nn, spec), spec, H.training_lengths(32, L, (1, 5, 17, 31)), L, L + k,
                            H.k_bars(K_DIRECT, "y", spec), H.k_bars(K_DIRECT, "gx", spec))


@pytest.mark.parametrize("C,k", [(32, 7), (16, 11)])
def test_resblock1_against_float64_with_the_engines_masks(nn, C, k):
    lengths, ld, dil = [1, 5, 63, 64, 65, 131], 132, (1, 3, 5)
    B = len(lengths)
    rs = np.random.RandomState(C + k)
    w = {}
    for m in range(3):
        for c in ("convs1", "convs2"):
            w[f"{c}.{m}.weight"] = torch.from_numpy((rs.uniform(-1, 1, (C, C, k)) / np.sqrt(C * k)).astype(np.float32))
            w[f"{c}.{m}.bias"] = torch.from_numpy((rs.uniform(-1, 1, C) / np.sqrt(C * k)).astype(np.float32))
    x = torch.from_numpy(rs.randn(B, C, ld).astype(np.float32))
    valid = torch.zeros(B, 1, ld, dtype=torch.bool)
    for i, n in enumerate(lengths):
        valid[i, :, :n] = True
    # the cotangent of an output that is never written: zero (the residual hands it through unmasked, as the gradient of add)
    gy = torch.from_numpy(rs.randn(B, C, ld).astype(np.float32)) * valid
    wd = {n: t.to(DEV).requires_grad_(True) for n, t in w.items()}
    xd = x.to(DEV).requires_grad_(True)
    taps = []
    y = nn.resblock1(xd, wd, k, dil, lengths=torch.tensor(lengths, dtype=torch.int32, device=DEV), taps=taps)
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    assert len(taps) == 6
    masks = [t.detach().cpu() > 0 for t in taps]
    own = []
    y64, gx64, g64 = R.resblock1_ref(w, x, k, dil, torch.float64, masks=masks, lengths=lengths, gy=gy)
    y32, gx32, g32 = R.resblock1_ref(w, x, k, dil, torch.float32, masks=masks, lengths=lengths, gy=gy)
    R.resblock1_ref(w, x, k, dil, torch.float64, lengths=lengths, taps=own)
    differ = sum(int((((t > 0) != m) & valid).sum()) for t, m in zip(own, masks))
    print(f"\nresblock1 C {C} k {k}: mask positions where float64's own sign differs: {differ} of {6 * int(valid.sum()) * C}")
    block = H.Spec("conv1d", C, C, k, 1)  # every conv of the block: chains of C k products
    bad = R.check("block y", "act", y.detach(), y64, y32, *H.k_bars(K_DIRECT, "y", block))
    bad += R.check("block gx", "act", xd.grad, gx64, gx32, *H.k_bars(K_DIRECT, "gx", block))
    for n in sorted(w):
        bad += R.check("block grad " + n, "weight" if n.endswith("weight") else "vec", wd[n].grad, g64[n], g32[n])
    assert not bad, bad
    assert not xd.grad.cpu()[(~valid).expand(B, C, ld)].any()
