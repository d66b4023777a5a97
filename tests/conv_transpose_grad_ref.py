"""Shared by tests/test_conv_transpose_grad_cpu.py and tests/test_gpu_conv_transpose_grad.py (not a test module): what is
nn.conv_transpose1d's own -- the generator's five upsamplers and the other shapes, the phase form of the weight gradient the
kernel uses (for seeding defects) and one generator stage.  The float64 / float32 restatement of the layer (layer_ref with
conv_transpose_op(stride)), the valid masks, the ResBlock chain and the bars are conv_grad_ref's."""
import torch
import torch.nn.functional as F

from conv_grad_ref import (SLOPE, check, compare, k_cap, K_WHOLE, K_CH, layer_ref, conv_transpose_op, valid_masks,  # noqa: F401
                           resblock_chain, mask_of, _ragged, _grad)

# ups[i] of the reference generator (synthdata.VCTK_CONFIG): (Cin, Cout, k, stride), and the input length of each at 28 frames
UPS = [(512, 256, 11, 5), (256, 128, 8, 4), (128, 64, 8, 4), (64, 32, 4, 2), (32, 16, 4, 2)]
UPS_L = [28, 140, 560, 2240, 4480]
OFF_GRID = [(24, 8, 4, 2), (40, 24, 8, 4), (257, 130, 11, 5)]
# the strides no generator layer has, each on a path of its own: s = 1 with Cin > 64 (the data gradient's two-share reduction
# on a slab smaller than the buffer the shares meet in), s = 8 with Cin > 64 (the weight gradient stages half a chunk at a
# time), s = 3 (an odd stride's de-interleave with a two-sided halo)
OTHER_STRIDES = [(128, 64, 3, 1), (96, 24, 8, 8), (72, 40, 9, 3)]


def ups_from_config():
    import synthdata as synth
    cfg = synth.VCTK_CONFIG
    ch, out = cfg["upsample_initial_channel"], []
    for u, k in zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"]):
        out.append((ch, ch // 2, k, u))
        ch //= 2
    return out


def phase_wgrad(xa, gym, k, stride, drop_phase=None, swap=None, plane_shift=None):
    """gw [Cin, Cout, k] in the kernel's phase form: tap kk correlates plane p = (kk - pad) mod stride of gy with
    lrelu(x) shifted by dl = (kk - pad - p) / stride.  xa = lrelu(x) and gym = gy, both already zero beyond the lengths.
    Defects: drop_phase = p (its taps left zero), swap = (p, q) (the two planes exchanged), plane_shift = (p, n) (plane p
    read n positions late)."""
    B, cin, L = xa.shape
    pad = (k - stride) // 2
    planes = [gym[:, :, p::stride] for p in range(stride)]  # [B, Cout, L]
    if swap is not None:
        planes[swap[0]], planes[swap[1]] = planes[swap[1]], planes[swap[0]]
    H = 8
    xp = F.pad(xa, (H, H))
    gw = torch.zeros(cin, gym.shape[1], k, dtype=xa.dtype)
    for kk in range(k):
        p = (kk - pad) % stride
        dl = (kk - pad - p) // stride
        if p == drop_phase:
            continue
        pl = planes[p]
        if plane_shift is not None and plane_shift[0] == p:
            pl = F.pad(pl, (0, plane_shift[1]))[:, :, plane_shift[1]:]
        # sum_q plane_p[co][q] xa[ci][q - dl]
        gw[:, :, kk] = torch.einsum("boq,biq->io", pl, xp[:, :, H - dl:H - dl + L])
    return gw


def stage_ref(wt, bt, stride, w, x, k, dilations, dtype, masks, lengths, gy):
    """one generator stage on the CPU in ``dtype``: conv_transpose1d (wt [Cin, Cout, kt], bt) of lrelu(x), then ResBlock1
    (w: conv_grad_ref.resblock1_ref's dict) on the stride * lengths outputs.  masks: six boolean tensors [B, Cout, stride ld]
    (x > 0 of every ResBlock conv's input, in call order) that replace those leaky ReLUs' branch decisions; the upsampler's
    own leaky ReLU reads x, which is an input.  Returns (y, gx, {name: gradient}) with "ups.weight" / "ups.bias" added."""
    wd = {n: t.detach().to("cpu", dtype).requires_grad_(True) for n, t in dict(w, **{"ups.weight": wt, "ups.bias": bt}).items()}
    up = conv_transpose_op(stride)

    def stage(i, n, xi):
        h = up.apply(F.leaky_relu(xi, SLOPE), wd["ups.weight"], wd["ups.bias"])
        return resblock_chain(h, wd, k, dilations, mask_of(masks, i, stride * n))

    y, gx = _ragged(x.detach().to("cpu", dtype), lengths, gy.detach().to("cpu", dtype), wt.shape[1], up, stage)
    return y, gx, {n: _grad(t) for n, t in wd.items()}
