"""Shared by tests/test_conv_grouped_cpu.py and tests/test_gpu_conv_grouped.py (not a test module): what is nn.conv1d_grouped's,
nn.mean_pool's and nn.discriminator_s's own -- the layer table of the scale discriminator, the average pool, and DiscriminatorS
restated both as torch's grouped Conv1d chain on one utterance and as the ragged composition the library runs.  The float64 /
float32 restatement of the layer (layer_ref with strided_op(stride, groups)), its phase form, the masks and the bars are
conv_grad_ref's."""
import numpy as np
import torch
import torch.nn.functional as F

from conv_grad_ref import (SLOPE, check, compare, k_cap, K_WHOLE, K_CH, cdiv, ceil4, out_ld, layer_ref, strided_op,  # noqa: F401
                           valid_masks, taps, phase_layer)

# (Cin, Cout, k, stride, groups) of convs.0 .. convs.5, reference sr/models.py:289-294
DISC_S = [(1, 128, 15, 1, 1), (128, 128, 41, 2, 4), (128, 256, 41, 2, 16), (256, 512, 41, 4, 16), (512, 1024, 41, 4, 16),
          (1024, 1024, 41, 1, 16)]
SMALL = [(16, 32, 7, 2, 2), (24, 48, 41, 4, 3), (1, 16, 3, 1, 1)]  # a short kernel at stride 2; an odd group count; Cin = 1, k = 3
DISC_S_TAIL = [(1024, 1024, 5), (1024, 1, 3)]  # convs.6 and conv_post: plain stride-1 layers
DISC_S_CHANNELS = [128, 128, 256, 512, 1024, 1024, 1024, 1]  # the eight maps
TRAIN_L = [8960, 8960, 4480, 2240, 560, 140]  # the input rows of convs.0 .. convs.5 at the trainer's segment, scale 0


# ---- the pool -----------------------------------------------------------------------------------------------------------
def pool_len(n):
    """outputs of AvgPool1d(4, 2, padding=2) on n samples"""
    return n // 2 + 1 if n > 0 else 0


def pool_ref(wav, lengths=None, gy=None, valid_taps=False):
    """(pooled [B, 1, ceil4(T // 2 + 1)], gwav or None): out[j] = ((x[2j - 2] + x[2j - 1]) + (x[2j] + x[2j + 1])) * 0.25 on every
    utterance alone, zero-padded at its own end, in wav's dtype and in exactly that order; zero beyond n // 2 + 1.  With gy the
    gradient's gather form gx[i] = 0.25 (gy[i // 2] + gy[i // 2 + 1]).  Defect: valid_taps (the divisor is the number of taps
    inside the utterance, count_include_pad=False)."""
    wav = wav.detach().cpu().reshape(wav.shape[0], 1, -1)
    B, _, T = wav.shape
    out = torch.zeros(B, 1, ceil4(T // 2 + 1), dtype=wav.dtype)
    gx = None if gy is None else torch.zeros_like(wav)
    for i in range(B):
        n = T if lengths is None else int(lengths[i])
        m = pool_len(n)
        if m == 0:
            continue
        xp = F.pad(wav[i, 0, :n], (2, 2 * m - n))  # x[-2 .. 2 m - 1]
        quad = (xp[0::2][:m] + xp[1::2][:m]) + (xp[2::2][:m] + xp[3::2][:m])
        if valid_taps:
            cnt = F.pad(torch.ones(n, dtype=wav.dtype), (2, 2 * m - n))
            out[i, 0, :m] = quad / ((cnt[0::2][:m] + cnt[1::2][:m]) + (cnt[2::2][:m] + cnt[3::2][:m]))
        else:
            out[i, 0, :m] = quad * 0.25
        if gy is not None:
            gp = F.pad(gy.detach().cpu().to(wav.dtype)[i, 0, :m], (0, 1))
            idx = torch.arange(n) // 2
            gx[i, 0, :n] = 0.25 * (gp[idx] + gp[idx + 1])
    return out, gx


# ---- DiscriminatorS -----------------------------------------------------------------------------------------------------
def disc_s_weights(seed, dtype=torch.float32):
    """seeded Conv1d weights [Cout, Cin / groups, k] and biases at uniform / sqrt(fan-in) scale under nn.discriminator_s's keys"""
    rs = np.random.RandomState(seed)
    w = {}
    shapes = [(cout, cin // g, k) for cin, cout, k, _, g in DISC_S] + [(cout, cin, k) for cin, cout, k in DISC_S_TAIL]
    for i, sh in enumerate(shapes):
        name = f"convs.{i}" if i < 7 else "conv_post"
        fan = sh[1] * sh[2]
        w[name + ".weight"] = torch.from_numpy((rs.uniform(-1, 1, sh) / np.sqrt(fan)).astype(np.float32)).to(dtype)
        w[name + ".bias"] = torch.from_numpy((rs.uniform(-1, 1, sh[0]) / np.sqrt(fan)).astype(np.float32)).to(dtype)
    return w


def layer_names():
    return [f"convs.{i}" for i in range(7)] + ["conv_post"]


def layer_params():
    """(stride, groups, k) of the eight layers"""
    return [(s, g, k) for _, _, k, s, g in DISC_S] + [(1, 1, k) for _, _, k in DISC_S_TAIL]


def map_lengths(n):
    """the eight maps' lengths for n samples: n, then divided by the stride (rounded up) layer by layer"""
    out = []
    for s, _, _ in layer_params():
        n = cdiv(n, s)
        out.append(n)
    return out


def map_lds(T):
    """the eight maps' row lengths, as nn.discriminator_s allocates them"""
    ld, out = ceil4(T), []
    for s, _, _ in layer_params():
        ld = out_ld(ld, s)
        out.append(ld)
    return out


def map_masks(T, lengths, B):
    """[B, 1, ld_l] float masks of the eight maps' valid positions"""
    masks = [torch.zeros(B, 1, ld) for ld in map_lds(T)]
    for i in range(B):
        for j, m in enumerate(map_lengths(T if lengths is None else int(lengths[i]))):
            masks[j][i, :, :m] = 1
    return masks


def disc_s_chain(weights, wav_i):
    """DiscriminatorS.forward on ONE utterance wav_i [1, 1, n] as torch's own grouped Conv1d chain: the eight PRE-activation maps
    (the reference appends leaky_relu of the first seven; the eighth is conv_post's output, the score)"""
    x, maps = wav_i, []
    for j, (name, (s, g, k)) in enumerate(zip(layer_names(), layer_params())):
        x = F.conv1d(F.leaky_relu(x, SLOPE) if j else x, weights[name + ".weight"], weights[name + ".bias"], stride=s,
                     padding=(k - 1) // 2, groups=g)
        maps.append(x)
    return maps


def disc_s_ragged(weights, wav, lengths=None):
    """the same eight maps for a ragged batch, laid out as nn.discriminator_s's: [B, C, ld_l], every utterance alone on its valid
    samples, zero beyond its lengths; in the dtype of ``weights`` (tensors that may require grad)"""
    wav = wav.reshape(wav.shape[0], 1, -1)
    B, _, T = wav.shape
    lds = map_lds(T)
    per_map = [[] for _ in lds]
    for i in range(B):
        n = T if lengths is None else int(lengths[i])
        if n <= 0:
            for j, ld in enumerate(lds):
                per_map[j].append(torch.zeros(1, DISC_S_CHANNELS[j], ld, dtype=wav.dtype))
            continue
        for j, m in enumerate(disc_s_chain(weights, wav[i:i + 1, :, :n])):
            assert m.shape[2] == map_lengths(n)[j]
            per_map[j].append(F.pad(m, (0, lds[j] - m.shape[2])))
    return [torch.cat(ms, 0) for ms in per_map]
