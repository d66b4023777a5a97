"""Shared by tests/test_conv_strided_grad_cpu.py and tests/test_gpu_conv_strided_grad.py (not a test module): what is
nn.conv1d_strided's and nn.discriminator_p's own -- the layer tables, the period fold, and DiscriminatorP restated with Conv2d as
reference sr/models.py:241-260 writes it, next to its period-major Conv1d composition.  The float64 / float32 restatement of the
layer (layer_ref with strided_op(stride)), its phase form, the masks and the bars are conv_grad_ref's."""
import numpy as np
import torch
import torch.nn.functional as F

from conv_grad_ref import (SLOPE, check, compare, k_cap, K_WHOLE, K_CH, cdiv, ceil4, out_ld, layer_ref, strided_op,  # noqa: F401
                           valid_masks, taps, phase_layer)

DISC_P = [(1, 32, 5, 3), (32, 128, 5, 3), (128, 512, 5, 3), (512, 1024, 5, 3)]  # (Cin, Cout, k, stride), sr/models.py:234-237
TAP_TABLE = [(16, 16, 7, 2), (8, 24, 7, 4)]  # other (k, stride): taps of two and three shifts, an even stride
DISC_P_CHANNELS = [1, 32, 128, 512, 1024, 1024, 1]  # convs.0 .. convs.4, conv_post
DISC_P_KERNELS = [5, 5, 5, 5, 5, 3]
PERIODS = [2, 3, 5, 7, 11]  # sr/models.py:267


# ---- the period fold and DiscriminatorP ---------------------------------------------------------------------------------
def _lengths(lengths, B, T):
    return [T] * B if lengths is None else [int(n) for n in lengths]


def fold_one(y, period):
    """sr/models.py:245-250 on one utterance y [1, 1, n] -> [1, 1, H, period]"""
    b, c, t = y.shape
    if t % period != 0:  # pad first
        n_pad = period - (t % period)
        y = F.pad(y, (0, n_pad), "reflect")
        t = t + n_pad
    return y.view(b, c, t // period, period)


def fold_ref(wav, period, lengths=None):
    """nn.period_fold's output [B period, 1, ceil4(ceil(T / period))] by torch: every utterance alone, period-major"""
    wav = wav.detach().cpu().reshape(wav.shape[0], 1, -1)
    B, _, T = wav.shape
    x0 = torch.zeros(B * period, 1, ceil4(cdiv(T, period)), dtype=wav.dtype)
    for i, n in enumerate(_lengths(lengths, B, T)):
        if n > 0:
            v = fold_one(wav[i:i + 1, :, :n], period)  # [1, 1, H, p]
            x0[i * period:(i + 1) * period, 0, :v.shape[2]] = v[0, 0].t()
    return x0


def disc_p_weights(seed, dtype=torch.float32):
    """seeded Conv2d weights [Cout, Cin, k, 1] and biases at uniform / sqrt(Cin k) scale under nn.discriminator_p's keys"""
    rs = np.random.RandomState(seed)
    w = {}
    for i, k in enumerate(DISC_P_KERNELS):
        cin, cout = DISC_P_CHANNELS[i], DISC_P_CHANNELS[i + 1]
        name = f"convs.{i}" if i < 5 else "conv_post"
        w[name + ".weight"] = torch.from_numpy((rs.uniform(-1, 1, (cout, cin, k, 1)) / np.sqrt(cin * k)).astype(np.float32)).to(dtype)
        w[name + ".bias"] = torch.from_numpy((rs.uniform(-1, 1, cout) / np.sqrt(cin * k)).astype(np.float32)).to(dtype)
    return w


def _layer_names():
    return [f"convs.{i}" for i in range(5)] + ["conv_post"]


def map_lds(T, period):
    """the six maps' row lengths, as nn.discriminator_p allocates them"""
    ld = ceil4(cdiv(T, period))
    out = []
    for _ in range(4):
        ld = out_ld(ld, 3)
        out.append(ld)
    return out + [ld, ld]


def disc_p_conv2d(weights, wav, period, lengths=None):
    """DiscriminatorP.forward (sr/models.py:241-260) with Conv2d, every utterance alone on its valid samples, in the dtype of
    ``weights`` (tensors that may require grad).  Returns the six PRE-activation maps (the reference appends leaky_relu of the
    first five; the sixth is conv_post's output, the score) laid out as nn.discriminator_p's: [B period, C, ld_l], row
    b period + w = column w of utterance b, zero beyond ceil(n / period) divided by 3, rounded up, per strided layer."""
    wav = wav.reshape(wav.shape[0], 1, -1)
    B, _, T = wav.shape
    lds = map_lds(T, period)
    per_map = [[] for _ in range(6)]
    for i, n in enumerate(_lengths(lengths, B, T)):
        if n <= 0:
            for j, ld in enumerate(lds):
                per_map[j].append(torch.zeros(period, DISC_P_CHANNELS[j + 1], ld, dtype=wav.dtype))
            continue
        x = fold_one(wav[i:i + 1, :, :n], period)
        for j, name in enumerate(_layer_names()):
            w = weights[name + ".weight"]
            w = w if w.dim() == 4 else w.unsqueeze(3)
            k = w.shape[2]
            if j > 0:
                x = F.leaky_relu(x, SLOPE)
            x = F.conv2d(x, w, weights[name + ".bias"], stride=(3, 1) if j < 4 else 1, padding=((k - 1) // 2, 0))
            m = x[0].permute(2, 0, 1)  # [p, C, H_l]
            per_map[j].append(F.pad(m, (0, lds[j] - m.shape[2])))
    return [torch.cat(ms, 0) for ms in per_map]


def disc_p_conv1d(weights, wav, period, lengths=None):
    """the same maps by the composition nn.discriminator_p runs: the fold, then plain Conv1d layers on the B period rows, each row
    alone on its valid part"""
    wav = wav.reshape(wav.shape[0], 1, -1)
    B, _, T = wav.shape
    lds = map_lds(T, period)
    x0 = fold_ref(wav, period, lengths)
    maps = [torch.zeros(B * period, DISC_P_CHANNELS[j + 1], ld, dtype=wav.dtype) for j, ld in enumerate(lds)]
    for i, n in enumerate(_lengths(lengths, B, T)):
        if n <= 0:
            continue
        x = x0[i * period:(i + 1) * period, :, :cdiv(n, period)]
        for j, name in enumerate(_layer_names()):
            w = weights[name + ".weight"]
            w = w[:, :, :, 0] if w.dim() == 4 else w
            x = F.conv1d(F.leaky_relu(x, SLOPE) if j > 0 else x, w, weights[name + ".bias"], stride=3 if j < 4 else 1,
                         padding=(w.shape[2] - 1) // 2)
            maps[j][i * period:(i + 1) * period, :, :x.shape[2]] = x
    return maps


def map_masks(T, period, lengths, B):
    """[B period, 1, ld_l] float masks of the six maps' valid positions"""
    lds = map_lds(T, period)
    masks = [torch.zeros(B * period, 1, ld) for ld in lds]
    for i, n in enumerate(_lengths(lengths, B, T)):
        h = cdiv(n, period)
        for j in range(6):
            if j < 4:
                h = cdiv(h, 3)
            masks[j][i * period:(i + 1) * period, :, :h] = 1
    return masks
