"""The numpy model of the six-point Toom-Cook residual pairs in the kernels' fp32 arithmetic (not a test module; why and against what:
tests/test_tc6_model.py): the matrices of F(3,4), the transform steps, the conv in the kernel's order and in the direct order, a whole
pair, its rms errors against float64, and the trained-like draws.  Shared by tests/test_tc6_model.py, test_tc6_c64_model.py and
test_f23_c64_model.py."""
import functools
from fractions import Fraction as Fr

import numpy as np
import pytest

BT = [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]]
AT = [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 1]]
G = [[Fr(1, 4), 0, 0, 0], [Fr(-1, 6)] * 4, [Fr(-1, 6), Fr(1, 6), Fr(-1, 6), Fr(1, 6)],
     [Fr(1, 24), Fr(2, 24), Fr(4, 24), Fr(8, 24)], [Fr(1, 24), Fr(-2, 24), Fr(4, 24), Fr(-8, 24)], [0, 0, 0, 1]]
SLOPE = 0.1


# ------------------------------------------------------------------------------------------------------------------------
# the fp32 model
# ------------------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in float64; one rounding to fp32 after the sum"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _bt(x0, x1, x2, x3, x4, x5, fma):
    one = x0.dtype.type
    pe, po, re, ro = fma(one(-4), x2, x4), fma(one(-4), x1, x3), x4 - x2, x3 - x1
    return [fma(one(4), x0, fma(one(-5), x2, x4)), pe + po, pe - po, fma(one(2), ro, re), fma(one(-2), ro, re),
            fma(one(4), x1, fma(one(-5), x3, x5))]


def _at(Y0, Y1, Y2, Y3, Y4, Y5, fma):
    one = Y0.dtype.type
    s12, d12, s34, d34 = Y1 + Y2, Y1 - Y2, Y3 + Y4, Y3 - Y4
    return [(Y0 + s12) + s34, fma(one(2), d34, d12), fma(one(4), s34, s12) + Y5]


def _conv_tc6(x, w, d):
    """x [C, L] fp32 (activated, zero outside), w [Co, Ci, k] fp32 -> conv without bias [Co, L] fp32, in the kernel's arithmetic"""
    Co, Ci, k = w.shape
    ns, L = (k + 3) // 4, x.shape[1]
    D, P = d * ns, (k - 1) // 2 * d
    nu = -(-L // (3 * D))
    xp = np.zeros((Ci, nu * 3 * D + (4 * ns - 1) * d + 1), np.float32)
    xp[:, P:P + L] = x  # x(t - P + tap d) = xp[t + tap d]
    first = (3 * D * np.arange(nu)[:, None] + np.arange(D)[None, :]).ravel()
    Gd = np.array([[float(v) for v in row] for row in G])
    wz = np.zeros((Co, Ci, 4 * ns))
    wz[:, :, :k] = w
    acc = [np.zeros((Co, first.size), np.float32) for _ in range(6)]
    for chunk in range(Ci // 16):
        for j in range(ns):
            U = np.einsum("pi,oci->poc", Gd, wz[:, :, j::ns]).astype(np.float32)  # [6][Co][Ci]
            for ci in range(16 * chunk, 16 * chunk + 16):
                b = _bt(*[xp[ci, first + j * d + q * D] for q in range(6)], fma=_fma32)
                for p in range(6):
                    acc[p] = _fma32(U[p][:, ci][:, None], b[p][None, :], acc[p])
    y = _at(*acc, fma=_fma32)
    out = np.zeros((Co, nu * 3 * D), np.float32)
    for m in range(3):
        out[:, first + m * D] = y[m]
    return out[:, :L]


def _conv_direct(x, w, d, dtype):
    """the direct order: one fused multiply-add chain per output over (tap, channel); dtype float64 is the reference"""
    Co, Ci, k = w.shape
    L, P = x.shape[1], (k - 1) // 2 * d
    xp = np.zeros((Ci, L + 2 * P), dtype)
    xp[:, P:P + L] = x
    acc = np.zeros((Co, L), dtype)
    for tap in range(k):
        for ci in range(Ci):
            a, b = w[:, ci, tap].astype(dtype)[:, None], xp[ci, tap * d:tap * d + L][None, :]
            acc = _fma32(a, b, acc) if dtype == np.float32 else acc + a * b
    return acc


def _lrelu(v):
    return np.where(v > 0, v, v * v.dtype.type(SLOPE))


def _pair(x, w1, b1, w2, b2, d, conv):
    t = _lrelu(conv(_lrelu(x), w1, d) + b1[:, None])
    return x + (conv(t, w2, 1) + b2[:, None])


def _rms_errors(x, w1, b1, w2, b2, d, conv):
    """rms error against float64 of the pair with `conv` as its conv model and with the direct-order fp32 one; the signal's rms"""
    ref = _pair(x.astype(np.float64), w1.astype(np.float64), b1.astype(np.float64), w2.astype(np.float64), b2.astype(np.float64), d,
                lambda v, w, dd: _conv_direct(v, w, dd, np.float64))
    y6 = _pair(x, w1, b1, w2, b2, d, conv)
    yd = _pair(x, w1, b1, w2, b2, d, lambda v, w, dd: _conv_direct(v, w, dd, np.float32))
    assert y6.dtype == np.float32 and yd.dtype == np.float32
    return float(np.sqrt(np.mean((y6 - ref) ** 2))), float(np.sqrt(np.mean((yd - ref) ** 2))), float(np.sqrt(np.mean(ref ** 2)))


@functools.lru_cache(maxsize=None)
def _trained_like():
    import torch
    from oracle import generator_ref as gr
    import synthdata as synth
    folded = gr.fold_state_dict(synth.synth_generator_state_dict(seed=0, kind="trained_like"))
    w64 = gr.to_double(folded)
    code, f0, spkr, _ = synth.synth_generator_inputs(1, 16, seed=199, kind="trained_like")
    x = gr.embed_concat(w64, torch.from_numpy(code), torch.from_numpy(f0), torch.from_numpy(spkr))
    conv_taps = {}
    gr.generator_forward(w64, synth.VCTK_CONFIG, x, taps={}, conv_taps=conv_taps)
    return folded, {key[:-2]: v[0].float().numpy() for key, v in conv_taps.items() if key.endswith(".x")}


@pytest.fixture(scope="module")
def trained_like():
    """the trained-like checkpoint (per-channel gains over decades, outlier channels, heavy tails) and the float64 oracle's
    inputs of every ResBlock conv on a trained-like utterance: built once per process, read-only"""
    return _trained_like()
