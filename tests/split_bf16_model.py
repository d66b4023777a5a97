"""CPU model of the encoder's split-bf16 mode (HubertEncoder(..., precision="split_bf16")): the yardstick of
tests/test_split_bf16_model_cpu.py and tests/test_gpu_hubert_split_bf16.py.

oracle.hubert_ref reaches ``linear`` and ``conv1d`` through its module global ``F``.  ``encode`` below swaps that global for
the duration of ONE hr.encode call (restored in a ``finally``) for a shim that evaluates the layers the mode replaces -- the
feature convs 1..6 and every linear -- as the mode does: each fp32 operand split into two bf16 halves, the three products
hi*hi + hi*lo + lo*hi, here with an EXACT (float64) accumulator, result rounded to fp32.  conv0 (one input channel) and the
grouped positional conv stay fp32 as on the device, and so does everything that is not a conv or a linear.  This is the
arithmetic of the mode without its fp32 accumulation, i.e. the error the mode is allowed to have; the device adds only what
the fp32 path's own bars already price.

``split`` is a parameter so that the two controls of the CPU test can replace it: the identity (the model must then be no
worse than the fp32 oracle) and hi-only, i.e. plain bf16 (hundreds of times worse: a dropped cross term cannot hide inside the
GPU bars)."""
import torch
import torch.nn.functional as TF

from oracle import hubert_ref as hr


def split(x):
    """fp32 -> two bf16 halves, widened to float64"""
    x = x.float()
    hi = x.bfloat16().float()
    lo = (x - hi).bfloat16().float()
    return hi.double(), lo.double()


def split_identity(x):
    return x.double(), torch.zeros((), dtype=torch.float64)


def split_hi_only(x):
    return x.float().bfloat16().double(), torch.zeros((), dtype=torch.float64)


def _three(op, x, w, sp):
    xh, xl = sp(x)
    wh, wl = sp(w)
    y = op(xh, wh)
    if wl.dim():
        y = y + op(xh, wl)
    if xl.dim():
        y = y + op(xl, wh)
    return y


class _Shim:
    """torch.nn.functional with ``linear`` and the ungrouped multi-channel ``conv1d`` in split arithmetic"""

    def __init__(self, sp):
        self._sp = sp

    def linear(self, x, w, b=None):
        y = _three(TF.linear, x, w, self._sp)
        return (y if b is None else y + b.double()).float()

    def conv1d(self, x, w, b=None, stride=1, padding=0, groups=1):
        if groups != 1 or x.shape[1] == 1:  # pos_conv, conv0: fp32 in both modes
            return TF.conv1d(x, w, b, stride=stride, padding=padding, groups=groups)
        y = _three(lambda u, v: TF.conv1d(u, v, None, stride=stride, padding=padding), x, w, self._sp)
        return (y if b is None else y + b.double()[None, :, None]).float()

    def __getattr__(self, name):
        return getattr(TF, name)


@torch.no_grad()
def encode(sd, centers, wav, n_layers=6, taps=None, sp=split):
    """hr.encode(sd, centers, wav, ...) with fp32 weights ``sd`` in the mode's arithmetic -> (units [T], dense [T,768] fp32)"""
    saved = hr.F
    hr.F = _Shim(sp)
    try:
        return hr.encode(sd, centers, wav, n_layers=n_layers, taps=taps)
    finally:
        hr.F = saved


# ---- one layer on its own (the direct kernel tests): float64 on the model's split operands -----------------------------------
def linear_ref(x, w, b=None):
    """x [.., K] fp32, w [M, K] fp32 -> float64: the three products of the split operands, exact accumulation, + bias"""
    y = _three(TF.linear, x, w, split)
    return y if b is None else y + b.double()


def conv1d_s2_ref(x, w, b=None):
    """x [B, C, L] fp32, w [M, C, k] fp32 -> float64 [B, M, (L - k) // 2 + 1]"""
    y = _three(lambda u, v: TF.conv1d(u, v, None, stride=2), x, w, split)
    return y if b is None else y + b.double()[None, :, None]
