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
GPU bars).

The generator's split-bf16 kernels (csrc/conv_bf3.hip, csrc/resblock_bf3.hip; CodeGenerator(..., precision="split_bf16")) have
their models at the end of this file: one conv, one ConvTranspose, one residual pair with its epilogue and a whole ResBlock as
resblock_bf3_kernel chains it, with a third control ("two terms": the lo half of the activations dropped, i.e. one of the two
cross terms missing) and an fp32-accumulating emulation of the device.  Yardsticks of tests/test_gen_split_bf16_model_cpu.py and
tests/test_gpu_gen_split_bf16.py."""
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


def split_two_terms(x):
    """the split itself; as ``sp`` of the generator's models it drops the product of the activations' lo half (x_lo * w_hi)"""
    return split(x)


split_two_terms.x_lo = False


def _three(op, x, w, sp, dtype=torch.float64):
    """dtype float32: the same products (exact in fp32: 8 x 8 significant bits) accumulated in fp32 like the matrix core"""
    xh, xl = (t.to(dtype) for t in sp(x))
    wh, wl = (t.to(dtype) for t in sp(w))
    y = op(xh, wh)
    if wl.dim():
        y = y + op(xh, wl)
    if xl.dim() and getattr(sp, "x_lo", True):
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


# ---- the generator's kernels: "same" convs on leaky-ReLU'd input, zeros outside the utterance ---------------------------------
def conv1d_ref(x, w, b, k, d, slope, sp=split, dtype=torch.float64):
    """x [B, Cin, n] fp32 (the valid columns only), w [Cout, Cin, k] -> float64 [B, Cout, n]: the leaky ReLU in fp32 as the
    kernel applies it on load, then the three products of split(lrelu(x)) against split(w), exact accumulation, + bias"""
    assert w.shape[2] == k
    a = TF.leaky_relu(x.float(), slope) if slope != 1.0 else x.float()
    y = _three(lambda u, v: TF.conv1d(u, v, None, padding=(k - 1) * d // 2, dilation=d), a, w, sp, dtype)
    return (y if b is None else y + b.to(dtype)[None, :, None]).double()


def conv_transpose1d_ref(x, w, b, s, slope, sp=split, dtype=torch.float64):
    """x [B, Cin, n] fp32, w [Cin, Cout, k]: ConvTranspose1d(stride s, padding (k - s) / 2) -> float64 [B, Cout, s n]"""
    a = TF.leaky_relu(x.float(), slope) if slope != 1.0 else x.float()
    y = _three(lambda u, v: TF.conv_transpose1d(u, v, None, stride=s, padding=(w.shape[2] - s) // 2), a, w, sp, dtype)
    return (y if b is None else y + b.to(dtype)[None, :, None]).double()


def pair_ref(x, w1, b1, w2, b2, k, d, slope=0.1, epi=1, acc=None, div=3.0, sp=split, dtype=torch.float64):
    """one residual pair as two launches of conv_bf3_kernel run it: t = fp32(conv_d(lrelu(x))), y = x + fp32(conv_1(lrelu(t))) in
    fp32, then the epilogue (1: y; 2: y; 3: acc + y; 4: (acc + y) / div, fp32) -> fp32 [B, C, n]"""
    t = conv1d_ref(x, w1, b1, k, d, slope, sp, dtype).float()
    y = x.float() + conv1d_ref(t, w2, b2, k, 1, slope, sp, dtype).float()
    if epi in (1, 2):
        return y
    return acc.float() + y if epi == 3 else (acc.float() + y) / div


def resblock_ref(x, w6, b6, k, dil, m0=0, m1=3, slope=0.1, sp=split, dtype=torch.float64):
    """pairs [m0, m1) of a ResBlock as resblock_bf3_kernel chains them, on ONE utterance's valid columns x [C, n] (zeros outside
    [0, n) at every layer: the "same" padding of each conv): every conv input is lrelu then split, every conv result is rounded
    to fp32, x_k stays in fp32 -> x_k fp32 [C, n].  w6 / b6 in execution order (c1_0, c2_0, c1_1, c2_1, c1_2, c2_2)."""
    xk = x.float()[None]
    for m in range(m0, m1):
        t = conv1d_ref(xk, w6[2 * m], b6[2 * m], k, dil[m], slope, sp, dtype).float()
        xk = xk + conv1d_ref(t, w6[2 * m + 1], b6[2 * m + 1], k, 1, slope, sp, dtype).float()
    return xk[0]


def resblock_plain(x, w6, b6, k, dil, m0=0, m1=3, slope=0.1, dtype=torch.float64):
    """the unsplit operation in `dtype` end to end (float64: the truth; float32: torch's own fp32 computation)"""
    xk = x.to(dtype)[None]
    for m in range(m0, m1):
        t = TF.conv1d(TF.leaky_relu(xk, slope), w6[2 * m].to(dtype), b6[2 * m].to(dtype), padding=(k - 1) * dil[m] // 2, dilation=dil[m])
        xk = xk + TF.conv1d(TF.leaky_relu(t, slope), w6[2 * m + 1].to(dtype), b6[2 * m + 1].to(dtype), padding=(k - 1) // 2)
    return xk[0]


def col_errs(y, ref):
    """y, ref [.., C, n] -> [.., n]: per column, l2 over the channels, relative to the reference's"""
    d = y.double() - ref.double()
    return d.norm(dim=-2) / ref.double().norm(dim=-2).clamp_min(1e-300)


FLOOR = 2.0 ** -24      # a yardstick error is never taken smaller than this
KERNEL_RATIO = 4.0      # tests/test_gpu_hubert_split_bf16.py: one launch against float64 on the split operands, x torch fp32's error
MODEL_FACTOR = 2.0      # the same file: margin on the model's error (fp32 instead of exact accumulation, summation order)
FP32_RATIO = 4.0        # ... plus the allowance of an fp32 kernel on torch fp32's own error


def launch_bar(e_fp32):
    """a single launch of conv_bf3_kernel against float64 on the same split operands"""
    return KERNEL_RATIO * max(e_fp32, FLOOR)


def block_bar(e_model, e_fp32):
    """a pair or a block against float64 on the unsplit operands"""
    return MODEL_FACTOR * e_model + FP32_RATIO * max(e_fp32, FLOOR)
