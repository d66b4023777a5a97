"""Differentiable layers for training the vocoder on the MI355X (C ABI ``dissc_convgrad_*``, csrc/conv_grad.hip,
``dissc_convtgrad_*``, csrc/conv_grad_t.hip, ``dissc_convsgrad_*`` / ``dissc_period_fold_*``, csrc/conv_grad_s.hip,
``dissc_convggrad_*`` / ``dissc_mean_pool_*``, csrc/conv_grad_g.hip, ``dissc_ganloss_*``, csrc/gan_loss.hip, and
``dissc_snorm_*``, csrc/spectral_norm.hip).

    y = nn.conv1d(x, weight, bias, lengths=lengths, dilation=d, in_slope=0.1, add=res)   # a torch.autograd.Function
    y = nn.resblock1(x, weights, k)                                                       # reference sr/models.py:34-41
    y = nn.resblock2(x, weights, k, (d0, d1))                                             # reference sr/models.py:50-63
    y = nn.conv_transpose1d(x, weight, bias, stride=u, lengths=lengths, in_slope=0.1)     # the upsamplers ups[i]
    y = nn.conv1d_strided(x, weight, bias, stride=3, lengths=lengths, in_slope=0.1)       # the period discriminator's layers
    score, fmaps, lens = nn.discriminator_p(wav, weights, period, lengths)                # reference sr/models.py:228-260
    y = nn.conv1d_grouped(x, weight, bias, stride=4, groups=16, lengths=lengths, in_slope=0.1)  # the scale discriminator's layers
    pooled, out_lengths = nn.mean_pool(wav, lengths)                                      # AvgPool1d(4, 2, padding=2)
    score, fmaps, lens = nn.discriminator_s(wav, weights, lengths)                        # reference sr/models.py:285-307
    nn.wgrad_partials_grouped(...), nn.workspace_bytes_grouped(...)                       # host-only plan queries
    out = nn.MultiPeriodDiscriminator()(y, y_hat, lengths)                                # reference sr/models.py:263-286
    out = nn.MultiScaleDiscriminator()(y, y_hat, lengths)                                 # reference sr/models.py:310-333
    nn.discriminator_loss(out), nn.generator_loss(out), nn.feature_loss(out)              # reference sr/models.py:352-383
    opt = nn.AdamW(D.parameters(), lr, betas); opt.step()                                 # torch.optim.AdamW, one launch (csrc/adamw.hip)

``conv1d`` is the stride-1 "same" Conv1d that 92 of the generator's 97 conv layers are, with dissc_conv1d's conventions:
the leaky ReLU of the INPUT is applied on load (``in_slope``; 1.0 = none), ``add`` is a residual added in the epilogue,
positions at and beyond ``lengths[b]`` are read as zero and never written.  Forward and the data gradient run on the direct
MFMA conv kernels, the weight gradient on its own MFMA kernel with fixed-order partial sums (no atomics: bit-reproducible).
The weights are a DEVICE tensor and are packed on the device on every call, because they change every step in training.
No torch compute op on the hot path, no CPU fallback.  First order only.

The four conv layers are one core: a ``_Kind`` describes each (its C entries, the weight layout, the row length of y for a
row length of x, whether it has groups), and one handle cache, one set of checks, ``_forward`` and ``_backward`` work on that
description; the four autograd Functions differ in their argument lists only.
"""
import ctypes

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from ._lib import DisscError, check, current_stream_ptr, lib

WGRAD_CHUNK = 64  # DISSC_CONVGRAD_CHUNK: time positions per chunk of the weight-gradient kernel
LRELU_SLOPE = 0.1  # reference sr/models.py:13


_ENTRIES = ("create", "destroy", "set_weights", "forward", "partials", "workspace_bytes", "backward")


class _Kind:
    """one differentiable conv layer kind: its C entries, how (Cin, Cout, k) are read from the weight's shape, the outputs
    nout(p, ld) of a row of ld inputs as a function of the layer's own parameter p (dilation or stride), and the names its
    messages use"""

    def __init__(self, who, prefix, layout, dims, nout, fwd_args, grouped=False, create="create"):
        vp, i32, sz, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_float
        self.who, self.prefix, self.layout, self.dims, self.nout = who, prefix, layout, dims, nout
        self.grouped = grouped  # one more create parameter, groups: dims() then reads Cin / groups from the weight
        self.names = {e: f"{prefix}_{e}" for e in _ENTRIES}
        self.names["create"] = f"{prefix}_{create}"
        for e, name in self.names.items():
            setattr(self, e, getattr(lib, name))
        self.create.argtypes = [i32] * (5 if grouped else 4) + [ctypes.POINTER(vp)]
        self.destroy.argtypes, self.destroy.restype = [vp], None
        self.set_weights.argtypes = [vp, vp, vp, vp]
        self.forward.argtypes = fwd_args + [vp, vp, i32, i32, i32, i32, f32, vp]  # ..., y, lengths, B, ldx, ldo, Lmax, slope, stream
        self.partials.argtypes = [vp, i32, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
        self.workspace_bytes.argtypes, self.workspace_bytes.restype = [vp, i32, i32], sz
        self.backward.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, f32, vp, vp, vp, vp, sz, vp]

    def ldo(self, p, ld):
        """the row length of y: the outputs, rounded up to 4"""
        return (self.nout(p, ld) + 3) // 4 * 4


# weight [Cout, Cin, k], p = dilation, forward(h, x, add, ...)  /  weight [Cin, Cout, k], p = stride, forward(h, x, ...)  /
# weight [Cout, Cin, k], p = stride, forward(h, x, ...)  /  weight [Cout, Cin / groups, k], p = stride, groups, forward(h, x, ...)
CONV1D = _Kind("nn.conv1d", "dissc_convgrad", "[Cout, {}, k]", lambda s: (s[1], s[0], s[2]), lambda p, ld: ld, [ctypes.c_void_p] * 3,
               create="create_wide")  # (k - 1) * dilation up to 72
CONV_TRANSPOSE1D = _Kind("nn.conv_transpose1d", "dissc_convtgrad", "[{}, Cout, k]", lambda s: (s[0], s[1], s[2]),
                         lambda p, ld: p * ld, [ctypes.c_void_p] * 2)
CONV1D_STRIDED = _Kind("nn.conv1d_strided", "dissc_convsgrad", "[Cout, {}, k]", lambda s: (s[1], s[0], s[2]),
                       lambda p, ld: -(-ld // p), [ctypes.c_void_p] * 2)
CONV1D_GROUPED = _Kind("nn.conv1d_grouped", "dissc_convggrad", "[Cout, {} / groups, k]", lambda s: (s[1], s[0], s[2]),
                       lambda p, ld: -(-ld // p), [ctypes.c_void_p] * 2, grouped=True)

lib.dissc_convgrad_create_prec.argtypes = [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_void_p)]
lib.dissc_convgrad_precision_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]
PRECISIONS = {"fp32": 0, "split_bf16": 1}  # the prec of dissc_convgrad_create_prec


def _prec(precision, who):
    """the C ABI's prec of a precision name; any other name is refused here, before any launch"""
    if precision not in PRECISIONS:
        raise DisscError(f"{who}: unknown precision {precision!r} (one of {', '.join(PRECISIONS)})")
    return PRECISIONS[precision]


_handles = {}     # (prefix, Cin, Cout, k, p, device[, groups][, "split_bf16"]) -> handle; device None: host-only queries
_workspaces = {}  # device -> uint8 tensor, grown on demand (calls on one device are stream-ordered)


def _handle(kind, Cin, Cout, k, p, device=None, groups=1, prec=0):
    """Cin: the layer's input channels (of all groups); groups is part of the key and of the create call of a grouped kind only;
    prec = 1 (nn.conv1d only): the split-bf16 handle of the shape, a handle of its own beside the fp32 one"""
    key = (kind.prefix, int(Cin), int(Cout), int(k), int(p), None if device is None else torch.device(device))
    extra = (int(groups),) if kind.grouped else ()
    key += extra
    if prec:
        if kind is not CONV1D:
            raise DisscError(f"{kind.who}: fp32 only (split_bf16 is nn.conv1d's)")
        key += ("split_bf16",)
    h = _handles.get(key)
    if h is None:
        h = ctypes.c_void_p()
        if prec:
            check(lib.dissc_convgrad_create_prec(key[1], key[2], key[3], key[4], int(prec), ctypes.byref(h)),
                  "dissc_convgrad_create_prec")
        else:
            check(kind.create(key[1], key[2], key[3], key[4], *extra, ctypes.byref(h)), kind.names["create"])
        _handles[key] = h
    return h


def _partials(kind, B, Lmax, Cin, Cout, k, p=1, groups=1):
    P, pairs = ctypes.c_int(0), ctypes.c_int(0)
    check(kind.partials(_handle(kind, Cin, Cout, k, p, groups=groups), int(B), int(Lmax), ctypes.byref(P), ctypes.byref(pairs)),
          kind.names["partials"])
    return P.value, pairs.value


def wgrad_partials(B, Lmax, Cin, Cout, k):
    """(P, pairs): the weight gradient of a [Cout, Cin, k] layer over B utterances of up to Lmax positions is summed in P
    partials; partial p takes the (utterance, chunk) pairs [p * pairs, (p + 1) * pairs) of the utterance-major list with
    ceil(Lmax / WGRAD_CHUNK) chunks per utterance.  A function of the shape only (host only, no GPU needed)."""
    return _partials(CONV1D, B, Lmax, Cin, Cout, k)


def workspace_bytes(B, Lmax, Cin, Cout, k):
    """bytes of the backward's workspace (host only)"""
    return int(CONV1D.workspace_bytes(_handle(CONV1D, Cin, Cout, k, 1), int(B), int(Lmax)))


def conv1d_precision(Cin, Cout, k, dilation=1):
    """(fwd, dgrad, wgrad): whether the forward, the data gradient and the weight gradient of
    conv1d(..., precision="split_bf16") on a [Cout, Cin, k] layer run split-bf16 (True) or on the fp32 kernels, with the
    default call's bits (False): dissc_convgrad_precision_info, answered by the functions the launches consult.  Host only."""
    out = (ctypes.c_int32 * 3)()
    check(lib.dissc_convgrad_precision_info(_handle(CONV1D, Cin, Cout, k, dilation, prec=1), out), "dissc_convgrad_precision_info")
    return tuple(bool(v) for v in out)


def _precision_report(precision, entries):
    """a module's precision_report(): entries (layer name, (Cin, Cout, k, dilation) of a conv1d layer or None for any other
    kind) -> {name: (fwd, dgrad, wgrad)}; the other kinds, and every layer of an fp32 module, are (False, False, False)"""
    fp32 = (False, False, False)
    return {name: conv1d_precision(*a) if a is not None and PRECISIONS[precision] else fp32 for name, a in entries}


def wgrad_partials_transpose(B, Lmax, Cin, Cout, k, stride):
    """wgrad_partials for conv_transpose1d's weight gradient [Cin, Cout, k]: Lmax and the chunks are INPUT positions (a chunk
    is stride * WGRAD_CHUNK columns of the output's gradient).  A function of the shape only (host only)."""
    return _partials(CONV_TRANSPOSE1D, B, Lmax, Cin, Cout, k, stride)


def workspace_bytes_transpose(B, Lmax, Cin, Cout, k, stride):
    """bytes of conv_transpose1d's backward workspace (host only)"""
    return int(CONV_TRANSPOSE1D.workspace_bytes(_handle(CONV_TRANSPOSE1D, Cin, Cout, k, stride), int(B), int(Lmax)))


def wgrad_partials_strided(B, Lmax, Cin, Cout, k, stride):
    """wgrad_partials for conv1d_strided's weight gradient [Cout, Cin, k]: Lmax is in INPUT positions, the chunks are
    WGRAD_CHUNK OUTPUT positions (stride * WGRAD_CHUNK columns of x), ceil(ceil(Lmax / stride) / WGRAD_CHUNK) per utterance.
    A function of the shape only (host only)."""
    return _partials(CONV1D_STRIDED, B, Lmax, Cin, Cout, k, stride)


def workspace_bytes_strided(B, Lmax, Cin, Cout, k, stride):
    """bytes of conv1d_strided's backward workspace (host only)"""
    return int(CONV1D_STRIDED.workspace_bytes(_handle(CONV1D_STRIDED, Cin, Cout, k, stride), int(B), int(Lmax)))


def wgrad_partials_grouped(B, Lmax, Cin, Cout, k, stride, groups):
    """wgrad_partials for conv1d_grouped's weight gradient [Cout, Cin / groups, k]: Lmax is in INPUT positions, the chunks are
    WGRAD_CHUNK OUTPUT positions, ceil(ceil(Lmax / stride) / WGRAD_CHUNK) per utterance; the partials take at most 56 MB.
    A function of the shape only (host only)."""
    return _partials(CONV1D_GROUPED, B, Lmax, Cin, Cout, k, stride, groups)


def workspace_bytes_grouped(B, Lmax, Cin, Cout, k, stride, groups):
    """bytes of conv1d_grouped's backward workspace (host only)"""
    return int(CONV1D_GROUPED.workspace_bytes(_handle(CONV1D_GROUPED, Cin, Cout, k, stride, groups=groups), int(B), int(Lmax)))


def _workspace(device, nbytes):
    ws = _workspaces.get(device)
    if ws is None or ws.numel() < nbytes:
        ws = _workspaces[device] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def _check_act(t, name, B=None, ld=None, who="nn.conv1d"):
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.is_contiguous() and t.shape[2] % 4 == 0):
        raise DisscError(f"{who}: {name} must be a contiguous fp32 device tensor [B, C, ld] with ld % 4 == 0")
    if B is not None and (t.shape[0] != B or t.shape[2] != ld):
        raise DisscError(f"{who}: {name} is {tuple(t.shape)}, expected batch {B} and row stride {ld}")


def _lengths_ok(lengths, B):
    return lengths is None or (lengths.is_cuda and lengths.dtype == torch.int32 and lengths.is_contiguous()
                               and tuple(lengths.shape) == (B,))


def _check_layer(kind, x, weight, bias, lengths, groups=1):
    """the refusals every conv layer shares; -> Cout"""
    _check_act(x, "x", who=kind.who)
    B, Cin, _ = x.shape
    if groups < 1 or (groups != 1 and not kind.grouped):
        raise DisscError(f"{kind.who}: groups = {groups}")
    if not (weight.is_cuda and weight.dtype == torch.float32 and weight.dim() == 3 and weight.is_contiguous()
            and kind.dims(weight.shape)[0] * groups == Cin):
        raise DisscError(f"{kind.who}: weight must be a contiguous fp32 device tensor {kind.layout.format(Cin)}")
    Cout = kind.dims(weight.shape)[1]
    if bias is not None and not (bias.is_cuda and bias.dtype == torch.float32 and bias.is_contiguous()
                                 and tuple(bias.shape) == (Cout,)):
        raise DisscError(f"{kind.who}: bias must be a contiguous fp32 device tensor [Cout]")
    if not _lengths_ok(lengths, B):
        raise DisscError(f"{kind.who}: lengths must be a contiguous int32 device tensor [B]")
    return Cout


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _forward(kind, ctx, x, weight, bias, lengths, p, in_slope, *add, groups=1, prec=0):
    """set_weights, the output (zeros where lengths, or a row longer than its outputs, leave part of it unwritten), forward;
    saves x and weight, never y"""
    B, Cin, ld = x.shape
    _, Cout, k = kind.dims(weight.shape)
    h = _handle(kind, Cin, Cout, k, p, x.device, groups, prec)
    st = current_stream_ptr(x.device)
    ldo = kind.ldo(p, ld)
    with torch.cuda.device(x.device):
        check(kind.set_weights(h, _ptr(weight), _ptr(bias), st), kind.names["set_weights"])
        y = torch.zeros((B, Cout, ldo), dtype=torch.float32, device=x.device) if lengths is not None or ldo != kind.nout(p, ld) else \
            torch.empty((B, Cout, ldo), dtype=torch.float32, device=x.device)
        check(kind.forward(h, _ptr(x), *map(_ptr, add), _ptr(y), _ptr(lengths), B, ld, ldo, ld, in_slope, st), kind.names["forward"])
    ctx.save_for_backward(x, weight)
    ctx.lengths, ctx.p, ctx.in_slope, ctx.has_bias, ctx.groups, ctx.prec = lengths, p, in_slope, bias is not None, groups, prec
    return y


def _backward(kind, ctx, gy):
    """-> (gx, gw, gb, gy made contiguous) for the inputs 0 .. 2 that need a gradient, None for the others"""
    x, weight = ctx.saved_tensors
    B, Cin, ld = x.shape
    _, Cout, k = kind.dims(weight.shape)
    need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    need_b = ctx.has_bias and ctx.needs_input_grad[2]
    gy = gy.contiguous()
    gx = gw = gb = ws = None
    if need_x or need_w or need_b:
        h = _handle(kind, Cin, Cout, k, ctx.p, x.device, ctx.groups, ctx.prec)
        st = current_stream_ptr(x.device)
        with torch.cuda.device(x.device):
            if need_x:  # another layer sharing the handle may have run since the forward: pack again (device only)
                check(kind.set_weights(h, _ptr(weight), None, st), kind.names["set_weights"])
                gx = torch.empty_like(x)
            if need_w:
                gw = torch.empty_like(weight)
            if need_b:
                gb = torch.empty(Cout, dtype=torch.float32, device=x.device)
            nws = 0
            if need_w or need_b:
                nws = int(kind.workspace_bytes(h, B, ld))
                ws = _workspace(x.device, nws)
            check(kind.backward(h, _ptr(x), _ptr(gy), _ptr(ctx.lengths), B, ld, kind.ldo(ctx.p, ld), ld, ctx.in_slope,
                                _ptr(gx), _ptr(gw), _ptr(gb), _ptr(ws), nws, st), kind.names["backward"])
    return gx, gw, gb, gy


class _Conv1dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, add, lengths, dilation, in_slope, prec):
        ctx.has_add = add is not None
        return _forward(CONV1D, ctx, x, weight, bias, lengths, dilation, in_slope, add, prec=prec)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        gx, gw, gb, gy = _backward(CONV1D, ctx, gy)
        return gx, gw, gb, (gy if ctx.has_add and ctx.needs_input_grad[3] else None), None, None, None, None


def conv1d(x, weight, bias=None, lengths=None, dilation=1, in_slope=1.0, add=None, precision="fp32"):
    """y = bias + conv(lrelu(x, in_slope), weight, dilation, padding "same") (+ add).

    x [B, Cin, ld], add / y [B, Cout, ld]: contiguous fp32 device tensors, ld % 4 == 0.  weight: DEVICE tensor
    [Cout, Cin, k], k odd, k <= 11, (k - 1) * dilation <= 72; bias [Cout] or None.  lengths: int32 [B] on the device (or
    None = ld): positions at and beyond lengths[b] are read as zero and left zero in y.  Gradients flow to x, weight,
    bias and add (the gradient of add is the incoming gradient itself, handed through unmasked: the cotangent of a position
    beyond lengths[b], which the forward never writes, is the caller's to keep zero); x and weight are saved, y is not.

    precision: "fp32" (the default) or "split_bf16": every operand v is split into hi = bf16(v), lo = bf16(v - hi) and every
    product is hi*hi + hi*lo + lo*hi on the bf16 matrix cores with fp32 accumulation (~2^-17 relative per product), in each of
    the three directions that has a split instance -- conv1d_precision(Cin, Cout, k, dilation) tells which; the others (fewer
    than 32 rows, (k - 1) * dilation > 60) run the fp32 kernels with the default call's bits.  The bias gradient is fp32."""
    prec = _prec(precision, "nn.conv1d")
    Cout = _check_layer(CONV1D, x, weight, bias, lengths)
    if add is not None:
        _check_act(add, "add", x.shape[0], x.shape[2])
        if add.shape[1] != Cout:
            raise DisscError("nn.conv1d: add must have Cout channels")
    return _Conv1dFn.apply(x, weight, bias, add, lengths, int(dilation), float(in_slope), prec)


class _ConvTranspose1dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, lengths, stride, in_slope):
        return _forward(CONV_TRANSPOSE1D, ctx, x, weight, bias, lengths, stride, in_slope)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return _backward(CONV_TRANSPOSE1D, ctx, gy)[:3] + (None, None, None)


def conv_transpose1d(x, weight, bias=None, stride=1, lengths=None, in_slope=1.0):
    """y = bias + ConvTranspose1d(lrelu(x, in_slope), weight, stride=stride, padding=(k - stride) // 2): the generator's
    upsamplers ups[i] (reference sr/models.py), which follow a leaky ReLU.

    x [B, Cin, ld]: contiguous fp32 device tensor, ld % 4 == 0; y [B, Cout, stride * ld].  weight: DEVICE tensor
    [Cin, Cout, k] (torch's ConvTranspose1d layout), 1 <= stride <= 8, stride <= k <= 11, k - stride even; bias [Cout] or None.
    lengths: int32 [B] on the device (or None = ld), INPUT lengths: utterance b has stride * lengths[b] valid output positions,
    y is left zero beyond them and the incoming gradient is read as zero there; the gradient of x is zero from lengths[b] on.
    Gradients flow to x, weight and bias; x and weight are saved, y is not."""
    _check_layer(CONV_TRANSPOSE1D, x, weight, bias, lengths)
    return _ConvTranspose1dFn.apply(x, weight, bias, lengths, int(stride), float(in_slope))


class _Conv1dStridedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, lengths, stride, in_slope):
        return _forward(CONV1D_STRIDED, ctx, x, weight, bias, lengths, stride, in_slope)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return _backward(CONV1D_STRIDED, ctx, gy)[:3] + (None, None, None)


def conv1d_strided(x, weight, bias=None, stride=2, lengths=None, in_slope=1.0):
    """y = bias + Conv1d(lrelu(x, in_slope), weight, stride=stride, padding=(k - 1) // 2): the strided layers of the period
    discriminator (reference sr/models.py:234-237 on period-major rows), the adjoint of conv_transpose1d.

    x [B, Cin, ld]: contiguous fp32 device tensor, ld % 4 == 0; y [B, Cout, ceil4(ceil(ld / stride))].  weight: DEVICE tensor
    [Cout, Cin, k], k odd, 3 <= k <= 11, 2 <= stride <= min(k, 8); bias [Cout] or None.  lengths: int32 [B] on the device (or
    None = ld), INPUT lengths: utterance b has ceil(lengths[b] / stride) valid output positions (torch's count for that input),
    x is read as zero from lengths[b] on, y is left zero beyond its length and the incoming gradient is read as zero there; the
    gradient of x is zero from lengths[b] on.  Gradients flow to x, weight and bias; x and weight are saved, y is not."""
    _check_layer(CONV1D_STRIDED, x, weight, bias, lengths)
    return _Conv1dStridedFn.apply(x, weight, bias, lengths, int(stride), float(in_slope))


class _Conv1dGroupedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, lengths, stride, groups, in_slope):
        return _forward(CONV1D_GROUPED, ctx, x, weight, bias, lengths, stride, in_slope, groups=groups)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return _backward(CONV1D_GROUPED, ctx, gy)[:3] + (None, None, None, None)


def conv1d_grouped(x, weight, bias=None, stride=1, groups=1, lengths=None, in_slope=1.0):
    """y = bias + Conv1d(lrelu(x, in_slope), weight, stride=stride, padding=(k - 1) // 2, groups=groups): the grouped, wide-tap
    layers of the scale discriminator (reference sr/models.py:289-294).

    x [B, Cin, ld]: contiguous fp32 device tensor, ld % 4 == 0; y [B, Cout, ceil4(ceil(ld / stride))].  weight: DEVICE tensor
    [Cout, Cin / groups, k], k odd, 3 <= k <= 41, stride 1, 2 or 4, Cin / groups 1 or a multiple of 8 up to 64, Cout / groups a
    multiple of 16 up to 128; bias [Cout] or None.  lengths: int32 [B] on the device (or None = ld), INPUT lengths: utterance b
    has ceil(lengths[b] / stride) valid output positions (torch's count for that input), x is read as zero from lengths[b] on, y
    is left zero beyond its length and the incoming gradient is read as zero there; the gradient of x is zero from lengths[b]
    on.  Gradients flow to x, weight and bias; x and weight are saved, y is not."""
    groups = int(groups)
    _check_layer(CONV1D_GROUPED, x, weight, bias, lengths, groups)
    return _Conv1dGroupedFn.apply(x, weight, bias, lengths, int(stride), groups, float(in_slope))


def resblock1(x, weights, k, dilations=(1, 3, 5), lengths=None, taps=None, precision="fp32"):
    """ResBlock1 (reference sr/models.py:34-41): for each dilation d,  x = x + conv_1(lrelu(conv_d(lrelu(x)))), composed
    from six conv1d calls with the residual through ``add=``.  weights: {"convs1.<m>.weight" / ".bias",
    "convs2.<m>.weight" / ".bias"} (device tensors, weight norm already folded).  taps: a list that receives the input
    tensor of every conv1d call in order -- the engine's own pre-activations.  precision: that of every conv1d call."""
    for m, d in enumerate(dilations):
        if taps is not None:
            taps.append(x)
        xt = conv1d(x, weights[f"convs1.{m}.weight"], weights.get(f"convs1.{m}.bias"), lengths=lengths, dilation=d,
                    in_slope=LRELU_SLOPE, precision=precision)
        if taps is not None:
            taps.append(xt)
        x = conv1d(xt, weights[f"convs2.{m}.weight"], weights.get(f"convs2.{m}.bias"), lengths=lengths, dilation=1,
                   in_slope=LRELU_SLOPE, add=x, precision=precision)
    return x


def resblock2(x, weights, k, dilations=(1, 3), lengths=None, taps=None, precision="fp32"):
    """ResBlock2 (reference sr/models.py:50-63, the light block of HiFi-GAN V3): for each of the two dilations d,
    x = x + conv_d(lrelu(x)), composed from two conv1d calls with the residual through ``add=``.  weights:
    {"convs.<m>.weight" / ".bias"} (device tensors, weight norm already folded).  taps, precision: as in resblock1."""
    if len(dilations) != 2:
        raise DisscError(f"nn.resblock2: {len(dilations)} dilations (ResBlock2 has two convs)")
    for m, d in enumerate(dilations):
        if taps is not None:
            taps.append(x)
        x = conv1d(x, weights[f"convs.{m}.weight"], weights.get(f"convs.{m}.bias"), lengths=lengths, dilation=d,
                   in_slope=LRELU_SLOPE, add=x, precision=precision)
    return x


# ---------------------------------------------------------------------------------------------------------------------
# The period discriminator (reference sr/models.py:228-260) on period-major rows: the fold (C ABI dissc_period_fold_*,
# csrc/conv_grad_s.hip), four conv1d_strided, two conv1d.
# ---------------------------------------------------------------------------------------------------------------------
lib.dissc_period_fold_fwd.argtypes = lib.dissc_period_fold_bwd.argtypes = \
    [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_void_p]
DISC_P_STRIDE, DISC_P_STRIDED_LAYERS = 3, 4  # reference sr/models.py:229, :234-237


def _ceil4(n):
    return (n + 3) // 4 * 4


def _host_lengths(lengths, B, T, who):
    """host int64 [B] from a list, an array or a tensor on either side; None: T"""
    if lengths is None:
        return np.full(B, T, dtype=np.int64)
    ln = np.asarray(lengths.cpu() if isinstance(lengths, torch.Tensor) else lengths, dtype=np.int64).reshape(-1)
    if ln.shape[0] != B or (ln < 0).any() or (ln > T).any():
        raise ValueError(f"{who}: lengths must be [B] counts within 0 .. {T}")
    return ln


def _check_reflect(ln, period, who):
    """F.pad(..., "reflect") of n samples to a multiple of the period needs the padding, period - n % period, below n"""
    for n in ln:
        if n % period and n <= period - n % period:
            raise ValueError(f"{who}: an utterance of {int(n)} samples cannot be reflect-padded to a multiple of the period {period}")


class _PeriodFoldFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, wav, period, lengths):
        B, T = wav.shape[0], wav.shape[-1]
        ldh = _ceil4(-(-T // period))
        x0 = torch.zeros((B * period, 1, ldh), dtype=torch.float32, device=wav.device)
        with torch.cuda.device(wav.device):
            check(lib.dissc_period_fold_fwd(_ptr(wav), _ptr(lengths), B, T, period, T, ldh, _ptr(x0), current_stream_ptr(wav.device)),
                  "dissc_period_fold_fwd")
        ctx.lengths, ctx.period, ctx.shape = lengths, period, tuple(wav.shape)
        return x0

    @staticmethod
    @once_differentiable
    def backward(ctx, gx0):
        gx0 = gx0.contiguous()
        B, T = ctx.shape[0], ctx.shape[-1]
        gwav = torch.empty(ctx.shape, dtype=torch.float32, device=gx0.device)
        with torch.cuda.device(gx0.device):
            check(lib.dissc_period_fold_bwd(_ptr(gx0), _ptr(ctx.lengths), B, T, ctx.period, T, gx0.shape[2], _ptr(gwav),
                                            current_stream_ptr(gx0.device)), "dissc_period_fold_bwd")
        return gwav, None, None


def _check_wav(wav, who):
    if not (wav.is_cuda and wav.dtype == torch.float32 and wav.is_contiguous() and wav.shape[-1] >= 1
            and (wav.dim() == 2 or (wav.dim() == 3 and wav.shape[1] == 1))):
        raise DisscError(f"{who}: wav must be a contiguous fp32 device tensor [B, 1, T] or [B, T]")


def period_fold(wav, period, lengths=None):
    """x0 [B * period, 1, ceil4(ceil(T / period))] from wav [B, 1, T] or [B, T] with lengths[b] valid samples (a list, an array
    or a tensor on either side; None = T): the view(b, c, t // period, period) of reference sr/models.py:245-250, period-major.
    Row b * period + w holds ypad_b[h * period + w] for h < ceil(lengths[b] / period), ypad_b = utterance b reflect-padded at
    ITS OWN end to a multiple of the period, zero beyond.  Every row is an independent 1-D sequence.  ValueError where torch's
    reflect pad raises (0 < n <= period - n % period with n % period != 0); n = 0 gives empty rows.  The gradient of wav sums
    each sample's one or two contributions (no atomics) and is zero from lengths[b] on."""
    who = "nn.period_fold"
    _check_wav(wav, who)
    period = int(period)
    if not 1 <= period <= 65535:
        raise DisscError(f"{who}: period {period} outside 1 .. 65535")
    dev_len = lengths if isinstance(lengths, torch.Tensor) and lengths.is_cuda else None
    if lengths is not None:
        ln = _host_lengths(lengths, wav.shape[0], wav.shape[-1], who)
        _check_reflect(ln, period, who)
        if dev_len is None:
            dev_len = torch.from_numpy(ln.astype(np.int32)).to(wav.device)
    else:
        _check_reflect([wav.shape[-1]], period, who)
    if not _lengths_ok(dev_len, wav.shape[0]):
        raise DisscError(f"{who}: device lengths must be a contiguous int32 tensor [B]")
    return _PeriodFoldFn.apply(wav, period, dev_len)


def discriminator_p(wav, weights, period, lengths=None, precision="fp32"):
    """DiscriminatorP (reference sr/models.py:228-260) of wav [B, 1, T] or [B, T] with lengths[b] valid samples (host counts; a
    device tensor is copied back) -> (score, fmaps, lens).

    weights: {"convs.<i>.weight" / ".bias" (i = 0 .. 4), "conv_post.weight" / ".bias"}, device tensors with weight norm already
    folded, Conv2d weights [Cout, Cin, k, 1] or [Cout, Cin, k].  Composed as period_fold, four conv1d_strided (k = 5, stride 3;
    the first with in_slope = 1), conv1d (k = 5) and conv1d (k = 3) with in_slope = 0.1, on B * period rows: no torch compute op
    on the path.  fmaps: the six feature maps [B * period, C, ld_l], PRE-ACTIVATION and zero beyond their lengths: where the
    reference appends leaky_relu(conv) to fmap, every consumer here applies the leaky ReLU on load, as the next layer does (a
    feature-matching loss reads lrelu(f, 0.1) of maps 0 .. 4 and map 5 as it is).  score: the last map, [B * period, 1, ld]
    (row b * period + w, column h is the reference's flattened score[b][h * period + w]).  lens: the six maps' per-row device
    lengths, int32 [B * period] each: ceil(n / period), divided by 3 (rounded up) once per strided layer.  precision: that of
    the two conv1d layers (convs.4, conv_post); the strided layers are fp32."""
    who = "nn.discriminator_p"
    _prec(precision, who)
    _check_wav(wav, who)
    period = int(period)
    B, T = wav.shape[0], wav.shape[-1]
    ln = _host_lengths(lengths, B, T, who)
    _check_reflect(ln, period, who)
    rows = [np.repeat(-(-ln // period), period)]
    for _ in range(DISC_P_STRIDED_LAYERS):
        rows.append(-(-rows[-1] // DISC_P_STRIDE))
    # the waveform's and every layer's lengths in one upload
    flat = torch.from_numpy(np.concatenate([ln] + rows).astype(np.int32)).to(wav.device)
    n = B * period
    wav_len, lens = flat[:B], [flat[B + i * n:B + (i + 1) * n] for i in range(len(rows))]

    def W(name):
        w = weights[name + ".weight"]
        return (w.view(w.shape[:3]) if w.dim() == 4 and w.shape[3] == 1 else w), weights.get(name + ".bias")

    x = _PeriodFoldFn.apply(wav, period, wav_len)
    fmaps = []
    for i in range(DISC_P_STRIDED_LAYERS):
        x = conv1d_strided(x, *W(f"convs.{i}"), stride=DISC_P_STRIDE, lengths=lens[i], in_slope=LRELU_SLOPE if i else 1.0)
        fmaps.append(x)
    x = conv1d(x, *W(f"convs.{DISC_P_STRIDED_LAYERS}"), lengths=lens[-1], in_slope=LRELU_SLOPE, precision=precision)
    fmaps.append(x)
    x = conv1d(x, *W("conv_post"), lengths=lens[-1], in_slope=LRELU_SLOPE, precision=precision)
    fmaps.append(x)
    return x, fmaps, lens[1:] + [lens[-1], lens[-1]]


# ---------------------------------------------------------------------------------------------------------------------
# The scale discriminator (reference sr/models.py:285-307): six conv1d_grouped, two conv1d; the average pool between the scales
# (C ABI dissc_mean_pool_*, csrc/conv_grad_g.hip).
# ---------------------------------------------------------------------------------------------------------------------
lib.dissc_mean_pool_fwd.argtypes = lib.dissc_mean_pool_bwd.argtypes = \
    [ctypes.c_void_p] * 3 + [ctypes.c_int] * 5 + [ctypes.c_void_p]
# (stride, groups) of convs.0 .. convs.5, reference sr/models.py:289-294; convs.6 and conv_post are plain conv1d layers
DISC_S_GROUPED = [(1, 1), (2, 4), (2, 16), (4, 16), (4, 16), (1, 16)]


class _MeanPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, wav, lengths):
        B, T = wav.shape[0], wav.shape[-1]
        ldo = _ceil4(T // 2 + 1)
        out = torch.zeros((B, 1, ldo), dtype=torch.float32, device=wav.device)
        with torch.cuda.device(wav.device):
            check(lib.dissc_mean_pool_fwd(_ptr(wav), _ptr(out), _ptr(lengths), B, 1, T, T, ldo, current_stream_ptr(wav.device)),
                  "dissc_mean_pool_fwd")
        ctx.lengths, ctx.shape = lengths, tuple(wav.shape)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        g = g.contiguous()
        B, T = ctx.shape[0], ctx.shape[-1]
        gwav = torch.empty(ctx.shape, dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            check(lib.dissc_mean_pool_bwd(_ptr(g), _ptr(gwav), _ptr(ctx.lengths), B, 1, T, T, g.shape[2], current_stream_ptr(g.device)),
                  "dissc_mean_pool_bwd")
        return gwav, None


def mean_pool(wav, lengths=None):
    """(pooled [B, 1, ceil4(T // 2 + 1)], out_lengths) from wav [B, 1, T] or [B, T] with lengths[b] valid samples (a list, an
    array or a tensor on either side; None = T): AvgPool1d(4, 2, padding=2) between the scales (reference sr/models.py:315),
    every utterance zero-padded at ITS OWN end.  pooled[b][j] = ((w[2j - 2] + w[2j - 1]) + (w[2j] + w[2j + 1])) / 4 for
    j <= n // 2, zero beyond; out_lengths: host int64 [B], n // 2 + 1 (0 for n = 0).  The gradient of wav is the gather form (no
    atomics) and is zero from lengths[b] on."""
    who = "nn.mean_pool"
    _check_wav(wav, who)
    B, T = wav.shape[0], wav.shape[-1]
    ln = _host_lengths(lengths, B, T, who)
    dev_len = lengths if isinstance(lengths, torch.Tensor) and lengths.is_cuda else None
    if lengths is not None and dev_len is None:
        dev_len = torch.from_numpy(ln.astype(np.int32)).to(wav.device)
    if not _lengths_ok(dev_len, B):
        raise DisscError(f"{who}: device lengths must be a contiguous int32 tensor [B]")
    return _MeanPoolFn.apply(wav, dev_len), np.where(ln > 0, ln // 2 + 1, 0)


def discriminator_s(wav, weights, lengths=None, precision="fp32"):
    """DiscriminatorS (reference sr/models.py:285-307) of wav [B, 1, T] or [B, T] with lengths[b] valid samples (host counts; a
    device tensor is copied back) -> (score, fmaps, lens).

    weights: {"convs.<i>.weight" / ".bias" (i = 0 .. 6), "conv_post.weight" / ".bias"}, device tensors with the norm (weight or
    spectral) already folded.  Composed as six conv1d_grouped (k = 15, then k = 41 with strides 2, 2, 4, 4, 1 and 4, 16, 16, 16,
    16 groups; the first with in_slope = 1), conv1d (k = 5) and conv1d (k = 3) with in_slope = 0.1: no torch compute op on the
    path.  A waveform whose T is no multiple of 4 is copied once into a zeroed row of ceil4(T) samples (allocation and copy;
    autograd slices the gradient back).  fmaps: the eight feature maps [B, C, ld_l], PRE-ACTIVATION and zero beyond their
    lengths, the contract of discriminator_p's.  score: the last map, [B, 1, ld].  lens: the eight maps' device lengths, int32
    [B] each: n, ceil(n / 2), ceil(/ 2), ceil(/ 4), ceil(/ 4), then unchanged three times.  precision: that of the two conv1d
    layers (convs.6, conv_post); the grouped layers are fp32."""
    who = "nn.discriminator_s"
    _prec(precision, who)
    _check_wav(wav, who)
    B, T = wav.shape[0], wav.shape[-1]
    ln = _host_lengths(lengths, B, T, who)
    rows = [ln]  # the input lengths of convs.0 .. convs.5, then of the three stride-1 layers behind them
    for s, _ in DISC_S_GROUPED:
        rows.append(-(-rows[-1] // s))
    flat = torch.from_numpy(np.concatenate(rows).astype(np.int32)).to(wav.device)  # every layer's lengths in one upload
    lens = [flat[i * B:(i + 1) * B] for i in range(len(rows))]
    fmaps = _disc_s_layers(_wav_rows4(wav), weights, lens, precision)
    return fmaps[-1], fmaps, lens[1:] + [lens[-1], lens[-1]]


def _wav_rows4(wav):
    """wav as [B, 1, T]; a T that is no multiple of 4 is copied once into zeroed rows of ceil4(T) samples"""
    B, T = wav.shape[0], wav.shape[-1]
    x = wav.reshape(B, 1, T)
    if T % 4:
        x = torch.zeros((B, 1, _ceil4(T)), dtype=torch.float32, device=wav.device)
        x[:, :, :T] = wav.reshape(B, 1, T)
    return x


def _disc_s_layers(x, weights, lens, precision="fp32"):
    """the eight maps of DiscriminatorS on x [rows, 1, ld] (ld % 4 == 0); lens: the device lengths of the inputs of convs.0 ..
    convs.5 and of the stride-1 layers behind them (seven tensors)"""
    fmaps = []
    for i, (s, g) in enumerate(DISC_S_GROUPED):
        x = conv1d_grouped(x, weights[f"convs.{i}.weight"], weights.get(f"convs.{i}.bias"), stride=s, groups=g, lengths=lens[i],
                           in_slope=LRELU_SLOPE if i else 1.0)
        fmaps.append(x)
    x = conv1d(x, weights["convs.6.weight"], weights.get("convs.6.bias"), lengths=lens[-1], in_slope=LRELU_SLOPE, precision=precision)
    fmaps.append(x)
    x = conv1d(x, weights["conv_post.weight"], weights.get("conv_post.bias"), lengths=lens[-1], in_slope=LRELU_SLOPE,
               precision=precision)
    fmaps.append(x)
    return fmaps


# ---------------------------------------------------------------------------------------------------------------------
# The rest of the generator's training step (C ABI dissc_wnorm_* / dissc_embed_concat_* / dissc_mrf_mean_* / dissc_tanh_*,
# csrc/gen_train.hip) and the module that composes it: nn.CodeGenerator.
# ---------------------------------------------------------------------------------------------------------------------
def _bind_gen_train():
    vp, i32, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    lib.dissc_wnorm_create.argtypes = [i32, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(vp)]
    lib.dissc_wnorm_destroy.argtypes = [vp]
    lib.dissc_wnorm_destroy.restype = None
    lib.dissc_wnorm_offsets.argtypes = [vp, ctypes.POINTER(ll), ctypes.POINTER(ll), ctypes.POINTER(ll), ctypes.POINTER(ll)]
    lib.dissc_wnorm_wave_cols.argtypes = []
    lib.dissc_wnorm_forward.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, vp]
    lib.dissc_wnorm_backward.argtypes = [vp, vp, vp, ctypes.POINTER(vp), vp, vp, ctypes.POINTER(vp), ctypes.POINTER(i32), vp, vp]
    lib.dissc_embed_concat_fwd.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, i32, vp]
    lib.dissc_embed_concat_bwd.argtypes = [vp, vp, i32, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp]
    lib.dissc_mrf_mean_fwd.argtypes = [ctypes.POINTER(vp), i32, vp, vp, i32, i32, i32, i32, vp]
    lib.dissc_mrf_mean_bwd.argtypes = [vp, i32, vp, vp, i32, i32, i32, i32, vp]
    lib.dissc_tanh_fwd.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, vp]
    lib.dissc_tanh_bwd.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]


_bind_gen_train()

WNORM_WAVE_COLS = int(lib.dissc_wnorm_wave_cols())  # rows of up to this many columns: one wave; longer: one workgroup
POST_SLOPE = 0.01  # F.leaky_relu's default, in front of conv_post (reference sr/models.py:110)


def _f32(t, name, who):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise DisscError(f"{who}: {name} must be a contiguous fp32 device tensor")
    return t


def _check_leaf_shaped(module, tensors):
    shapes = module.leaf_shapes()
    if len(tensors) != len(shapes) or any(tuple(t.shape) != s for t, s in zip(tensors, shapes)):
        raise DisscError(f"{type(module).__name__}.named_views: tensors of the shapes {shapes} expected (parameters()'s), got "
                         f"{[tuple(t.shape) for t in tensors]}")


class WeightNorm:
    """w = g v / ||v|| over every dim but 0 for a whole list of tensors at once (dissc_wnorm_*): ``shapes`` are the tensors'
    (rows, cols), cols the product of every dim but 0.  ``off[i]`` / ``row_off[i]`` place tensor i in the flat layouts of
    ``total`` floats (v, w, gv; every tensor 16-byte aligned) and ``total_rows`` rows (g, gg, 1 / ||v||).  ``bias_sizes``
    (optional): the layers' bias lengths; ``bias_off[i]`` places them, each 16-byte aligned, in ``bias_total`` floats."""

    def __init__(self, shapes, bias_sizes=None):
        n = len(shapes)
        rows = (ctypes.c_int * max(n, 1))(*[int(r) for r, _ in shapes])
        cols = (ctypes.c_int * max(n, 1))(*[int(c) for _, c in shapes])
        self._h = ctypes.c_void_p()
        check(lib.dissc_wnorm_create(n, rows, cols, ctypes.byref(self._h)), "dissc_wnorm_create")
        self.n, self.shapes = n, [(int(r), int(c)) for r, c in shapes]
        off, roff = (ctypes.c_longlong * n)(), (ctypes.c_longlong * n)()
        tot, rtot = ctypes.c_longlong(0), ctypes.c_longlong(0)
        check(lib.dissc_wnorm_offsets(self._h, off, roff, ctypes.byref(tot), ctypes.byref(rtot)), "dissc_wnorm_offsets")
        self.off, self.row_off, self.total, self.total_rows = list(off), list(roff), tot.value, rtot.value
        self.has_gaps = self.total != sum(r * c for r, c in self.shapes)
        self.bias_sizes = None if bias_sizes is None else [int(b) for b in bias_sizes]
        self.bias_off, self.bias_total = [], 0
        if self.bias_sizes is not None:
            if len(self.bias_sizes) != n:
                raise DisscError("WeightNorm: one bias size per tensor")
            at = 0
            for b in self.bias_sizes:
                at = (at + 3) & ~3
                self.bias_off.append(at)
                at += b
            self.bias_total = (at + 3) & ~3
            self._bias_n = (ctypes.c_int * n)(*self.bias_sizes)

    def __del__(self):
        try:
            lib.dissc_wnorm_destroy(self._h)
        except Exception:
            pass

    def forward(self, v_flat, g_flat, bias_flat=None, out=None):
        """-> (buf, inv_norm): buf = [w_flat (total) | the biases (bias_total)] in one buffer (``out``, or a new one whose
        alignment gaps are zero), inv_norm [total_rows]"""
        who = "WeightNorm.forward"
        _f32(v_flat, "v_flat", who), _f32(g_flat, "g_flat", who)
        nb = 0 if bias_flat is None else self.bias_total
        if v_flat.numel() != self.total or g_flat.numel() != self.total_rows or (nb and _f32(bias_flat, "bias_flat", who).numel() != nb):
            raise DisscError(f"{who}: v_flat / g_flat / bias_flat must have {self.total} / {self.total_rows} / {self.bias_total} floats")
        dev = v_flat.device
        if out is None:
            out = (torch.zeros if self.has_gaps else torch.empty)(self.total + nb, dtype=torch.float32, device=dev)
        inv = torch.empty(self.total_rows, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(lib.dissc_wnorm_forward(self._h, _ptr(v_flat), _ptr(g_flat), _ptr(out), _ptr(inv), _ptr(bias_flat),
                                          ctypes.c_void_p(out.data_ptr() + 4 * self.total) if nb else None, nb,
                                          current_stream_ptr(dev)), "dissc_wnorm_forward")
        return out, inv

    def backward(self, v_flat, g_flat, gws, gbs=None, gv_out=None):
        """gws: the layers' own weight gradients (None = zero); gbs: their bias gradients (None = zero), or None for no
        biases at all -> (gv_flat, gg_flat, gb_flat or None)"""
        who = "WeightNorm.backward"
        dev = v_flat.device
        if len(gws) != self.n or (gbs is not None and (self.bias_sizes is None or len(gbs) != self.n)):
            raise DisscError(f"{who}: {self.n} weight gradients (and bias gradients, with bias_sizes) expected")
        for i, t in enumerate(gws):
            if t is not None and _f32(t, f"gws[{i}]", who).numel() != self.shapes[i][0] * self.shapes[i][1]:
                raise DisscError(f"{who}: gws[{i}] has {t.numel()} elements, expected {self.shapes[i]}")
        for i, t in enumerate(gbs or ()):
            if t is not None and _f32(t, f"gbs[{i}]", who).numel() != self.bias_sizes[i]:
                raise DisscError(f"{who}: gbs[{i}] has {t.numel()} elements, expected {self.bias_sizes[i]}")
        pw = (ctypes.c_void_p * self.n)(*[None if t is None else t.data_ptr() for t in gws])
        pb = None if gbs is None else (ctypes.c_void_p * self.n)(*[None if t is None else t.data_ptr() for t in gbs])
        gv = gv_out if gv_out is not None else \
            (torch.zeros if self.has_gaps else torch.empty)(self.total, dtype=torch.float32, device=dev)
        gg = torch.empty(self.total_rows, dtype=torch.float32, device=dev)
        gb = None if gbs is None else torch.zeros(self.bias_total, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(lib.dissc_wnorm_backward(self._h, _ptr(v_flat), _ptr(g_flat), pw, _ptr(gv), _ptr(gg), pb,
                                           None if gbs is None else self._bias_n, _ptr(gb), current_stream_ptr(dev)),
                  "dissc_wnorm_backward")
        return gv, gg, gb


class _WeightsFn(torch.autograd.Function):
    """(v_flat, g_flat, bias_flat) -> every layer's weight and bias, views of ONE buffer made here (children of a flat leaf by
    narrow / view would make autograd zero-fill and add a whole flat tensor per layer); the backward is one launch"""

    @staticmethod
    def forward(ctx, v_flat, g_flat, bias_flat, wn, dims):
        buf, _ = wn.forward(v_flat, g_flat, bias_flat)
        ctx.save_for_backward(v_flat, g_flat)
        ctx.wn = wn
        ws = [buf[o:o + r * c].view(d) for o, (r, c), d in zip(wn.off, wn.shapes, dims)]
        bs = [buf[wn.total + o:wn.total + o + n] for o, n in zip(wn.bias_off, wn.bias_sizes)]
        return tuple(ws + bs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        v_flat, g_flat = ctx.saved_tensors
        n = ctx.wn.n
        gws = [None if t is None else t.contiguous() for t in grads[:n]]
        gbs = [None if t is None else t.contiguous() for t in grads[n:]]
        gv, gg, gb = ctx.wn.backward(v_flat, g_flat, gws, gbs)
        return gv, gg, gb, None, None


class _EmbedConcatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dict_w, spkr_w, code, f0, spkr, lengths, ld):
        B, T = code.shape
        n_codes, E = dict_w.shape
        C = E + (0 if f0 is None else 1) + (0 if spkr is None else E)
        dev = dict_w.device
        x = torch.zeros((B, C, ld), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(lib.dissc_embed_concat_fwd(_ptr(code), _ptr(f0), _ptr(spkr), _ptr(dict_w), _ptr(spkr_w) if spkr is not None else None,
                                             _ptr(lengths), B, T, E, n_codes, 0 if spkr is None else spkr_w.shape[0], _ptr(x), ld,
                                             current_stream_ptr(dev)), "dissc_embed_concat_fwd")
        ctx.code, ctx.spkr, ctx.lengths, ctx.has_f0 = code, spkr, lengths, f0 is not None
        ctx.dims = (B, T, E, n_codes, 0 if spkr is None else spkr_w.shape[0], ld)
        return x

    @staticmethod
    @once_differentiable
    def backward(ctx, gx):
        B, T, E, n_codes, n_spk, ld = ctx.dims
        gx = gx.contiguous()
        dev = gx.device
        g_dict = torch.empty((n_codes, E), dtype=torch.float32, device=dev)
        g_spkr = None if ctx.spkr is None else torch.empty((n_spk, E), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(lib.dissc_embed_concat_bwd(_ptr(gx), _ptr(ctx.code), int(ctx.has_f0), _ptr(ctx.spkr), _ptr(ctx.lengths), B, T, E,
                                             n_codes, n_spk, ld, _ptr(g_dict), _ptr(g_spkr), current_stream_ptr(dev)),
                  "dissc_embed_concat_bwd")
        return g_dict, g_spkr, None, None, None, None, None


def embed_concat(dict_w, spkr_w, code, f0=None, spkr=None, lengths=None, ld=None):
    """x [B, C, ld] = [dict_w[code] (E) | f0 (1) | spkr_w[spkr] (E)] per position, zero at and beyond lengths[b] (the
    generator's input; reference sr/models.py:189,207-215).  dict_w [n_codes, E] and spkr_w [n_spk, E]: device tensors that
    get dense gradients (rows of unused ids: exact zeros); code i64 [B, T], f0 f32 [B, T] or None, spkr i64 [B] or None,
    lengths i32 [B] (at most T) or None, all on the device; ids outside a table are clamped to it.  ld: the row stride,
    default T rounded up to 4."""
    who = "nn.embed_concat"
    _f32(dict_w, "dict_w", who)
    B, T = code.shape
    ld = (T + 3) // 4 * 4 if ld is None else int(ld)
    ok = code.is_cuda and code.dtype == torch.int64 and code.is_contiguous() and code.dim() == 2
    ok = ok and (f0 is None or (f0.is_cuda and f0.dtype == torch.float32 and f0.is_contiguous() and tuple(f0.shape) == (B, T)))
    ok = ok and (spkr is None or (spkr.is_cuda and spkr.dtype == torch.int64 and spkr.is_contiguous() and tuple(spkr.shape) == (B,)))
    ok = ok and _lengths_ok(lengths, B)
    if not ok or dict_w.dim() != 2 or (spkr is not None and (_f32(spkr_w, "spkr_w", who).dim() != 2 or spkr_w.shape[1] != dict_w.shape[1])):
        raise DisscError(f"{who}: code i64 [B, T], f0 f32 [B, T], spkr i64 [B], lengths i32 [B], contiguous on the device; "
                         "tables [rows, E]")
    return _EmbedConcatFn.apply(dict_w, spkr_w if spkr is not None else None, code, f0, spkr, lengths, ld)


class _MrfMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lengths, *rs):
        B, C, ld = rs[0].shape
        dev = rs[0].device
        y = torch.zeros_like(rs[0]) if lengths is not None else torch.empty_like(rs[0])
        ptrs = (ctypes.c_void_p * len(rs))(*[r.data_ptr() for r in rs])
        with torch.cuda.device(dev):
            check(lib.dissc_mrf_mean_fwd(ptrs, len(rs), _ptr(y), _ptr(lengths), B, C, ld, ld, current_stream_ptr(dev)),
                  "dissc_mrf_mean_fwd")
        ctx.lengths, ctx.nk = lengths, len(rs)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        g = g.contiguous()
        B, C, ld = g.shape
        gx = torch.empty_like(g)
        with torch.cuda.device(g.device):
            check(lib.dissc_mrf_mean_bwd(_ptr(g), ctx.nk, _ptr(gx), _ptr(ctx.lengths), B, C, ld, ld, current_stream_ptr(g.device)),
                  "dissc_mrf_mean_bwd")
        return (None,) + (gx,) * ctx.nk  # written once: every branch takes the same tensor


def mrf_mean(rs, lengths=None):
    """((r0 + r1) + r2 ...) / len(rs) with a true division: the mean over the ResBlocks of a stage (reference
    sr/models.py:104-109).  rs: 1 .. 4 tensors [B, C, ld] as nn.conv1d's; zero at and beyond lengths[b]."""
    rs = list(rs)
    if not 1 <= len(rs) <= 4:
        raise DisscError("nn.mrf_mean: 1 to 4 branches")
    for r in rs:
        _check_act(r, "a branch", rs[0].shape[0], rs[0].shape[2], who="nn.mrf_mean")
        if r.shape[1] != rs[0].shape[1]:
            raise DisscError("nn.mrf_mean: the branches differ in channels")
    return _MrfMeanFn.apply(lengths, *rs)


class _TanhFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, lengths, cols):
        B, C, ld = x.shape
        y = torch.zeros((B, C, cols), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            check(lib.dissc_tanh_fwd(_ptr(x), _ptr(y), _ptr(lengths), B, C, ld, cols, cols, current_stream_ptr(x.device)),
                  "dissc_tanh_fwd")
        ctx.save_for_backward(y)
        ctx.lengths, ctx.ld = lengths, ld
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        B, C, cols = y.shape
        gy = gy.contiguous()
        gx = torch.empty((B, C, ctx.ld), dtype=torch.float32, device=y.device)
        with torch.cuda.device(y.device):
            check(lib.dissc_tanh_bwd(_ptr(y), _ptr(gy), _ptr(gx), _ptr(ctx.lengths), B, C, ctx.ld, cols, cols,
                                     current_stream_ptr(y.device)), "dissc_tanh_bwd")
        return gx, None, None


def tanh(x, lengths=None, cols=None):
    """y [B, C, cols] = tanh(x [B, C, ld]) inside lengths[b] (default cols), zero beyond; cols <= ld (default ld) is the
    output's row length: the waveform has hop * T samples, the activations rows of hop * ceil4(T).  The output is saved,
    the gradient gy (1 - y^2) is zero from lengths[b] on."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.is_contiguous()):
        raise DisscError("nn.tanh: x must be a contiguous fp32 device tensor [B, C, ld]")
    cols = x.shape[2] if cols is None else int(cols)
    if not 1 <= cols <= x.shape[2]:
        raise DisscError(f"nn.tanh: cols {cols} outside 1 .. {x.shape[2]}")
    return _TanhFn.apply(x, lengths, cols)


class CodeGenerator:
    """The trainable twin of dissc_amd.generator.CodeGenerator (reference sr/models.py:125-225): the same config keys and
    checkpoint format (the reference's UNFOLDED keys *.weight_g / *.weight_v / *.bias, dict.weight, spkr.weight), a forward
    with a grad_fn composed from this module's layers.

        G = nn.CodeGenerator(h).to("cuda:0"); G.load_state_dict(sd)
        loss = 45 * mel.l1_loss(y, G(code=, f0=, spkr=, lengths=)); loss.backward()
        torch.optim.AdamW(G.parameters()).step(); G.state_dict()          # loads into the inference CodeGenerator

    parameters(): five flat leaves -- every weight_v, every weight_g, every bias, dict.weight, spkr.weight; weight norm of all
    layers is one launch in each direction.  No torch compute op on the path (allocation, views, autograd's own sums where a
    tensor feeds several layers)."""

    _UNSUPPORTED = ("lambda_commit", "lambda_commit_code", "f0_quantizer_path")
    N_SPEAKERS = 200  # nn.Embedding(200, ...), reference sr/models.py:133

    def __init__(self, h, precision="fp32"):
        from .generator import AttrDict, resblock_conv_names, resblock_dilations, resblock_type
        _prec(precision, "nn.CodeGenerator")
        self.precision = precision  # of the conv1d layers (conv_pre, the ResBlock convs, conv_post); the upsamplers are fp32
        self.h = AttrDict(h)
        for k in self._UNSUPPORTED:
            if self.h.get(k, None):
                raise NotImplementedError(f"config option '{k}' (VQ-VAE branch) is not supported")
        self.resblock = resblock_type(self.h)
        h = self.h
        self.num_kernels, self.num_upsamples = len(h.resblock_kernel_sizes), len(h.upsample_rates)
        if not 1 <= self.num_kernels <= 4:
            raise NotImplementedError("1 to 4 ResBlocks per stage")
        self.f0, self.multispkr = h.get("f0", None), h.get("multispkr", None)
        self.hop = 1
        for u in h.upsample_rates:
            self.hop *= int(u)
        c0, E = int(h.upsample_initial_channel), int(h.embedding_dim)
        self.in_dim = int(h.get("model_in_dim", 128))
        if self.in_dim != E + (1 if self.f0 else 0) + (E if self.multispkr else 0):
            raise NotImplementedError(f"model_in_dim {self.in_dim} is not embedding_dim (+ 1 for f0) (+ embedding_dim for speakers)")
        # (name, weight shape, bias length) in the reference's order
        L = [("conv_pre", (c0, self.in_dim, 7), c0)]
        for i, k in enumerate(h.upsample_kernel_sizes):
            L.append((f"ups.{i}", (c0 >> i, c0 >> (i + 1), int(k)), c0 >> (i + 1)))
        for i in range(self.num_upsamples):
            ch = c0 >> (i + 1)
            for j, (k, ds) in enumerate(zip(h.resblock_kernel_sizes, h.resblock_dilation_sizes)):
                resblock_dilations(self.resblock, ds, k if self.resblock == 2 else None)  # (refuses what cannot run, by its key)
                L += [(name, (ch, ch, int(k)), ch) for name in resblock_conv_names(self.resblock, i * self.num_kernels + j)]
        L.append(("conv_post", (1, c0 >> self.num_upsamples, 7), 1))
        self.layers = L
        # each conv1d layer's dilation, for precision_report (the upsamplers have none)
        self._dilation = {"conv_pre": 1, "conv_post": 1}
        for n, (k, ds) in ((i * self.num_kernels + j, kd) for i in range(self.num_upsamples)
                           for j, kd in enumerate(zip(h.resblock_kernel_sizes, h.resblock_dilation_sizes))):
            dl = resblock_dilations(self.resblock, ds)
            for name, d in zip(resblock_conv_names(self.resblock, n), dl + [1] * len(dl) if self.resblock == 1 else dl):
                self._dilation[name] = d
        self._index = {name: i for i, (name, _, _) in enumerate(L)}
        self.wn = WeightNorm([(s[0], s[1] * s[2]) for _, s, _ in L], [nb for _, _, nb in L])
        self.device = torch.device("cuda:0")
        self.v_flat = self.g_flat = self.bias_flat = self.dict_weight = self.spkr_weight = None

    # -- nn.Module-like surface --------------------------------------------------------------------------------------
    def to(self, device):
        if isinstance(device, int):
            device = f"cuda:{device}"
        device = torch.device(device)
        if device.type != "cuda":
            raise DisscError("dissc_amd.nn.CodeGenerator runs on an MI355X only (device='cuda:N')")
        if self.v_flat is not None and device != self.device:
            raise DisscError("nn.CodeGenerator: choose the device before load_state_dict()")
        self.device = device
        return self

    def cuda(self, device=0):
        return self.to(device)

    def precision_report(self):
        """{layer name: (fwd, dgrad, wgrad)}: which directions of each layer run split-bf16 under this module's precision
        (nn.conv1d_precision per conv1d layer; the upsamplers are fp32).  Host only."""
        return _precision_report(self.precision, [(name, (s[1], s[0], s[2], self._dilation[name]) if name in self._dilation else None)
                                                  for name, s, _ in self.layers])

    def _keys(self):
        keys = []
        for name, _, _ in self.layers:
            keys += [name + ".bias", name + ".weight_g", name + ".weight_v"]
        return keys + ["dict.weight"] + (["spkr.weight"] if self.multispkr else [])

    def load_state_dict(self, sd, strict=True):
        """the reference's checkpoint layout: weight_g / weight_v / bias per conv, dict.weight, spkr.weight"""
        keys = self._keys()
        missing = [k for k in keys if k not in sd]
        unexpected = sorted(set(sd.keys()) - set(keys))
        if missing or (strict and unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for CodeGenerator: missing {missing[:5]}, unexpected {unexpected[:5]}")
        wn = self.wn
        v, g, b = torch.zeros(wn.total), torch.zeros(wn.total_rows), torch.zeros(wn.bias_total)
        for i, (name, shape, nb) in enumerate(self.layers):
            tv, tg, tb = (sd[name + s].detach().to("cpu", torch.float32) for s in (".weight_v", ".weight_g", ".bias"))
            if tuple(tv.shape) != shape or tg.numel() != shape[0] or tb.numel() != nb:
                raise RuntimeError(f"size mismatch for {name}: weight_v {tuple(tv.shape)}, expected {shape}")
            v[wn.off[i]:wn.off[i] + tv.numel()] = tv.reshape(-1)
            g[wn.row_off[i]:wn.row_off[i] + shape[0]] = tg.reshape(-1)
            b[wn.bias_off[i]:wn.bias_off[i] + nb] = tb.reshape(-1)
        E = int(self.h.embedding_dim)
        tables = [sd["dict.weight"]] + ([sd["spkr.weight"]] if self.multispkr else [])
        if tuple(tables[0].shape) != (int(self.h.num_embeddings), E) or (self.multispkr and tuple(tables[1].shape) != (self.N_SPEAKERS, E)):
            raise RuntimeError("size mismatch for dict.weight / spkr.weight")
        leaf = lambda t: t.detach().to(self.device, torch.float32).contiguous().clone().requires_grad_(True)
        self.v_flat, self.g_flat, self.bias_flat = leaf(v), leaf(g), leaf(b)
        self.dict_weight = leaf(tables[0])
        self.spkr_weight = leaf(tables[1]) if self.multispkr else None
        return self

    def _loaded(self):
        if self.v_flat is None:
            raise RuntimeError("load_state_dict() first")

    def parameters(self):
        """the five flat leaves (four without speakers): v_flat, g_flat, bias_flat, dict.weight, spkr.weight"""
        self._loaded()
        return [p for p in (self.v_flat, self.g_flat, self.bias_flat, self.dict_weight, self.spkr_weight) if p is not None]

    def zero_grad(self):
        for p in self.parameters():
            p.grad = None

    def _named(self, v, g, b, d, s):
        out = {}
        wn = self.wn
        for i, (name, shape, nb) in enumerate(self.layers):
            n = shape[0] * shape[1] * shape[2]
            out[name + ".bias"] = b[wn.bias_off[i]:wn.bias_off[i] + nb]
            out[name + ".weight_g"] = g[wn.row_off[i]:wn.row_off[i] + shape[0]].view(shape[0], 1, 1)
            out[name + ".weight_v"] = v[wn.off[i]:wn.off[i] + n].view(shape)
        out["dict.weight"] = d
        if s is not None:
            out["spkr.weight"] = s
        return out

    def named_grads(self):
        """{reference key: a view of its leaf's .grad} after a backward"""
        ps = self.parameters()
        if any(p.grad is None for p in ps):
            raise RuntimeError("named_grads(): run a backward first")
        return self._named(self.v_flat.grad, self.g_flat.grad, self.bias_flat.grad, self.dict_weight.grad,
                           None if self.spkr_weight is None else self.spkr_weight.grad)

    def leaf_shapes(self):
        """the shapes of parameters(), known before load_state_dict()"""
        E = int(self.h.embedding_dim)
        return [(self.wn.total,), (self.wn.total_rows,), (self.wn.bias_total,), (int(self.h.num_embeddings), E)] + \
            ([(self.N_SPEAKERS, E)] if self.multispkr else [])

    def named_views(self, *tensors):
        """{reference key of a parameter: its view} of tensors shaped like parameters(), in that order and on any device (an
        optimiser's moments, say); the order of the keys is the reference module's named_parameters()"""
        _check_leaf_shaped(self, tensors)
        return self._named(*tensors, *([] if self.multispkr else [None]))

    def named_leaves(self):
        """{reference key of a parameter: the index in parameters() of the leaf that holds it}, in named_views()'s order"""
        out = {}
        for name, _, _ in self.layers:
            out.update({name + ".bias": 2, name + ".weight_g": 1, name + ".weight_v": 0})
        out["dict.weight"] = 3
        if self.multispkr:
            out["spkr.weight"] = 4
        return out

    def state_dict(self):
        """host copies under the reference's unfolded keys"""
        self._loaded()
        host = [None if p is None else p.detach().cpu() for p in (self.v_flat, self.g_flat, self.bias_flat, self.dict_weight,
                                                                   self.spkr_weight)]
        return {k: t.clone() for k, t in self._named(*host).items()}

    # -- forward -------------------------------------------------------------------------------------------------------
    def forward(self, code=None, f0=None, spkr=None, lengths=None, taps=None, **extra):
        """code [B, T] ids, f0 [B, 1, T'] or [B, T'] (with "f0" in the config), spkr [B, 1] (with "multispkr"), lengths [B]
        valid frames (default T) -> wav [B, 1, hop T] with a grad_fn, zero beyond hop lengths[b].  The shorter of the code and
        f0 streams is repeated up to the longer one, as in the reference.  taps: a list that receives every conv's input in
        call order (conv_pre's, then per stage the upsampler's and its ResBlocks' as nn.resblock1 / nn.resblock2 give them, conv_post's)."""
        from .generator import CodeGenerator as _Inference, resblock_conv_names, resblock_dilations
        self._loaded()
        if extra:
            raise NotImplementedError(f"extra conditioning features {sorted(extra)} are not supported")
        dev = self.device
        if torch.as_tensor(code).device.type == "cpu":  # nn.Embedding raises on a bad id; device ids are clamped
            for name, t, rows in (("code", code, int(self.h.num_embeddings)), ("spkr", spkr if self.multispkr else None, self.N_SPEAKERS)):
                t = None if t is None else torch.as_tensor(t)
                if t is not None and t.device.type == "cpu" and t.numel() and (int(t.min()) < 0 or int(t.max()) >= rows):
                    raise IndexError(f"{name} id out of range: [{int(t.min())}, {int(t.max())}] not within [0, {rows})")
        code = torch.as_tensor(code).to(dev, torch.int64)
        if code.dim() != 2:
            raise ValueError("code must be [B,T]")
        f0d = None
        if self.f0:
            f0d = torch.as_tensor(f0).to(dev, torch.float32)
            if f0d.dim() == 2:
                f0d = f0d.unsqueeze(1)
            if code.shape[-1] < f0d.shape[-1]:
                code = _Inference._upsample(code.unsqueeze(1), f0d.shape[-1]).squeeze(1)
            elif f0d.shape[-1] != code.shape[-1]:
                f0d = _Inference._upsample(f0d, code.shape[-1])
            if f0d.shape[-1] != code.shape[-1] or f0d.shape[0] != code.shape[0] or f0d.shape[1] != 1:
                raise RuntimeError(f"Sizes of tensors must match: code {tuple(code.shape)} vs f0 {tuple(f0d.shape)} "
                                   "after conditioning upsample")
            f0d = f0d.reshape(code.shape[0], -1).contiguous()
        code = code.contiguous()
        B, T = code.shape
        sp = None
        if self.multispkr:
            sp = torch.as_tensor(spkr).to(dev, torch.int64).reshape(-1).contiguous()
            if sp.numel() != B:
                raise ValueError("spkr must be [B,1]")
        ln = np.full(B, T, dtype=np.int64) if lengths is None else \
            np.asarray(lengths.cpu() if isinstance(lengths, torch.Tensor) else lengths, dtype=np.int64).reshape(-1)
        if ln.shape[0] != B or (ln < 0).any() or (ln > T).any():
            raise ValueError(f"lengths must be [B] counts within 0 .. {T}")
        muls, m = [1], 1
        for u in self.h.upsample_rates:
            m *= int(u)
            muls.append(m)
        # every stage's lengths in one upload
        stage = torch.from_numpy(np.stack([ln * m for m in muls]).astype(np.int32)).to(dev)
        lens = [stage[i] for i in range(len(muls))]
        ld = (T + 3) // 4 * 4
        n = len(self.layers)
        dims = [s for _, s, _ in self.layers]
        wb = _WeightsFn.apply(self.v_flat, self.g_flat, self.bias_flat, self.wn, dims)
        W = lambda name: (wb[self._index[name]], wb[n + self._index[name]])

        def tap(t):
            if taps is not None:
                taps.append(t)
            return t

        x = embed_concat(self.dict_weight, self.spkr_weight, code, f0d, sp, lens[0], ld)
        x = conv1d(tap(x), *W("conv_pre"), lengths=lens[0], precision=self.precision)
        nk = self.num_kernels
        for i, u in enumerate(self.h.upsample_rates):
            x = conv_transpose1d(tap(x), *W(f"ups.{i}"), stride=int(u), lengths=lens[i], in_slope=LRELU_SLOPE)
            rs = []
            for j, (k, ds) in enumerate(zip(self.h.resblock_kernel_sizes, self.h.resblock_dilation_sizes)):
                pre = f"resblocks.{i * nk + j}."
                wts = {}
                for name in resblock_conv_names(self.resblock, i * nk + j):
                    wts[name[len(pre):] + ".weight"], wts[name[len(pre):] + ".bias"] = W(name)
                block = resblock1 if self.resblock == 1 else resblock2
                rs.append(block(x, wts, int(k), tuple(resblock_dilations(self.resblock, ds)), lengths=lens[i + 1], taps=taps,
                                precision=self.precision))
            x = mrf_mean(rs, lens[i + 1])
        x = conv1d(tap(x), *W("conv_post"), lengths=lens[-1], in_slope=POST_SLOPE, precision=self.precision)
        return tanh(x, lens[-1], self.hop * T)

    __call__ = forward


# ---------------------------------------------------------------------------------------------------------------------
# The period half of the GAN step (reference sr/models.py:263-286, :352-383; sr/train.py:157-190): the fused ragged losses
# (C ABI dissc_ganloss_*, csrc/gan_loss.hip) and nn.MultiPeriodDiscriminator, which runs y and y_hat as ONE batch of paired maps.
# ---------------------------------------------------------------------------------------------------------------------
def _bind_gan_loss():
    vp, i32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    pi, pf, pp = ctypes.POINTER(i32), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(vp)
    lib.dissc_ganloss_workspace_bytes.argtypes, lib.dissc_ganloss_workspace_bytes.restype = [i32, pi, pi, pi], sz
    lib.dissc_ganloss_forward.argtypes = [i32, pp, pp, pi, pi, pi, pi, pf, vp, vp, sz, vp]
    lib.dissc_ganloss_backward.argtypes = [i32, pp, pp, pi, pi, pi, pi, pf, vp, vp, pp, vp]


_bind_gan_loss()

GANLOSS_MAX_MAPS = 64                # DISSC_GANLOSS_MAX_MAPS
GANLOSS_WG_UNITS = 1024              # float4s per half that one workgroup of the loss kernels takes
FM, DISC, GEN = 0, 1, 2              # DISSC_GANLOSS_FM / _DISC / _GEN
MPD_PERIODS = (2, 3, 5, 7, 11)       # reference sr/models.py:267
_DISC_P_LAYERS = [("convs.0", 1, 32, 5), ("convs.1", 32, 128, 5), ("convs.2", 128, 512, 5), ("convs.3", 512, 1024, 5),
                  ("convs.4", 1024, 1024, 5), ("conv_post", 1024, 1, 3)]  # (name, Cin, Cout, k), reference sr/models.py:233-239


def _int_array(values):
    return (ctypes.c_int * len(values))(*[int(v) for v in values])


def ganloss_workspace_bytes(R, C, ld):
    """bytes of the loss forward's workspace for maps of R[i] row pairs, C[i] channels and row stride ld[i]: a function of the
    shapes only (host only, no GPU needed); DisscError where the entries would refuse the list"""
    n = len(R)
    if n < 1 or len(C) != n or len(ld) != n:
        raise DisscError("nn.ganloss_workspace_bytes: R, C and ld must be lists of one length, at least 1")
    nbytes = int(lib.dissc_ganloss_workspace_bytes(n, _int_array(R), _int_array(C), _int_array(ld)))
    if nbytes == 0:
        check(-1, "dissc_ganloss_workspace_bytes")
    return nbytes


class _GanLossArgs:
    """the host arrays of one dissc_ganloss_* call"""

    def __init__(self, ops, maps, lens, R, slopes):
        n = len(maps)
        self.n = n
        self.maps = (ctypes.c_void_p * n)(*[m.data_ptr() for m in maps])
        self.lens = (ctypes.c_void_p * n)(*[t.data_ptr() for t in lens])
        self.R, self.C, self.ld = _int_array(R), _int_array([m.shape[1] for m in maps]), _int_array([m.shape[2] for m in maps])
        self.ops, self.slopes = _int_array(ops), (ctypes.c_float * n)(*[float(s) for s in slopes])

    def head(self):
        return (self.n, self.maps, self.lens, self.R, self.C, self.ld, self.ops, self.slopes)


class _GanLossFn(torch.autograd.Function):
    """(total, vals [2, n]) of a list of paired maps in one forward and one backward call; the maps are saved (the layer that
    reads a map saves it anyway)"""

    @staticmethod
    def forward(ctx, ops, lens, R, slopes, *maps):
        n, dev = len(maps), maps[0].device
        a = _GanLossArgs(ops, maps, lens, R, slopes)
        nws = ganloss_workspace_bytes(R, [m.shape[1] for m in maps], [m.shape[2] for m in maps])
        out = torch.empty(1 + 2 * n, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            ws = _workspace(dev, nws)
            check(lib.dissc_ganloss_forward(*a.head(), _ptr(out), _ptr(ws), nws, current_stream_ptr(dev)), "dissc_ganloss_forward")
        ctx.save_for_backward(*maps)
        ctx.ops, ctx.lens, ctx.R, ctx.slopes = ops, lens, R, slopes
        ctx.set_materialize_grads(False)
        return out[0], out[1:].view(2, n)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_total, g_vals):
        maps = ctx.saved_tensors
        n, dev = len(maps), maps[0].device
        if g_total is None and g_vals is None:
            return (None,) * (4 + n)
        a = _GanLossArgs(ctx.ops, maps, ctx.lens, ctx.R, ctx.slopes)
        gmaps = [torch.empty_like(m) if ctx.needs_input_grad[4 + i] else None for i, m in enumerate(maps)]
        pg = (ctypes.c_void_p * n)(*[None if g is None else g.data_ptr() for g in gmaps])
        g_total = None if g_total is None else g_total.contiguous()
        g_vals = None if g_vals is None else g_vals.contiguous()
        with torch.cuda.device(dev):
            check(lib.dissc_ganloss_backward(*a.head(), _ptr(g_total), _ptr(g_vals), pg, current_stream_ptr(dev)),
                  "dissc_ganloss_backward")
        return (None, None, None, None) + tuple(gmaps)


def gan_loss(op, maps, lens, R, slopes=None):
    """The fused ragged GAN losses over a list of PAIRED maps -> (total, vals [2, n]), device tensors with a grad_fn.

    maps[i]: contiguous fp32 device tensor [2 R[i], C, ld], ld % 4 == 0, PRE-activation: rows 0 .. R - 1 the real half, rows
    R .. 2 R - 1 the generated half.  lens[i]: int32 device tensor of at least R[i] per-row lengths (row r and row R + r share
    lens[i][r]); positions at or beyond a length are never read for their value.  op: nn.FM, nn.DISC or nn.GEN, one for all maps
    or one per map; slopes: the leaky ReLU FM applies on load, per map (default 1.0).  With N = C sum(lens[:R]):
      FM    vals[0][i] = 2 / N sum |lrelu(real) - lrelu(gen)|
      DISC  vals[0][i] = 1 / N sum (1 - real)^2,  vals[1][i] = 1 / N sum gen^2
      GEN   vals[0][i] = 1 / N sum (1 - gen)^2
    (vals[1] is zero for FM and GEN; N = 0: value and gradient 0.)  total = the sum of all values in index order.  One forward
    launch pair and one backward launch for the whole list (at most nn.GANLOSS_MAX_MAPS maps); sums in double, no atomics: the
    values are bit-reproducible and a map's do not depend on the list it is in.  The gradient reaches both halves of every map
    that requires one and is exactly zero at and beyond the lengths."""
    who = "nn.gan_loss"
    maps, lens = list(maps), list(lens)
    n = len(maps)
    ops = [int(op)] * n if isinstance(op, int) else [int(o) for o in op]
    R = [int(r) for r in R]
    slopes = [1.0] * n if slopes is None else [float(s) for s in slopes]
    if not 1 <= n <= GANLOSS_MAX_MAPS:
        raise DisscError(f"{who}: {n} maps; one call takes 1 .. {GANLOSS_MAX_MAPS}")
    if not (len(lens) == len(R) == len(ops) == len(slopes) == n):
        raise DisscError(f"{who}: maps, lens, R, ops and slopes must have one entry per map")
    for i, (m, t, r, o) in enumerate(zip(maps, lens, R, ops)):
        _check_act(m, f"maps[{i}]", who=who)
        if m.device != maps[0].device or r < 1 or m.shape[0] != 2 * r:
            raise DisscError(f"{who}: maps[{i}] is {tuple(m.shape)} for R = {r}: a paired map has 2 R rows, on one device")
        if not (t.is_cuda and t.device == m.device and t.dtype == torch.int32 and t.is_contiguous() and t.dim() == 1 and t.numel() >= r):
            raise DisscError(f"{who}: lens[{i}] must be a contiguous int32 device tensor of at least R = {r} lengths")
        if o not in (FM, DISC, GEN):
            raise DisscError(f"{who}: op {o} is none of nn.FM, nn.DISC, nn.GEN")
    return _GanLossFn.apply(tuple(ops), tuple(lens), tuple(R), tuple(slopes), *maps)


class _PairedFoldFn(torch.autograd.Function):
    """x0 [2 B period, 1, ldh]: period_fold of y into the first half and of y_hat into the second, by two calls of
    dissc_period_fold_fwd on the halves of one buffer (no concatenation); the backward runs dissc_period_fold_bwd on a half only
    where that input requires a gradient"""

    @staticmethod
    def forward(ctx, y, y_hat, period, lengths):
        B, T = y.shape[0], y.shape[-1]
        ldh = _ceil4(-(-T // period))
        x0 = torch.zeros((2 * B * period, 1, ldh), dtype=torch.float32, device=y.device)
        half = 4 * B * period * ldh  # bytes; ldh % 4 == 0 keeps the second half 16-byte aligned
        st = current_stream_ptr(y.device)
        with torch.cuda.device(y.device):
            for i, w in enumerate((y, y_hat)):
                check(lib.dissc_period_fold_fwd(_ptr(w), _ptr(lengths), B, T, period, T, ldh, ctypes.c_void_p(x0.data_ptr() + i * half),
                                                st), "dissc_period_fold_fwd")
        ctx.lengths, ctx.period, ctx.shapes = lengths, period, (tuple(y.shape), tuple(y_hat.shape))
        return x0

    @staticmethod
    @once_differentiable
    def backward(ctx, gx0):
        gx0 = gx0.contiguous()
        B, T = ctx.shapes[0][0], ctx.shapes[0][-1]
        ldh = gx0.shape[2]
        half = 4 * B * ctx.period * ldh
        st = current_stream_ptr(gx0.device)
        grads = [None, None]
        with torch.cuda.device(gx0.device):
            for i in range(2):
                if ctx.needs_input_grad[i]:
                    grads[i] = torch.empty(ctx.shapes[i], dtype=torch.float32, device=gx0.device)
                    check(lib.dissc_period_fold_bwd(ctypes.c_void_p(gx0.data_ptr() + i * half), _ptr(ctx.lengths), B, T, ctx.period, T,
                                                    ldh, _ptr(grads[i]), st), "dissc_period_fold_bwd")
        return grads[0], grads[1], None, None


class MPDOutput:
    """what nn.MultiPeriodDiscriminator returns: per period i, scores[i] (= fmaps[i][5]), the six paired PRE-activation maps
    fmaps[i][j] [2 R[i], C_j, ld_j] (rows 0 .. R[i] - 1 from y, the rest from y_hat), their per-row device lengths lens[i][j]
    (int32 [2 R[i]], the two halves alike) and R[i] = B * period"""

    def __init__(self, scores, fmaps, lens, R):
        self.scores, self.fmaps, self.lens, self.R = scores, fmaps, lens, R


class MultiPeriodDiscriminator:
    """The trainable MultiPeriodDiscriminator (reference sr/models.py:263-286) under the reference's checkpoint keys
    ``discriminators.<i>.convs.<j>.{weight_g, weight_v, bias}`` (j = 0 .. 4) and ``discriminators.<i>.conv_post.{...}``, Conv2d
    shapes (weight_v [Cout, Cin, k, 1], weight_g [Cout, 1, 1, 1]): the ``mpd`` entry of a reference ``do_*`` checkpoint.

        D = nn.MultiPeriodDiscriminator().to("cuda:0"); D.load_state_dict(sd["mpd"])
        out = D(y, y_hat.detach(), lengths); loss_d, r_losses, g_losses = nn.discriminator_loss(out); loss_d.backward()
        out = D(y, y_hat, lengths, param_grads=False)
        (nn.feature_loss(out) + nn.generator_loss(out)[0] + 45 * mel.l1_loss(y, y_hat)).backward()

    parameters(): three flat leaves -- every weight_v, every weight_g, every bias of the 30 layers; their weight norm is one
    launch in each direction.  y and y_hat run as ONE batch [y ; y_hat] per period: the weights are packed once for both and
    every weight gradient is one pass over both.  No torch compute op on the path (allocation, views, autograd's own sums where a
    map feeds a layer and a loss)."""

    def __init__(self, periods=MPD_PERIODS, precision="fp32"):
        _prec(precision, "nn.MultiPeriodDiscriminator")
        self.precision = precision  # of convs.4 and conv_post, the conv1d layers; the strided layers are fp32
        self.periods = tuple(int(p) for p in periods)
        if not self.periods or any(not 1 <= p <= 65535 for p in self.periods):
            raise DisscError("nn.MultiPeriodDiscriminator: at least one period, each within 1 .. 65535")
        if 6 * len(self.periods) > GANLOSS_MAX_MAPS:
            raise DisscError(f"nn.MultiPeriodDiscriminator: {len(self.periods)} periods give more than {GANLOSS_MAX_MAPS} maps, "
                             "the most one loss launch takes")
        # (name, weight shape as the layers take it, bias length) in the reference's order
        self.layers = [(f"discriminators.{i}.{name}", (cout, cin, k), cout) for i in range(len(self.periods))
                       for name, cin, cout, k in _DISC_P_LAYERS]
        self.wn = WeightNorm([(s[0], s[1] * s[2]) for _, s, _ in self.layers], [nb for _, _, nb in self.layers])
        self.device = torch.device("cuda:0")
        self.v_flat = self.g_flat = self.bias_flat = None

    # -- nn.Module-like surface --------------------------------------------------------------------------------------
    def to(self, device):
        if isinstance(device, int):
            device = f"cuda:{device}"
        device = torch.device(device)
        if device.type != "cuda":
            raise DisscError("dissc_amd.nn.MultiPeriodDiscriminator runs on an MI355X only (device='cuda:N')")
        if device.index is None:
            device = torch.device("cuda:0")
        if self.v_flat is not None and device != self.device:
            raise DisscError("nn.MultiPeriodDiscriminator: choose the device before load_state_dict()")
        self.device = device
        return self

    def cuda(self, device=0):
        return self.to(device)

    def precision_report(self):
        """{layer name: (fwd, dgrad, wgrad)}: which directions of each layer run split-bf16 under this module's precision
        (nn.conv1d_precision for convs.4 and conv_post; the strided layers are fp32).  Host only."""
        conv1d_layers = [name for name, _, _, _ in _DISC_P_LAYERS[DISC_P_STRIDED_LAYERS:]]
        return _precision_report(self.precision, [(name, (s[1], s[0], s[2], 1) if name.split(".", 2)[2] in conv1d_layers else None)
                                                  for name, s, _ in self.layers])

    def _keys(self):
        keys = []
        for name, _, _ in self.layers:
            keys += [name + ".bias", name + ".weight_g", name + ".weight_v"]
        return keys

    def load_state_dict(self, sd, strict=True):
        """the reference's layout: weight_g [Cout, 1, 1, 1] / weight_v [Cout, Cin, k, 1] / bias [Cout] per Conv2d"""
        keys = self._keys()
        missing = [k for k in keys if k not in sd]
        unexpected = sorted(set(sd.keys()) - set(keys))
        if missing or (strict and unexpected):
            raise RuntimeError("Error(s) in loading state_dict for MultiPeriodDiscriminator: "
                               f"missing {missing[:5]}, unexpected {unexpected[:5]}")
        wn = self.wn
        v, g, b = torch.zeros(wn.total), torch.zeros(wn.total_rows), torch.zeros(wn.bias_total)
        for i, (name, shape, nb) in enumerate(self.layers):
            tv, tg, tb = (sd[name + s].detach().to("cpu", torch.float32) for s in (".weight_v", ".weight_g", ".bias"))
            if tuple(tv.shape) != shape + (1,) or tuple(tg.shape) != (shape[0], 1, 1, 1) or tuple(tb.shape) != (nb,):
                raise RuntimeError(f"size mismatch for {name}: weight_v {tuple(tv.shape)}, weight_g {tuple(tg.shape)}, bias "
                                   f"{tuple(tb.shape)}; expected {shape + (1,)}, {(shape[0], 1, 1, 1)}, {(nb,)}")
            v[wn.off[i]:wn.off[i] + tv.numel()] = tv.reshape(-1)
            g[wn.row_off[i]:wn.row_off[i] + shape[0]] = tg.reshape(-1)
            b[wn.bias_off[i]:wn.bias_off[i] + nb] = tb.reshape(-1)
        leaf = lambda t: t.to(self.device).contiguous().requires_grad_(True)
        self.v_flat, self.g_flat, self.bias_flat = leaf(v), leaf(g), leaf(b)
        return self

    def _loaded(self):
        if self.v_flat is None:
            raise RuntimeError("load_state_dict() first")

    def parameters(self):
        """the three flat leaves: v_flat, g_flat, bias_flat"""
        self._loaded()
        return [self.v_flat, self.g_flat, self.bias_flat]

    def zero_grad(self):
        for p in self.parameters():
            p.grad = None

    def _named(self, v, g, b):
        out = {}
        wn = self.wn
        for i, (name, shape, nb) in enumerate(self.layers):
            n = shape[0] * shape[1] * shape[2]
            out[name + ".bias"] = b[wn.bias_off[i]:wn.bias_off[i] + nb]
            out[name + ".weight_g"] = g[wn.row_off[i]:wn.row_off[i] + shape[0]].view(shape[0], 1, 1, 1)
            out[name + ".weight_v"] = v[wn.off[i]:wn.off[i] + n].view(shape + (1,))
        return out

    def named_grads(self):
        """{reference key: a view of its leaf's .grad} after a backward"""
        ps = self.parameters()
        if any(p.grad is None for p in ps):
            raise RuntimeError("named_grads(): run a backward first")
        return self._named(*(p.grad for p in ps))

    def leaf_shapes(self):
        """the shapes of parameters(), known before load_state_dict()"""
        return [(self.wn.total,), (self.wn.total_rows,), (self.wn.bias_total,)]

    def named_views(self, *tensors):
        """{reference key: its view, Conv2d shapes} of tensors shaped like parameters(), in that order and on any device (an
        optimiser's moments, say); the order of the keys is the reference module's named_parameters()"""
        _check_leaf_shaped(self, tensors)
        return self._named(*tensors)

    def named_leaves(self):
        """{reference key: the index in parameters() of the leaf that holds it}, in named_views()'s order"""
        out = {}
        for name, _, _ in self.layers:
            out.update({name + ".bias": 2, name + ".weight_g": 1, name + ".weight_v": 0})
        return out

    def state_dict(self):
        """host copies under the reference's unfolded keys and Conv2d shapes"""
        self._loaded()
        return {k: t.clone() for k, t in self._named(*(p.detach().cpu() for p in self.parameters())).items()}

    def folded(self, i):
        """discriminator i's weights g v / ||v|| as the forward folds them, under nn.discriminator_p's keys (detached device
        tensors [Cout, Cin, k] and [Cout])"""
        self._loaded()
        buf, _ = self.wn.forward(self.v_flat.detach(), self.g_flat.detach(), self.bias_flat.detach())
        wn, out = self.wn, {}
        for j, (name, _, _, _) in enumerate(_DISC_P_LAYERS):
            l = 6 * i + j
            shape, nb = self.layers[l][1], self.layers[l][2]
            out[name + ".weight"] = buf[wn.off[l]:wn.off[l] + shape[0] * shape[1] * shape[2]].view(shape)
            out[name + ".bias"] = buf[wn.total + wn.bias_off[l]:wn.total + wn.bias_off[l] + nb]
        return out

    # -- forward -------------------------------------------------------------------------------------------------------
    def forward(self, y, y_hat, lengths=None, param_grads=True):
        """y, y_hat: contiguous fp32 device tensors of ONE shape, [B, 1, T] or [B, T], with lengths[b] valid samples each (host
        counts; a device tensor is copied back; None = T) -> MPDOutput.  ValueError where torch's reflect pad would raise for one
        of the periods.  param_grads=False detaches the three leaves in front of the weight norm: a backward then reaches y_hat
        (and y) only and skips every weight- and bias-gradient kernel -- the generator's step, whose discriminator gradients the
        reference computes and throws away."""
        who = "nn.MultiPeriodDiscriminator"
        self._loaded()
        _check_wav(y, who), _check_wav(y_hat, who)
        if y.shape != y_hat.shape or y.device != y_hat.device or y.device != self.device:
            raise DisscError(f"{who}: y {tuple(y.shape)} and y_hat {tuple(y_hat.shape)} must have one shape, on {self.device}")
        B, T = y.shape[0], y.shape[-1]
        ln = _host_lengths(lengths, B, T, who)
        for p in self.periods:
            _check_reflect(ln, p, who)
        # the waveform's lengths and every period's every layer's row lengths (both halves) in one upload
        parts, where = [ln], []
        at = B
        for p in self.periods:
            rows = np.tile(np.repeat(-(-ln // p), p), 2)
            per = []
            for j in range(DISC_P_STRIDED_LAYERS + 1):
                if j:
                    rows = -(-rows // DISC_P_STRIDE)
                parts.append(rows)
                per.append(at)
                at += rows.shape[0]
            where.append(per)
        flat = torch.from_numpy(np.concatenate(parts).astype(np.int32)).to(self.device)
        wav_len = flat[:B]
        n = len(self.layers)
        leaves = (self.v_flat, self.g_flat, self.bias_flat) if param_grads else \
            (self.v_flat.detach(), self.g_flat.detach(), self.bias_flat.detach())
        wb = _WeightsFn.apply(*leaves, self.wn, [s for _, s, _ in self.layers])
        scores, fmaps, lens, Rs = [], [], [], []
        for i, p in enumerate(self.periods):
            rows2 = 2 * B * p
            ls = [flat[o:o + rows2] for o in where[i]]  # the fold's rows, then the four strided layers' outputs
            W = lambda j: (wb[6 * i + j], wb[n + 6 * i + j])
            x = _PairedFoldFn.apply(y, y_hat, p, wav_len)
            fm = []
            for j in range(DISC_P_STRIDED_LAYERS):
                x = conv1d_strided(x, *W(j), stride=DISC_P_STRIDE, lengths=ls[j], in_slope=LRELU_SLOPE if j else 1.0)
                fm.append(x)
            x = conv1d(x, *W(DISC_P_STRIDED_LAYERS), lengths=ls[-1], in_slope=LRELU_SLOPE, precision=self.precision)
            fm.append(x)
            x = conv1d(x, *W(DISC_P_STRIDED_LAYERS + 1), lengths=ls[-1], in_slope=LRELU_SLOPE, precision=self.precision)
            fm.append(x)
            scores.append(x)
            fmaps.append(fm)
            lens.append(ls[1:] + [ls[-1], ls[-1]])
            Rs.append(B * p)
        return MPDOutput(scores, fmaps, lens, Rs)

    __call__ = forward


def discriminator_loss(out):
    """reference sr/models.py:363-374 on an MPDOutput or MSDOutput of D(y, y_hat.detach()) -> (loss, r_losses, g_losses): loss =
    the sum over the discriminators of mean((1 - score_real)^2) + mean(score_gen^2) over the valid scores; r_losses / g_losses:
    device tensors [number of periods or scales] (no host copy, no sync).  One forward and one backward launch over the scores
    (each discriminator's last map, with that map's lengths)."""
    total, vals = gan_loss(DISC, out.scores, [ls[-1] for ls in out.lens], out.R)
    return total, vals[0], vals[1]


def generator_loss(out):
    """reference sr/models.py:377-383 -> (loss, gen_losses): the sum over the discriminators of mean((1 - score_gen)^2)"""
    total, vals = gan_loss(GEN, out.scores, [ls[-1] for ls in out.lens], out.R)
    return total, vals[0]


def feature_loss(out):
    """reference sr/models.py:352-360 -> loss = 2 * the sum over all maps (6 a period, 8 a scale) of every discriminator of
    mean |fmap_real - fmap_gen| over the valid positions, fmap = the leaky ReLU (0.1) of all but the last map and conv_post's
    output as it is.  One forward and one backward launch over all maps."""
    maps = [m for fm in out.fmaps for m in fm]
    lens = [t for ls in out.lens for t in ls]
    R = [r for r, fm in zip(out.R, out.fmaps) for _ in fm]
    slopes = [LRELU_SLOPE if j < len(fm) - 1 else 1.0 for fm in out.fmaps for j in range(len(fm))]
    return gan_loss(FM, maps, lens, R, slopes)[0]


# ---------------------------------------------------------------------------------------------------------------------
# The scale half of the GAN step (reference sr/models.py:285-333): spectral norm of a list of matrices (C ABI dissc_snorm_*,
# csrc/spectral_norm.hip) and nn.MultiScaleDiscriminator.  Discriminator 0 is spectrally normalised, and torch's spectral_norm runs
# one power iteration in EVERY training-mode forward of a wrapped conv: the reference's d(y) and d(y_hat) see W / sigma_1 and
# W / sigma_2, two different weights.  Scale 0 therefore runs as two chains of B rows; scales 1 and 2 run paired, as the periods do.
# ---------------------------------------------------------------------------------------------------------------------
def _bind_snorm():
    vp, i32, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    pll = ctypes.POINTER(ll)
    lib.dissc_snorm_create.argtypes = [i32, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(vp)]
    lib.dissc_snorm_destroy.argtypes, lib.dissc_snorm_destroy.restype = [vp], None
    lib.dissc_snorm_offsets.argtypes = [vp, pll, pll, pll, pll, pll, pll, pll]
    for name in ("chunk_rows", "span_cols", "wave_cols", "flat_span"):
        getattr(lib, "dissc_snorm_" + name).argtypes = []
    lib.dissc_snorm_forward.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp]
    lib.dissc_snorm_backward.argtypes = [vp, vp, vp, ctypes.POINTER(vp), vp, vp]


_bind_snorm()

SNORM_CHUNK_ROWS = int(lib.dissc_snorm_chunk_rows())  # rows per partial chunk of W^T u
SNORM_SPAN_COLS = int(lib.dissc_snorm_span_cols())    # columns per workgroup span of W^T u and v
SNORM_WAVE_COLS = int(lib.dissc_snorm_wave_cols())    # rows of up to this many columns: one wave; longer: one workgroup
SNORM_FLAT_SPAN = int(lib.dissc_snorm_flat_span())    # elements per workgroup of the passes over a tensor as a flat array
# (name, Cout, Cin / groups, k) of DiscriminatorS's eight layers, reference sr/models.py:289-295
_DISC_S_LAYERS = [("convs.0", 128, 1, 15), ("convs.1", 128, 32, 41), ("convs.2", 256, 8, 41), ("convs.3", 512, 16, 41),
                  ("convs.4", 1024, 32, 41), ("convs.5", 1024, 64, 41), ("convs.6", 1024, 1024, 5), ("conv_post", 1, 1024, 3)]


def _aligned_offsets(sizes):
    """([offset of each entry, 16-byte aligned], total floats)"""
    offs, at = [], 0
    for n in sizes:
        at = (at + 3) & ~3
        offs.append(at)
        at += n
    return offs, (at + 3) & ~3


class SpectralNorm:
    """torch.nn.utils.spectral_norm's weight for a whole list of matrices at once (dissc_snorm_*): ``shapes`` are the tensors'
    (rows, cols) = weight_orig seen as [Cout, Cin / groups * k].  ``off[i]`` places tensor i in the flat layout of ``total``
    floats (weight_orig, w, its gradient), ``u_off[i]`` / ``v_off[i]`` its power-iteration vectors in ``u_total`` / ``v_total``
    floats; every entry 16-byte aligned.  A state is one tensor [u | v | sigma per tensor] of ``state_total`` floats."""

    def __init__(self, shapes):
        n = len(shapes)
        rows = (ctypes.c_int * max(n, 1))(*[int(r) for r, _ in shapes])
        cols = (ctypes.c_int * max(n, 1))(*[int(c) for _, c in shapes])
        self._h = ctypes.c_void_p()
        check(lib.dissc_snorm_create(n, rows, cols, ctypes.byref(self._h)), "dissc_snorm_create")
        self.n, self.shapes = n, [(int(r), int(c)) for r, c in shapes]
        off, uoff, voff = ((ctypes.c_longlong * n)() for _ in range(3))
        tot, ut, vt, st = (ctypes.c_longlong(0) for _ in range(4))
        check(lib.dissc_snorm_offsets(self._h, off, uoff, voff, ctypes.byref(tot), ctypes.byref(ut), ctypes.byref(vt), ctypes.byref(st)),
              "dissc_snorm_offsets")
        self.off, self.u_off, self.v_off = list(off), list(uoff), list(voff)
        self.total, self.u_total, self.v_total, self.state_total = tot.value, ut.value, vt.value, st.value
        self.has_gaps = self.total != sum(r * c for r, c in self.shapes)

    def __del__(self):
        try:
            lib.dissc_snorm_destroy(self._h)
        except Exception:
            pass

    def split(self, state):
        """(u [u_total], v [v_total], sigma [n]): views of a state"""
        a, b = self.u_total, self.u_total + self.v_total
        return state[:a], state[a:b], state[b:b + self.n]

    def forward(self, w_flat, u_flat, v_flat, iterate=True, out=None, state=None):
        """-> (w, state): w = weight_orig / sigma in the flat layout, state = [u | v | sigma] as this call used them: after one
        power iteration from (u_flat, v_flat) with ``iterate``, else (u_flat, v_flat) themselves.  New tensors whose alignment
        gaps are zero, or ``out`` / ``state``; the inputs are never written."""
        who = "SpectralNorm.forward"
        _f32(w_flat, "w_flat", who), _f32(u_flat, "u_flat", who), _f32(v_flat, "v_flat", who)
        if w_flat.numel() != self.total or u_flat.numel() != self.u_total or v_flat.numel() != self.v_total:
            raise DisscError(f"{who}: w_flat / u_flat / v_flat must have {self.total} / {self.u_total} / {self.v_total} floats")
        dev = w_flat.device
        if out is None:
            out = (torch.zeros if self.has_gaps else torch.empty)(self.total, dtype=torch.float32, device=dev)
        if state is None:
            state = torch.zeros(self.state_total, dtype=torch.float32, device=dev)
        if _f32(out, "out", who).numel() != self.total or _f32(state, "state", who).numel() != self.state_total:
            raise DisscError(f"{who}: out / state must have {self.total} / {self.state_total} floats")
        with torch.cuda.device(dev):
            check(lib.dissc_snorm_forward(self._h, _ptr(w_flat), _ptr(u_flat), _ptr(v_flat), 1 if iterate else 0, _ptr(out), _ptr(state),
                                          current_stream_ptr(dev)), "dissc_snorm_forward")
        return out, state

    def backward(self, w_flat, state, gws, gw_out=None):
        """gws: the tensors' own gradients (None = zero) -> the gradient of weight_orig in the flat layout, with the state's u, v
        and sigma as constants"""
        who = "SpectralNorm.backward"
        _f32(w_flat, "w_flat", who), _f32(state, "state", who)
        if w_flat.numel() != self.total or state.numel() != self.state_total or len(gws) != self.n:
            raise DisscError(f"{who}: w_flat / state of {self.total} / {self.state_total} floats and {self.n} gradients expected")
        for i, t in enumerate(gws):
            if t is not None and _f32(t, f"gws[{i}]", who).numel() != self.shapes[i][0] * self.shapes[i][1]:
                raise DisscError(f"{who}: gws[{i}] has {t.numel()} elements, expected {self.shapes[i]}")
        dev = w_flat.device
        pw = (ctypes.c_void_p * self.n)(*[None if t is None else t.data_ptr() for t in gws])
        gw = gw_out if gw_out is not None else \
            (torch.zeros if self.has_gaps else torch.empty)(self.total, dtype=torch.float32, device=dev)
        if _f32(gw, "gw_out", who).numel() != self.total:
            raise DisscError(f"{who}: gw_out must have {self.total} floats")
        with torch.cuda.device(dev):
            check(lib.dissc_snorm_backward(self._h, _ptr(w_flat), _ptr(state), pw, _ptr(gw), current_stream_ptr(dev)),
                  "dissc_snorm_backward")
        return gw


class _SnWeightsFn(torch.autograd.Function):
    """(weight_orig flat, bias flat) with the buffers (u, v) -> every layer's weight W / sigma and bias, views of buffers made
    here, and the state [u | v | sigma] this call used (not differentiable; its u and v are the module's next buffers).  The
    Function saves weight_orig and that very state: no later call can write what it saved.  The backward is three launches."""

    @staticmethod
    def forward(ctx, w_flat, bias_flat, u_flat, v_flat, sn, dims, bias_off, bias_sizes, iterate):
        buf, state = sn.forward(w_flat, u_flat, v_flat, iterate)
        ctx.save_for_backward(w_flat, state)
        ctx.sn, ctx.bias_off, ctx.bias_sizes, ctx.nbias = sn, bias_off, bias_sizes, bias_flat.numel()
        ws = [buf[o:o + r * c].view(d) for o, (r, c), d in zip(sn.off, sn.shapes, dims)]
        bias = bias_flat.detach().clone()
        bs = [bias[o:o + n] for o, n in zip(bias_off, bias_sizes)]
        ctx.mark_non_differentiable(state)
        return tuple(ws + bs + [state])

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        w_flat, state = ctx.saved_tensors
        n = ctx.sn.n
        gw = gb = None
        if ctx.needs_input_grad[0]:
            gw = ctx.sn.backward(w_flat, state, [None if t is None else t.contiguous() for t in grads[:n]])
        if ctx.needs_input_grad[1]:
            gb = torch.zeros(ctx.nbias, dtype=torch.float32, device=w_flat.device)
            for o, nb, g in zip(ctx.bias_off, ctx.bias_sizes, grads[n:2 * n]):
                if g is not None:
                    gb[o:o + nb].copy_(g)
        return (gw, gb) + (None,) * 7


class _JoinFn(torch.autograd.Function):
    """[a ; b] along dim 0 as one paired map: two device copies into the halves of one allocation; the backward hands out the two
    contiguous row ranges of the gradient, no copy"""

    @staticmethod
    def forward(ctx, a, b):
        out = torch.empty((a.shape[0] + b.shape[0],) + tuple(a.shape[1:]), dtype=a.dtype, device=a.device)
        out[:a.shape[0]].copy_(a)
        out[a.shape[0]:].copy_(b)
        ctx.rows = a.shape[0]
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        g = g.contiguous()
        return g[:ctx.rows], g[ctx.rows:]


class _PairedPoolFn(torch.autograd.Function):
    """[2 B, 1, ldo]: mean_pool of y into the first half and of y_hat into the second, by two calls of dissc_mean_pool_fwd on the
    halves of one buffer; the backward runs dissc_mean_pool_bwd on a half only where that input requires a gradient"""

    @staticmethod
    def forward(ctx, y, y_hat, lengths):
        B, T = y.shape[0], y.shape[-1]
        ldo = _ceil4(T // 2 + 1)
        out = torch.zeros((2 * B, 1, ldo), dtype=torch.float32, device=y.device)
        half = 4 * B * ldo  # bytes; ldo % 4 == 0 keeps the second half 16-byte aligned
        st = current_stream_ptr(y.device)
        with torch.cuda.device(y.device):
            for i, w in enumerate((y, y_hat)):
                check(lib.dissc_mean_pool_fwd(_ptr(w), ctypes.c_void_p(out.data_ptr() + i * half), _ptr(lengths), B, 1, T, T, ldo, st),
                      "dissc_mean_pool_fwd")
        ctx.lengths, ctx.shapes = lengths, (tuple(y.shape), tuple(y_hat.shape))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        g = g.contiguous()
        B, T = ctx.shapes[0][0], ctx.shapes[0][-1]
        ldo = g.shape[2]
        half = 4 * B * ldo
        st = current_stream_ptr(g.device)
        grads = [None, None]
        with torch.cuda.device(g.device):
            for i in range(2):
                if ctx.needs_input_grad[i]:
                    grads[i] = torch.empty(ctx.shapes[i], dtype=torch.float32, device=g.device)
                    check(lib.dissc_mean_pool_bwd(ctypes.c_void_p(g.data_ptr() + i * half), _ptr(grads[i]), _ptr(ctx.lengths), B, 1, T, T,
                                                  ldo, st), "dissc_mean_pool_bwd")
        return grads[0], grads[1], None


def msd_row_lengths(ln):
    """host only: [scale][7] int64 arrays of 2 B row lengths (the halves alike) for utterances of ln[b] samples -- per scale the
    inputs of convs.0 .. convs.5 and then of the stride-1 layers behind them; scale i + 1's utterances have n // 2 + 1 samples
    (AvgPool1d(4, 2, padding=2); 0 stays 0)"""
    ln = np.asarray(ln, dtype=np.int64).reshape(-1)
    out = []
    for _ in range(3):
        rows = [np.tile(ln, 2)]
        for s, _ in DISC_S_GROUPED:
            rows.append(-(-rows[-1] // s))
        out.append(rows)
        ln = np.where(ln > 0, ln // 2 + 1, 0)
    return out


class MSDOutput(MPDOutput):
    """what nn.MultiScaleDiscriminator returns: MPDOutput's fields per scale i -- scores[i] (= fmaps[i][7]), the eight paired
    PRE-activation maps fmaps[i][j] [2 B, C_j, ld_j] (rows 0 .. B - 1 from y, the rest from y_hat), their per-row device lengths
    lens[i][j] (int32 [2 B], the two halves alike), R[i] = B -- and sigma, a device tensor [2, 8]: the sigmas of discriminator
    0's eight layers as the real half (sigma[0]) and the generated half (sigma[1]) used them"""

    def __init__(self, scores, fmaps, lens, R, sigma):
        super().__init__(scores, fmaps, lens, R)
        self.sigma = sigma


class MultiScaleDiscriminator:
    """The trainable MultiScaleDiscriminator (reference sr/models.py:310-333) under the reference's checkpoint keys: discriminator
    0 is spectrally normalised, ``discriminators.0.convs.<j>.{bias, weight_orig, weight_u, weight_v}`` (j = 0 .. 6) and
    ``discriminators.0.conv_post.{...}`` -- weight_u [Cout] and weight_v [Cin / groups * k] are the power iteration's BUFFERS --,
    discriminators 1 and 2 are weight-normalised, ``{bias, weight_g [Cout, 1, 1], weight_v [Cout, Cin / groups, k]}``: the ``msd``
    entry of a reference ``do_*`` checkpoint.

        D = nn.MultiScaleDiscriminator().to("cuda:0"); D.load_state_dict(sd["msd"])
        out = D(y, y_hat.detach(), lengths); loss_d, r_losses, g_losses = nn.discriminator_loss(out); loss_d.backward()
        out = D(y, y_hat, lengths, param_grads=False)
        (nn.feature_loss(out) + nn.generator_loss(out)[0]).backward()

    parameters(): five flat leaves -- discriminator 0's eight weight_orig and its eight biases, and every weight_v, every
    weight_g and every bias of the 16 layers of discriminators 1 and 2.  The two-sigma rule: a training-mode forward of the
    reference calls d(y) and then d(y_hat), and each call runs one power iteration, so y sees W / sigma_1 and y_hat sees
    W / sigma_2.  Scale 0 therefore runs as two chains of B rows with two folds, and its maps are joined by a copy; scales 1 and
    2 run as ONE batch [y ; y_hat] of pooled rows (weights packed once, every weight gradient one pass over both halves).
    state_dict() returns the current buffers: after n forwards, what torch's module holds after n forwards.  No torch compute
    op on the path (allocation, copies, views, autograd's own sums)."""

    def __init__(self, precision="fp32"):
        _prec(precision, "nn.MultiScaleDiscriminator")
        self.precision = precision  # of convs.6 and conv_post, the conv1d layers; the grouped layers are fp32
        shape = lambda cout, cig, k: (cout, cig, k)
        self.layers0 = [(f"discriminators.0.{name}", shape(cout, cig, k), cout) for name, cout, cig, k in _DISC_S_LAYERS]
        self.layers12 = [(f"discriminators.{i}.{name}", shape(cout, cig, k), cout) for i in (1, 2) for name, cout, cig, k in _DISC_S_LAYERS]
        self.sn = SpectralNorm([(s[0], s[1] * s[2]) for _, s, _ in self.layers0])
        self.bias0_sizes = [nb for _, _, nb in self.layers0]
        self.bias0_off, self.bias0_total = _aligned_offsets(self.bias0_sizes)
        self.wn = WeightNorm([(s[0], s[1] * s[2]) for _, s, _ in self.layers12], [nb for _, _, nb in self.layers12])
        self.device = torch.device("cuda:0")
        self.w_orig = self.bias0 = self.v_flat = self.g_flat = self.bias_flat = None  # the five leaves
        self.u = self.v = None                                                        # discriminator 0's buffers, flat

    # -- nn.Module-like surface --------------------------------------------------------------------------------------
    def to(self, device):
        if isinstance(device, int):
            device = f"cuda:{device}"
        device = torch.device(device)
        if device.type != "cuda":
            raise DisscError("dissc_amd.nn.MultiScaleDiscriminator runs on an MI355X only (device='cuda:N')")
        if device.index is None:
            device = torch.device("cuda:0")
        if self.w_orig is not None and device != self.device:
            raise DisscError("nn.MultiScaleDiscriminator: choose the device before load_state_dict()")
        self.device = device
        return self

    def cuda(self, device=0):
        return self.to(device)

    def precision_report(self):
        """{layer name: (fwd, dgrad, wgrad)}: which directions of each layer run split-bf16 under this module's precision
        (nn.conv1d_precision for convs.6 and conv_post; the grouped layers are fp32).  Host only."""
        conv1d_layers = [name for name, _, _, _ in _DISC_S_LAYERS[len(DISC_S_GROUPED):]]
        return _precision_report(self.precision, [(name, (s[1], s[0], s[2], 1) if name.split(".", 2)[2] in conv1d_layers else None)
                                                  for name, s, _ in self.layers0 + self.layers12])

    def _keys(self):
        keys = []
        for name, _, _ in self.layers0:
            keys += [name + ".bias", name + ".weight_orig", name + ".weight_u", name + ".weight_v"]
        for name, _, _ in self.layers12:
            keys += [name + ".bias", name + ".weight_g", name + ".weight_v"]
        return keys

    def load_state_dict(self, sd, strict=True):
        """the reference's layout: Conv1d shapes, weight_u [Cout] and weight_v [Cin / groups * k] for discriminator 0"""
        keys = self._keys()
        missing = [k for k in keys if k not in sd]
        unexpected = sorted(set(sd.keys()) - set(keys))
        if missing or (strict and unexpected):
            raise RuntimeError("Error(s) in loading state_dict for MultiScaleDiscriminator: "
                               f"missing {missing[:5]}, unexpected {unexpected[:5]}")
        get = lambda k: sd[k].detach().to("cpu", torch.float32)

        def expect(name, what, t, shape):
            if tuple(t.shape) != tuple(shape):
                raise RuntimeError(f"size mismatch for {name}.{what}: {tuple(t.shape)}, expected {tuple(shape)}")
            return t.reshape(-1)

        sn, wn = self.sn, self.wn
        w, b0, u, v0 = torch.zeros(sn.total), torch.zeros(self.bias0_total), torch.zeros(sn.u_total), torch.zeros(sn.v_total)
        for i, (name, shape, nb) in enumerate(self.layers0):
            r, c = sn.shapes[i]
            w[sn.off[i]:sn.off[i] + r * c] = expect(name, "weight_orig", get(name + ".weight_orig"), shape)
            u[sn.u_off[i]:sn.u_off[i] + r] = expect(name, "weight_u", get(name + ".weight_u"), (r,))
            v0[sn.v_off[i]:sn.v_off[i] + c] = expect(name, "weight_v", get(name + ".weight_v"), (c,))
            b0[self.bias0_off[i]:self.bias0_off[i] + nb] = expect(name, "bias", get(name + ".bias"), (nb,))
        v, g, b = torch.zeros(wn.total), torch.zeros(wn.total_rows), torch.zeros(wn.bias_total)
        for i, (name, shape, nb) in enumerate(self.layers12):
            v[wn.off[i]:wn.off[i] + shape[0] * shape[1] * shape[2]] = expect(name, "weight_v", get(name + ".weight_v"), shape)
            g[wn.row_off[i]:wn.row_off[i] + shape[0]] = expect(name, "weight_g", get(name + ".weight_g"), (shape[0], 1, 1))
            b[wn.bias_off[i]:wn.bias_off[i] + nb] = expect(name, "bias", get(name + ".bias"), (nb,))
        leaf = lambda t: t.to(self.device).contiguous().requires_grad_(True)
        self.w_orig, self.bias0, self.v_flat, self.g_flat, self.bias_flat = leaf(w), leaf(b0), leaf(v), leaf(g), leaf(b)
        self.u, self.v = u.to(self.device), v0.to(self.device)
        return self

    def _loaded(self):
        if self.w_orig is None:
            raise RuntimeError("load_state_dict() first")

    def parameters(self):
        """the five flat leaves: discriminator 0's weight_orig and bias, discriminators 1 and 2's weight_v, weight_g and bias"""
        self._loaded()
        return [self.w_orig, self.bias0, self.v_flat, self.g_flat, self.bias_flat]

    def zero_grad(self):
        for p in self.parameters():
            p.grad = None

    def _named(self, w, b0, v, g, b):
        out = {}
        sn, wn = self.sn, self.wn
        for i, (name, shape, nb) in enumerate(self.layers0):
            out[name + ".bias"] = b0[self.bias0_off[i]:self.bias0_off[i] + nb]
            out[name + ".weight_orig"] = w[sn.off[i]:sn.off[i] + shape[0] * shape[1] * shape[2]].view(shape)
        for i, (name, shape, nb) in enumerate(self.layers12):
            out[name + ".bias"] = b[wn.bias_off[i]:wn.bias_off[i] + nb]
            out[name + ".weight_g"] = g[wn.row_off[i]:wn.row_off[i] + shape[0]].view(shape[0], 1, 1)
            out[name + ".weight_v"] = v[wn.off[i]:wn.off[i] + shape[0] * shape[1] * shape[2]].view(shape)
        return out

    def named_grads(self):
        """{reference key of a PARAMETER: a view of its leaf's .grad} after a backward"""
        ps = self.parameters()
        if any(p.grad is None for p in ps):
            raise RuntimeError("named_grads(): run a backward first")
        return self._named(*(p.grad for p in ps))

    def leaf_shapes(self):
        """the shapes of parameters(), known before load_state_dict()"""
        return [(self.sn.total,), (self.bias0_total,), (self.wn.total,), (self.wn.total_rows,), (self.wn.bias_total,)]

    def named_views(self, *tensors):
        """{reference key of a PARAMETER: its view} of tensors shaped like parameters(), in that order and on any device (an
        optimiser's moments, say); discriminator 0's weight_u / weight_v are buffers and stay out.  The order of the keys is the
        reference module's named_parameters()"""
        _check_leaf_shaped(self, tensors)
        return self._named(*tensors)

    def named_leaves(self):
        """{reference key of a PARAMETER: the index in parameters() of the leaf that holds it}, in named_views()'s order"""
        out = {}
        for name, _, _ in self.layers0:
            out.update({name + ".bias": 1, name + ".weight_orig": 0})
        for name, _, _ in self.layers12:
            out.update({name + ".bias": 4, name + ".weight_g": 3, name + ".weight_v": 2})
        return out

    def state_dict(self):
        """host copies under the reference's keys and Conv1d shapes, with discriminator 0's CURRENT weight_u / weight_v"""
        self._loaded()
        out = {k: t.clone() for k, t in self._named(*(p.detach().cpu() for p in self.parameters())).items()}
        u, v = self.u.cpu(), self.v.cpu()
        for i, (name, _, _) in enumerate(self.layers0):
            r, c = self.sn.shapes[i]
            out[name + ".weight_u"] = u[self.sn.u_off[i]:self.sn.u_off[i] + r].clone()
            out[name + ".weight_v"] = v[self.sn.v_off[i]:self.sn.v_off[i] + c].clone()
        return out

    def _dict0(self, outs):
        n = self.sn.n
        return {f"{name}.{what}": outs[j + k * n] for j, (name, _, _, _) in enumerate(_DISC_S_LAYERS) for k, what in enumerate(("weight", "bias"))}

    def folded(self, i):
        """discriminator i's weights as a forward folds them, under nn.discriminator_s's keys (detached device tensors): for
        i = 0, weight_orig / sigma at the CURRENT buffers with no power iteration (torch's eval())"""
        self._loaded()
        if i == 0:
            with torch.no_grad():
                outs = _SnWeightsFn.apply(self.w_orig.detach(), self.bias0.detach(), self.u, self.v, self.sn,
                                          [s for _, s, _ in self.layers0], self.bias0_off, self.bias0_sizes, False)
            return self._dict0(outs)
        if i not in (1, 2):
            raise DisscError("nn.MultiScaleDiscriminator.folded: the discriminators are 0, 1 and 2")
        buf, _ = self.wn.forward(self.v_flat.detach(), self.g_flat.detach(), self.bias_flat.detach())
        wn, out = self.wn, {}
        for j, (name, _, _, _) in enumerate(_DISC_S_LAYERS):
            l = 8 * (i - 1) + j
            shape, nb = self.layers12[l][1], self.layers12[l][2]
            out[name + ".weight"] = buf[wn.off[l]:wn.off[l] + shape[0] * shape[1] * shape[2]].view(shape)
            out[name + ".bias"] = buf[wn.total + wn.bias_off[l]:wn.total + wn.bias_off[l] + nb]
        return out

    # -- forward -------------------------------------------------------------------------------------------------------
    def forward(self, y, y_hat, lengths=None, param_grads=True, power_iteration=True):
        """y, y_hat: contiguous fp32 device tensors of ONE shape, [B, 1, T] or [B, T], with lengths[b] valid samples each (host
        counts; a device tensor is copied back; None = T) -> MSDOutput.  power_iteration=True is the reference's train() mode:
        discriminator 0's buffers advance by one iteration in front of y's chain and by another in front of y_hat's;
        False is its eval(): no iteration, both chains use weight_orig / sigma at the current buffers.  param_grads=False
        detaches the five leaves in front of both norms: a backward then reaches y_hat (and y) only and skips every weight- and
        bias-gradient kernel; the power iterations still run (the reference's generator step iterates too)."""
        who = "nn.MultiScaleDiscriminator"
        self._loaded()
        _check_wav(y, who), _check_wav(y_hat, who)
        if y.shape != y_hat.shape or y.device != y_hat.device or y.device != self.device:
            raise DisscError(f"{who}: y {tuple(y.shape)} and y_hat {tuple(y_hat.shape)} must have one shape, on {self.device}")
        B, T = y.shape[0], y.shape[-1]
        ln = _host_lengths(lengths, B, T, who)
        # every scale's every layer's row lengths (both halves) in one upload; a scale's first entry is also the lengths its input
        # rows have for the pool behind it
        flat = torch.from_numpy(np.concatenate([r for rows in msd_row_lengths(ln) for r in rows]).astype(np.int32)).to(self.device)
        L = [[flat[(7 * i + j) * 2 * B:(7 * i + j + 1) * 2 * B] for j in range(7)] for i in range(3)]
        leaves = self.parameters() if param_grads else [p.detach() for p in self.parameters()]
        # scale 0: two folds, two chains of B rows, joined maps
        lens0 = [t[:B] for t in L[0]]
        halves, sigma = [], torch.empty((2, self.sn.n), dtype=torch.float32, device=self.device)
        for h, wav in enumerate((y, y_hat)):
            outs = _SnWeightsFn.apply(leaves[0], leaves[1], self.u, self.v, self.sn, [s for _, s, _ in self.layers0], self.bias0_off,
                                      self.bias0_sizes, bool(power_iteration))
            self.u, self.v, sg = self.sn.split(outs[-1])
            sigma[h].copy_(sg)
            halves.append(_disc_s_layers(_wav_rows4(wav), self._dict0(outs), lens0, self.precision))
        fmaps = [[_JoinFn.apply(a, b) for a, b in zip(*halves)]]
        # scales 1 and 2: one weight-norm launch for their 16 layers, one paired chain of 2 B pooled rows each
        n = len(self.layers12)
        wb = _WeightsFn.apply(leaves[2], leaves[3], leaves[4], self.wn, [s for _, s, _ in self.layers12])
        x = _PairedPoolFn.apply(y, y_hat, L[0][0][:B])
        for i in (1, 2):
            if i == 2:
                x = _MeanPoolFn.apply(x, L[1][0])
            W = {f"{name}.{what}": wb[k * n + 8 * (i - 1) + j] for j, (name, _, _, _) in enumerate(_DISC_S_LAYERS)
                 for k, what in enumerate(("weight", "bias"))}
            fmaps.append(_disc_s_layers(x, W, L[i], self.precision))
        lens = [ls[1:] + [ls[-1], ls[-1]] for ls in L]
        return MSDOutput([fm[-1] for fm in fmaps], fmaps, lens, [B, B, B], sigma)

    __call__ = forward


# ---------------------------------------------------------------------------------------------------------------------
# nn.AdamW: torch.optim.AdamW's update over all leaves of an optimiser in one launch (dissc_adamw_step, csrc/adamw.hip), and the
# conversion of its state to and from the reference's per-layer parameter list (the optim_g / optim_d of a do_* checkpoint).
# ---------------------------------------------------------------------------------------------------------------------
def _bind_adamw():
    vp, i32, ll, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double
    pp, pll = ctypes.POINTER(vp), ctypes.POINTER(ll)
    lib.dissc_adamw_chunk.argtypes = lib.dissc_adamw_max_tensors.argtypes = []
    lib.dissc_adamw_step.argtypes = [i32, pp, pp, pp, pp, pll, pll, f64, f64, f64, f64, f64, vp]


_bind_adamw()

ADAMW_CHUNK = int(lib.dissc_adamw_chunk())              # elements per workgroup
ADAMW_MAX_TENSORS = int(lib.dissc_adamw_max_tensors())  # tensors per optimiser: one launch steps them all


class AdamW:
    """torch.optim.AdamW (amsgrad False, maximize False) over up to ADAMW_MAX_TENSORS float32 device leaves, one launch per step().

        opt = nn.AdamW(D.parameters() + S.parameters(), lr=2e-4, betas=(0.8, 0.99)); loss.backward(); opt.step(); opt.lr *= 0.999

    ``lr`` is a plain attribute read at each step.  A leaf whose .grad is None is skipped entirely, as torch skips it: no state,
    no step count.  state_dict() / load_state_dict() use torch's format over the optimiser's own leaves (state[i] = {step: float32
    scalar, exp_avg, exp_avg_sq}; one param group with torch's keys and ``initial_lr``): a torch.optim.AdamW over the same leaves
    loads it, and this class loads torch's."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        self.params = list(params)
        if not 1 <= len(self.params) <= ADAMW_MAX_TENSORS:
            raise DisscError(f"nn.AdamW: {len(self.params)} tensors; one launch steps 1 .. {ADAMW_MAX_TENSORS}")
        for i, p in enumerate(self.params):
            if not (isinstance(p, torch.Tensor) and p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.is_leaf
                    and p.numel() >= 1):
                raise DisscError(f"nn.AdamW: params[{i}] must be a non-empty contiguous float32 CUDA leaf tensor")
            if p.device != self.params[0].device:
                raise DisscError(f"nn.AdamW: params[{i}] is on {p.device}, params[0] on {self.params[0].device}")
        spans = sorted((p.data_ptr(), p.data_ptr() + 4 * p.numel(), i) for i, p in enumerate(self.params))
        for (_, end, i), (start, _, j) in zip(spans, spans[1:]):
            if start < end:
                raise DisscError(f"nn.AdamW: params[{i}] and params[{j}] share memory; each element is stepped by one tensor")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        self.lr, self.initial_lr = float(lr), float(lr)
        self.betas, self.eps, self.weight_decay = (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.state = {}  # index in params -> {"step": int, "exp_avg", "exp_avg_sq"}

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    @torch.no_grad()
    def step(self):
        todo = [i for i, p in enumerate(self.params) if p.grad is not None]
        for i in todo:
            p, g = self.params[i], self.params[i].grad
            if g.shape != p.shape or g.dtype != torch.float32 or g.device != p.device or not g.is_contiguous() or g.is_sparse:
                raise DisscError(f"nn.AdamW: the grad of params[{i}] is {tuple(g.shape)} {g.dtype} on {g.device}; a contiguous "
                                 f"float32 tensor of the shape {tuple(p.shape)} on {p.device} expected")
        if not todo:
            return
        for i in todo:
            if i not in self.state:
                self.state[i] = {"step": 0, "exp_avg": torch.zeros_like(self.params[i]), "exp_avg_sq": torch.zeros_like(self.params[i])}
        n = len(todo)
        st = [self.state[i] for i in todo]
        arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
        numel = (ctypes.c_longlong * n)(*[self.params[i].numel() for i in todo])
        t = (ctypes.c_longlong * n)(*[s["step"] + 1 for s in st])
        dev = self.params[0].device
        with torch.cuda.device(dev):
            check(lib.dissc_adamw_step(n, arr([self.params[i] for i in todo]), arr([self.params[i].grad for i in todo]),
                                       arr([s["exp_avg"] for s in st]), arr([s["exp_avg_sq"] for s in st]), numel, t, float(self.lr),
                                       self.betas[0], self.betas[1], self.eps, self.weight_decay, current_stream_ptr(dev)),
                  "dissc_adamw_step")
        for s in st:
            s["step"] += 1

    def state_dict(self):
        """torch's format; the moments are the optimiser's own tensors, as torch returns its own"""
        state = {i: {"step": torch.tensor(float(s["step"]), dtype=torch.float32), "exp_avg": s["exp_avg"], "exp_avg_sq": s["exp_avg_sq"]}
                 for i, s in sorted(self.state.items())}
        group = {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "decoupled_weight_decay": True, "initial_lr": self.initial_lr, "params": list(range(len(self.params)))}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        if len(groups) != 1 or list(groups[0]["params"]) != list(range(len(self.params))):
            raise DisscError(f"nn.AdamW.load_state_dict: one param group over {len(self.params)} tensors expected")
        g = groups[0]
        if g.get("amsgrad", False) or g.get("maximize", False) or not g.get("decoupled_weight_decay", True):
            raise DisscError("nn.AdamW.load_state_dict: amsgrad, maximize and coupled weight decay are not supported")
        new = {}
        for i, s in sd["state"].items():
            i = int(i)
            if not 0 <= i < len(self.params):
                raise DisscError(f"nn.AdamW.load_state_dict: state[{i}] is outside the optimiser's {len(self.params)} tensors")
            p = self.params[i]
            if tuple(s["exp_avg"].shape) != tuple(p.shape) or tuple(s["exp_avg_sq"].shape) != tuple(p.shape):
                raise DisscError(f"nn.AdamW.load_state_dict: state[{i}] has the shape {tuple(s['exp_avg'].shape)}, params[{i}] "
                                 f"{tuple(p.shape)}")
            step = float(s["step"])
            if step != int(step) or step < 0:
                raise DisscError(f"nn.AdamW.load_state_dict: state[{i}]['step'] = {step} is no step count")
            own = lambda t: t.detach().to(p.device, torch.float32).contiguous().clone()
            new[i] = {"step": int(step), "exp_avg": own(s["exp_avg"]), "exp_avg_sq": own(s["exp_avg_sq"])}
        self.state = new
        self.lr, self.betas, self.eps = float(g["lr"]), (float(g["betas"][0]), float(g["betas"][1])), float(g["eps"])
        self.weight_decay, self.initial_lr = float(g["weight_decay"]), float(g.get("initial_lr", g["lr"]))


def _module_leaf_ranges(modules):
    out, at = [], 0
    for m in modules:
        n = len(m.leaf_shapes())
        out.append((m, at, at + n))
        at += n
    return out, at


def optimizer_state_to_reference(opt, modules):
    """The state dictionary of an optimiser over the flat leaves of ``modules`` (their parameters() one after the other; ``opt``
    is the optimiser or its state_dict(), ours or torch's) -> torch's dictionary over the reference's PER-LAYER parameter list:
    indices 0 .. n - 1 in the order of the modules' named_views(), which is the reference modules' named_parameters() (optim_d:
    [msd, mpd], reference sr/train.py chains msd.parameters() first), every moment with the shape of state_dict() at its key, every
    parameter of one leaf with that leaf's step.  Host tensors out; works on CPU tensors."""
    sd = opt.state_dict() if hasattr(opt, "state_dict") else opt
    ranges, n_leaves = _module_leaf_ranges(modules)
    groups = sd["param_groups"]
    if len(groups) != 1 or list(groups[0]["params"]) != list(range(n_leaves)):
        raise DisscError(f"optimizer_state_to_reference: one param group over the modules' {n_leaves} leaves expected")
    state, k = {}, 0
    for m, a, b in ranges:
        present = [i for i in range(a, b) if i in sd["state"]]
        zeros = [torch.zeros(shape) for shape in m.leaf_shapes()] if len(present) < b - a else None  # stand-ins of leaves without state
        pick = lambda what: m.named_views(*[sd["state"][i][what].detach().cpu() if i in sd["state"] else zeros[i - a] for i in range(a, b)])
        ms, vs = pick("exp_avg"), pick("exp_avg_sq")
        for key, j in m.named_leaves().items():
            if a + j in sd["state"]:
                state[k] = {"step": torch.tensor(float(sd["state"][a + j]["step"]), dtype=torch.float32),
                            "exp_avg": ms[key].clone(), "exp_avg_sq": vs[key].clone()}
            k += 1
    group = dict(groups[0])
    group["params"] = list(range(k))
    return {"state": state, "param_groups": [group]}


def optimizer_state_from_reference(sd, modules):
    """The inverse: torch's dictionary over the reference's per-layer parameters -> the dictionary over the modules' flat leaves
    (host tensors; the alignment gaps of a leaf get zero moments).  Refused: a parameter count or a shape other than the modules',
    and per-parameter steps that differ within one leaf -- a reference checkpoint never has them, all its parameters step
    together."""
    ranges, n_leaves = _module_leaf_ranges(modules)
    groups = sd["param_groups"]
    state, k = {}, 0
    for m, a, b in ranges:
        shapes = m.leaf_shapes()
        ms, vs = [torch.zeros(s) for s in shapes], [torch.zeros(s) for s in shapes]
        vm, vv, leaves = m.named_views(*ms), m.named_views(*vs), m.named_leaves()
        steps = {}  # leaf -> {step or None of each of its parameters}
        for key, view in vm.items():
            leaf = a + leaves[key]
            s = sd["state"].get(k, None)
            steps.setdefault(leaf, set()).add(None if s is None else float(s["step"]))
            if s is not None:
                for what, dst in (("exp_avg", view), ("exp_avg_sq", vv[key])):
                    if tuple(s[what].shape) != tuple(dst.shape):
                        raise DisscError(f"optimizer_state_from_reference: parameter {k} ({key}) has {what} of the shape "
                                         f"{tuple(s[what].shape)}, expected {tuple(dst.shape)}")
                    dst.copy_(s[what].detach().to("cpu", torch.float32))
            k += 1
        for leaf, seen in steps.items():
            if len(seen) != 1:
                raise DisscError(f"optimizer_state_from_reference: the parameters of flat leaf {leaf} of {type(m).__name__} have "
                                 f"different steps {sorted(seen, key=str)}; one leaf steps as a whole")
            step = next(iter(seen))
            if step is not None:
                state[leaf] = {"step": torch.tensor(step, dtype=torch.float32), "exp_avg": ms[leaf - a], "exp_avg_sq": vs[leaf - a]}
    if len(groups) != 1 or list(groups[0]["params"]) != list(range(k)):
        raise DisscError(f"optimizer_state_from_reference: one param group over the modules' {k} parameters expected, got "
                         f"{[len(g['params']) for g in groups]}")
    group = dict(groups[0])
    group["params"] = list(range(n_leaves))
    return {"state": state, "param_groups": [group]}
