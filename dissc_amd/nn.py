"""Differentiable layers for training the vocoder's generator on the MI355X (C ABI ``dissc_convgrad_*``,
csrc/conv_grad.hip, and ``dissc_convtgrad_*``, csrc/conv_grad_t.hip).

    y = nn.conv1d(x, weight, bias, lengths=lengths, dilation=d, in_slope=0.1, add=res)   # a torch.autograd.Function
    y = nn.resblock1(x, weights, k)                                                       # reference sr/models.py:34-41
    y = nn.conv_transpose1d(x, weight, bias, stride=u, lengths=lengths, in_slope=0.1)     # the upsamplers ups[i]

``conv1d`` is the stride-1 "same" Conv1d that 92 of the generator's 97 conv layers are, with dissc_conv1d's conventions:
the leaky ReLU of the INPUT is applied on load (``in_slope``; 1.0 = none), ``add`` is a residual added in the epilogue,
positions at and beyond ``lengths[b]`` are read as zero and never written.  Forward and the data gradient run on the direct
MFMA conv kernels, the weight gradient on its own MFMA kernel with fixed-order partial sums (no atomics: bit-reproducible).
The weights are a DEVICE tensor and are packed on the device on every call, because they change every step in training.
No torch compute op on the hot path, no CPU fallback.  First order only.
"""
import ctypes

import torch
from torch.autograd.function import once_differentiable

from ._lib import DisscError, check, current_stream_ptr, lib

WGRAD_CHUNK = 64  # DISSC_CONVGRAD_CHUNK: time positions per chunk of the weight-gradient kernel
LRELU_SLOPE = 0.1  # reference sr/models.py:13


def _bind():
    vp, i32, sz, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_float
    lib.dissc_convgrad_create.argtypes = [i32, i32, i32, i32, ctypes.POINTER(vp)]
    lib.dissc_convgrad_destroy.argtypes = [vp]
    lib.dissc_convgrad_destroy.restype = None
    lib.dissc_convgrad_set_weights.argtypes = [vp, vp, vp, vp]
    lib.dissc_convgrad_forward.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, vp]
    lib.dissc_convgrad_partials.argtypes = [vp, i32, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    lib.dissc_convgrad_workspace_bytes.argtypes = [vp, i32, i32]
    lib.dissc_convgrad_workspace_bytes.restype = sz
    lib.dissc_convgrad_backward.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, f32, vp, vp, vp, vp, sz, vp]
    lib.dissc_convtgrad_create.argtypes = [i32, i32, i32, i32, ctypes.POINTER(vp)]
    lib.dissc_convtgrad_destroy.argtypes = [vp]
    lib.dissc_convtgrad_destroy.restype = None
    lib.dissc_convtgrad_set_weights.argtypes = [vp, vp, vp, vp]
    lib.dissc_convtgrad_forward.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, f32, vp]
    lib.dissc_convtgrad_partials.argtypes = [vp, i32, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    lib.dissc_convtgrad_workspace_bytes.argtypes = [vp, i32, i32]
    lib.dissc_convtgrad_workspace_bytes.restype = sz
    lib.dissc_convtgrad_backward.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, f32, vp, vp, vp, vp, sz, vp]


_bind()

_handles = {}     # (Cin, Cout, k, dilation, device) -> handle; device None: host-only queries
_workspaces = {}  # device -> uint8 tensor, grown on demand (calls on one device are stream-ordered)


def _handle(Cin, Cout, k, dilation, device=None):
    key = (int(Cin), int(Cout), int(k), int(dilation), None if device is None else torch.device(device))
    h = _handles.get(key)
    if h is None:
        h = ctypes.c_void_p()
        check(lib.dissc_convgrad_create(key[0], key[1], key[2], key[3], ctypes.byref(h)), "dissc_convgrad_create")
        _handles[key] = h
    return h


def wgrad_partials(B, Lmax, Cin, Cout, k):
    """(P, pairs): the weight gradient of a [Cout, Cin, k] layer over B utterances of up to Lmax positions is summed in P
    partials; partial p takes the (utterance, chunk) pairs [p * pairs, (p + 1) * pairs) of the utterance-major list with
    ceil(Lmax / WGRAD_CHUNK) chunks per utterance.  A function of the shape only (host only, no GPU needed)."""
    P, pairs = ctypes.c_int(0), ctypes.c_int(0)
    check(lib.dissc_convgrad_partials(_handle(Cin, Cout, k, 1), int(B), int(Lmax), ctypes.byref(P), ctypes.byref(pairs)),
          "dissc_convgrad_partials")
    return P.value, pairs.value


def workspace_bytes(B, Lmax, Cin, Cout, k):
    """bytes of the backward's workspace (host only)"""
    return int(lib.dissc_convgrad_workspace_bytes(_handle(Cin, Cout, k, 1), int(B), int(Lmax)))


def _handle_t(Cin, Cout, k, stride, device=None):
    key = ("T", int(Cin), int(Cout), int(k), int(stride), None if device is None else torch.device(device))
    h = _handles.get(key)
    if h is None:
        h = ctypes.c_void_p()
        check(lib.dissc_convtgrad_create(key[1], key[2], key[3], key[4], ctypes.byref(h)), "dissc_convtgrad_create")
        _handles[key] = h
    return h


def wgrad_partials_transpose(B, Lmax, Cin, Cout, k, stride):
    """wgrad_partials for conv_transpose1d's weight gradient [Cin, Cout, k]: Lmax and the chunks are INPUT positions (a chunk
    is stride * WGRAD_CHUNK columns of the output's gradient).  A function of the shape only (host only)."""
    P, pairs = ctypes.c_int(0), ctypes.c_int(0)
    check(lib.dissc_convtgrad_partials(_handle_t(Cin, Cout, k, stride), int(B), int(Lmax), ctypes.byref(P), ctypes.byref(pairs)),
          "dissc_convtgrad_partials")
    return P.value, pairs.value


def workspace_bytes_transpose(B, Lmax, Cin, Cout, k, stride):
    """bytes of conv_transpose1d's backward workspace (host only)"""
    return int(lib.dissc_convtgrad_workspace_bytes(_handle_t(Cin, Cout, k, stride), int(B), int(Lmax)))


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


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class _Conv1dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, add, lengths, dilation, in_slope):
        B, Cin, ld = x.shape
        Cout, _, k = weight.shape
        h = _handle(Cin, Cout, k, dilation, x.device)
        st = current_stream_ptr(x.device)
        with torch.cuda.device(x.device):
            check(lib.dissc_convgrad_set_weights(h, _ptr(weight), _ptr(bias), st), "dissc_convgrad_set_weights")
            y = torch.zeros((B, Cout, ld), dtype=torch.float32, device=x.device) if lengths is not None else \
                torch.empty((B, Cout, ld), dtype=torch.float32, device=x.device)
            check(lib.dissc_convgrad_forward(h, _ptr(x), _ptr(add), _ptr(y), _ptr(lengths), B, ld, ld, ld, float(in_slope), st),
                  "dissc_convgrad_forward")
        ctx.save_for_backward(x, weight)  # never y
        ctx.lengths, ctx.dilation, ctx.in_slope = lengths, int(dilation), float(in_slope)
        ctx.has_bias, ctx.has_add = bias is not None, add is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        B, Cin, ld = x.shape
        Cout, _, k = weight.shape
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        need_add = ctx.has_add and ctx.needs_input_grad[3]
        gy = gy.contiguous()
        gx = gw = gb = ws = None
        if need_x or need_w or need_b:
            h = _handle(Cin, Cout, k, ctx.dilation, x.device)
            st = current_stream_ptr(x.device)
            with torch.cuda.device(x.device):
                if need_x:  # another layer sharing the handle may have run since the forward: pack again (device only)
                    check(lib.dissc_convgrad_set_weights(h, _ptr(weight), None, st), "dissc_convgrad_set_weights")
                    gx = torch.empty_like(x)
                if need_w:
                    gw = torch.empty_like(weight)
                if need_b:
                    gb = torch.empty(Cout, dtype=torch.float32, device=x.device)
                nws = 0
                if need_w or need_b:
                    nws = int(lib.dissc_convgrad_workspace_bytes(h, B, ld))
                    ws = _workspace(x.device, nws)
                check(lib.dissc_convgrad_backward(h, _ptr(x), _ptr(gy), _ptr(ctx.lengths), B, ld, ld, ld, ctx.in_slope,
                                                  _ptr(gx), _ptr(gw), _ptr(gb), _ptr(ws), nws, st), "dissc_convgrad_backward")
        return gx, gw, gb, (gy if need_add else None), None, None, None


def conv1d(x, weight, bias=None, lengths=None, dilation=1, in_slope=1.0, add=None):
    """y = bias + conv(lrelu(x, in_slope), weight, dilation, padding "same") (+ add).

    x [B, Cin, ld], add / y [B, Cout, ld]: contiguous fp32 device tensors, ld % 4 == 0.  weight: DEVICE tensor
    [Cout, Cin, k], k odd, k <= 11, (k - 1) * dilation <= 60; bias [Cout] or None.  lengths: int32 [B] on the device (or
    None = ld): positions at and beyond lengths[b] are read as zero and left zero in y.  Gradients flow to x, weight,
    bias and add (the gradient of add is the incoming gradient itself, handed through unmasked: the cotangent of a position
    beyond lengths[b], which the forward never writes, is the caller's to keep zero); x and weight are saved, y is not."""
    _check_act(x, "x")
    B, Cin, ld = x.shape
    if not (weight.is_cuda and weight.dtype == torch.float32 and weight.dim() == 3 and weight.is_contiguous()
            and weight.shape[1] == Cin):
        raise DisscError(f"nn.conv1d: weight must be a contiguous fp32 device tensor [Cout, {Cin}, k]")
    if bias is not None and not (bias.is_cuda and bias.dtype == torch.float32 and bias.is_contiguous()
                                 and tuple(bias.shape) == (weight.shape[0],)):
        raise DisscError("nn.conv1d: bias must be a contiguous fp32 device tensor [Cout]")
    if add is not None:
        _check_act(add, "add", B, ld)
        if add.shape[1] != weight.shape[0]:
            raise DisscError("nn.conv1d: add must have Cout channels")
    if lengths is not None and not (lengths.is_cuda and lengths.dtype == torch.int32 and lengths.is_contiguous()
                                    and tuple(lengths.shape) == (B,)):
        raise DisscError("nn.conv1d: lengths must be a contiguous int32 device tensor [B]")
    return _Conv1dFn.apply(x, weight, bias, add, lengths, int(dilation), float(in_slope))


class _ConvTranspose1dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, lengths, stride, in_slope):
        B, Cin, ld = x.shape
        _, Cout, k = weight.shape
        h = _handle_t(Cin, Cout, k, stride, x.device)
        st = current_stream_ptr(x.device)
        ldo = stride * ld
        with torch.cuda.device(x.device):
            check(lib.dissc_convtgrad_set_weights(h, _ptr(weight), _ptr(bias), st), "dissc_convtgrad_set_weights")
            y = torch.zeros((B, Cout, ldo), dtype=torch.float32, device=x.device) if lengths is not None else \
                torch.empty((B, Cout, ldo), dtype=torch.float32, device=x.device)
            check(lib.dissc_convtgrad_forward(h, _ptr(x), _ptr(y), _ptr(lengths), B, ld, ldo, ld, float(in_slope), st),
                  "dissc_convtgrad_forward")
        ctx.save_for_backward(x, weight)  # never y
        ctx.lengths, ctx.stride, ctx.in_slope, ctx.has_bias = lengths, int(stride), float(in_slope), bias is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        B, Cin, ld = x.shape
        _, Cout, k = weight.shape
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        gy = gy.contiguous()
        gx = gw = gb = ws = None
        if need_x or need_w or need_b:
            h = _handle_t(Cin, Cout, k, ctx.stride, x.device)
            st = current_stream_ptr(x.device)
            with torch.cuda.device(x.device):
                if need_x:  # another layer sharing the handle may have run since the forward: pack again (device only)
                    check(lib.dissc_convtgrad_set_weights(h, _ptr(weight), None, st), "dissc_convtgrad_set_weights")
                    gx = torch.empty_like(x)
                if need_w:
                    gw = torch.empty_like(weight)
                if need_b:
                    gb = torch.empty(Cout, dtype=torch.float32, device=x.device)
                nws = 0
                if need_w or need_b:
                    nws = int(lib.dissc_convtgrad_workspace_bytes(h, B, ld))
                    ws = _workspace(x.device, nws)
                check(lib.dissc_convtgrad_backward(h, _ptr(x), _ptr(gy), _ptr(ctx.lengths), B, ld, ctx.stride * ld, ld,
                                                   ctx.in_slope, _ptr(gx), _ptr(gw), _ptr(gb), _ptr(ws), nws, st),
                      "dissc_convtgrad_backward")
        return gx, gw, gb, None, None, None


def conv_transpose1d(x, weight, bias=None, stride=1, lengths=None, in_slope=1.0):
    """y = bias + ConvTranspose1d(lrelu(x, in_slope), weight, stride=stride, padding=(k - stride) // 2): the generator's
    upsamplers ups[i] (reference sr/models.py), which follow a leaky ReLU.

    x [B, Cin, ld]: contiguous fp32 device tensor, ld % 4 == 0; y [B, Cout, stride * ld].  weight: DEVICE tensor
    [Cin, Cout, k] (torch's ConvTranspose1d layout), 1 <= stride <= 8, stride <= k <= 11, k - stride even; bias [Cout] or None.
    lengths: int32 [B] on the device (or None = ld), INPUT lengths: utterance b has stride * lengths[b] valid output positions,
    y is left zero beyond them and the incoming gradient is read as zero there; the gradient of x is zero from lengths[b] on.
    Gradients flow to x, weight and bias; x and weight are saved, y is not."""
    who = "nn.conv_transpose1d"
    _check_act(x, "x", who=who)
    B, Cin, ld = x.shape
    if not (weight.is_cuda and weight.dtype == torch.float32 and weight.dim() == 3 and weight.is_contiguous()
            and weight.shape[0] == Cin):
        raise DisscError(f"{who}: weight must be a contiguous fp32 device tensor [{Cin}, Cout, k]")
    if bias is not None and not (bias.is_cuda and bias.dtype == torch.float32 and bias.is_contiguous()
                                 and tuple(bias.shape) == (weight.shape[1],)):
        raise DisscError(f"{who}: bias must be a contiguous fp32 device tensor [Cout]")
    if lengths is not None and not (lengths.is_cuda and lengths.dtype == torch.int32 and lengths.is_contiguous()
                                    and tuple(lengths.shape) == (B,)):
        raise DisscError(f"{who}: lengths must be a contiguous int32 device tensor [B]")
    return _ConvTranspose1dFn.apply(x, weight, bias, lengths, int(stride), float(in_slope))


def resblock1(x, weights, k, dilations=(1, 3, 5), lengths=None, taps=None):
    """ResBlock1 (reference sr/models.py:34-41): for each dilation d,  x = x + conv_1(lrelu(conv_d(lrelu(x)))), composed
    from six conv1d calls with the residual through ``add=``.  weights: {"convs1.<m>.weight" / ".bias",
    "convs2.<m>.weight" / ".bias"} (device tensors, weight norm already folded).  taps: a list that receives the input
    tensor of every conv1d call in order -- the engine's own pre-activations."""
    for m, d in enumerate(dilations):
        if taps is not None:
            taps.append(x)
        xt = conv1d(x, weights[f"convs1.{m}.weight"], weights.get(f"convs1.{m}.bias"), lengths=lengths, dilation=d,
                    in_slope=LRELU_SLOPE)
        if taps is not None:
            taps.append(xt)
        x = conv1d(xt, weights[f"convs2.{m}.weight"], weights.get(f"convs2.{m}.bias"), lengths=lengths, dilation=1,
                   in_slope=LRELU_SLOPE, add=x)
    return x
