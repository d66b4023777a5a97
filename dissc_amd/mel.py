"""Log-mel spectrograms and their L1 distance on the MI355X: the figure the reference's vocoder trainer logs as
``validation/mel_spec_error`` (reference sr/train.py:231-269 on mel_spectrogram, sr/dataset.py:46-69).

    ms = MelSpectrogram.from_config(h).to('cuda:0')
    ms.forward(wav, n_samples)["mel"]          # f32 [B, num_mels, F], log(max(mel, 1e-5))
    ms.l1(gt, y_hat, n_samples)["mean"]        # f64 [B]: mean |logmel(gt) - logmel(y_hat)| per utterance
    ms.l1_loss(gt, y_hat).backward()           # the generator's mel loss (reference sr/train.py:154-176, before the * 45)

Kernels: csrc/mel.hip (C ABI ``dissc_mel_*``): the STFT as a GEMM on the fp32 matrix cores with the frames read straight
from the staged samples, magnitudes and the mel GEMM in registers, and for ``l1`` a fused reduction that stores neither
mel.  csrc/mel_grad.hip: the gradient with respect to the samples (``dissc_mel_backward``, and ``dissc_mel_l1_grad``, which
gives the L1 sums and their gradient in one pass); a waveform that requires grad goes through it, so ``mel_spectrogram``
and ``forward`` return a mel with a ``grad_fn``.  Restated for the tests in tests/mel_ref.py.  No torch compute op on the
hot path, no CPU fallback.
"""
import ctypes

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import check, lib

TILE_FRAMES = 64  # DISSC_MEL_TILE_FRAMES: frames per workgroup of the kernel (the tests straddle it)
GRAD_TILE_FRAMES = 64  # DISSC_MEL_GRAD_TILE_FRAMES: the same for the gradient's kernel
_LINEAR = 1       # DISSC_MEL_LINEAR


def _bind():
    vp, i32, sz, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_double
    lib.dissc_mel_filterbank.argtypes = [i32, i32, i32, f64, f64, vp]
    lib.dissc_mel_create.argtypes = [i32, i32, i32, i32, i32, f64, f64, ctypes.POINTER(vp)]
    lib.dissc_mel_destroy.argtypes = [vp]
    lib.dissc_mel_destroy.restype = None
    lib.dissc_mel_frames.argtypes = [vp, i32]
    lib.dissc_mel_workspace_bytes.argtypes = [vp, i32, i32]
    lib.dissc_mel_workspace_bytes.restype = sz
    lib.dissc_mel_forward.argtypes = [vp, vp, i32, vp, i32, vp, i32, i32, vp, sz, vp]
    lib.dissc_mel_l1.argtypes = [vp, vp, i32, vp, i32, vp, i32, vp, vp, sz, vp]
    lib.dissc_mel_grad_workspace_bytes.argtypes = [vp, i32, i32]
    lib.dissc_mel_grad_workspace_bytes.restype = sz
    lib.dissc_mel_backward.argtypes = [vp, vp, i32, vp, i32, vp, i32, i32, vp, i32, vp, sz, vp]
    lib.dissc_mel_l1_grad.argtypes = [vp, vp, i32, vp, i32, vp, i32, vp, vp, vp, i32, vp, sz, vp]


_bind()


class _MelFn(torch.autograd.Function):
    """mel of a waveform that requires grad: forward is the plain kernel, backward is dissc_mel_backward (first order
    only: a backward through the backward raises)"""

    @staticmethod
    def forward(ctx, wav, ms, ns_dev, linear):
        ctx.ms, ctx.ns_dev, ctx.linear = ms, ns_dev, linear
        ctx.save_for_backward(wav)
        return ms._forward(wav, ns_dev, linear)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_mel):
        (wav,) = ctx.saved_tensors
        return ctx.ms._backward(wav, ctx.ns_dev, g_mel, ctx.linear), None, None, None


class _L1LossFn(torch.autograd.Function):
    """sum_b scale_b * sum |logmel(a_b) - logmel(y_b)|: value and gradient from one dissc_mel_l1_grad call"""

    @staticmethod
    def forward(ctx, y_hat, ms, target, ns_dev, scale):
        total, grad = ms._l1_grad(target, y_hat, ns_dev, scale)
        ctx.save_for_backward(grad)
        return (total * scale).sum().to(torch.float32)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g.to(torch.float32), None, None, None, None


def mel_filterbank(sampling_rate, n_fft, num_mels, fmin=0.0, fmax=None):
    """librosa.filters.mel with its defaults (Slaney scale and area normalisation), float64 [num_mels, n_fft // 2 + 1];
    computed on the host by the library, needs no GPU"""
    out = np.empty((int(num_mels), int(n_fft) // 2 + 1), dtype=np.float64)
    check(lib.dissc_mel_filterbank(int(sampling_rate), int(n_fft), int(num_mels), float(fmin),
                                   float(fmax) if fmax else 0.0, out.ctypes.data), "dissc_mel_filterbank")
    return out


class MelSpectrogram:
    """mel_spectrogram(center=False) of the reference for a batch of ragged utterances.  The handle is created on first use
    (host only); the packed bases go to ``device`` with the first launch."""

    def __init__(self, sampling_rate=16000, n_fft=1024, num_mels=80, hop_size=256, win_size=1024, fmin=0.0, fmax=None):
        self.sampling_rate, self.n_fft, self.num_mels = int(sampling_rate), int(n_fft), int(num_mels)
        self.hop_size, self.win_size = int(hop_size), int(win_size)
        self.fmin, self.fmax = float(fmin), (float(fmax) if fmax else None)
        self.pad = (self.n_fft - self.hop_size) // 2
        self.device = None
        self._h = None
        self._ws = None
        self._gws = None

    @classmethod
    def from_config(cls, h, for_loss=True):
        """from a vocoder config: ``fmax_for_loss`` (what the trainer's validation uses) or ``fmax``"""
        get = h.get if hasattr(h, "get") else lambda k, d=None: getattr(h, k, d)
        return cls(get("sampling_rate"), get("n_fft"), get("num_mels"), get("hop_size"), get("win_size"), get("fmin"),
                   get("fmax_for_loss", None) if for_loss else get("fmax", None))

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.DisscError("dissc_amd.mel.MelSpectrogram runs on an MI355X only")
        if self.device is not None and device != self.device:
            self.close()
        self.device = device
        return self

    def close(self):
        if self._h is not None:
            lib.dissc_mel_destroy(self._h)
        self._h, self._ws, self._gws = None, None, None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def handle(self):
        if self._h is None:
            h = ctypes.c_void_p()
            check(lib.dissc_mel_create(self.sampling_rate, self.n_fft, self.num_mels, self.hop_size, self.win_size,
                                       self.fmin, self.fmax or 0.0, ctypes.byref(h)), "dissc_mel_create")
            self._h = h
        return self._h

    def frames(self, n_samples):
        return int(lib.dissc_mel_frames(self.handle(), int(n_samples)))

    def _workspace(self, B, N):
        need = lib.dissc_mel_workspace_bytes(self._h, B, N)
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
        return self._ws, need

    def _signal(self, wav, what):
        if self.device is None:
            raise _lib.DisscError("MelSpectrogram: call .to('cuda:N') first (no CPU fallback)")
        wav = torch.as_tensor(wav)
        if wav.dim() == 1:
            wav = wav[None]
        if wav.dim() == 3 and wav.shape[1] == 1:
            wav = wav[:, 0]
        if wav.dim() != 2:
            raise ValueError(f"{what}: expected [B, N] (or [N], [B, 1, N]), got {tuple(wav.shape)}")
        return wav.to(self.device, torch.float32).contiguous()

    def _lengths(self, n_samples, B, N):
        ns = np.full(B, N, dtype=np.int64) if n_samples is None else \
            np.asarray(n_samples.cpu() if isinstance(n_samples, torch.Tensor) else n_samples, dtype=np.int64).reshape(-1)
        if ns.shape[0] != B or (ns > N).any():
            raise ValueError(f"n_samples: need {B} counts of at most {N}")
        if (ns <= self.pad).any():  # torch's reflection pad raises as well
            raise _lib.DisscError(f"MelSpectrogram: an utterance of {int(ns.min())} samples cannot be mirrored by "
                                  f"(n_fft - hop) / 2 = {self.pad}; need more than that")
        return ns, torch.from_numpy(ns.astype(np.int32)).to(self.device)

    def _grad_workspace(self, B, N):
        need = lib.dissc_mel_grad_workspace_bytes(self._h, B, N)
        if self._gws is None or self._gws.numel() < need:
            self._gws = None
            self._gws = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
        return self._gws, need

    def _forward(self, wav, ns_dev, linear):
        B, N = wav.shape
        ldF = max(N // self.hop_size, 1)
        mel = torch.zeros(B, self.num_mels, ldF, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(lib.dissc_mel_forward(self.handle(), wav.data_ptr(), N, ns_dev.data_ptr(), B, mel.data_ptr(), ldF,
                                        _LINEAR if linear else 0, None, 0, _lib.current_stream_ptr(self.device)),
                  "dissc_mel_forward")
        return mel

    def _backward(self, wav, ns_dev, g_mel, linear):
        h = self.handle()
        B, N = wav.shape
        ldF = max(N // self.hop_size, 1)
        if tuple(g_mel.shape) != (B, self.num_mels, ldF):
            raise ValueError(f"g_mel: expected {(B, self.num_mels, ldF)}, got {tuple(g_mel.shape)}")
        g_mel = g_mel.to(self.device, torch.float32).contiguous()
        grad = torch.empty(B, N, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            ws, need = self._grad_workspace(B, N)
            check(lib.dissc_mel_backward(h, wav.data_ptr(), N, ns_dev.data_ptr(), B, g_mel.data_ptr(), ldF,
                                         _LINEAR if linear else 0, grad.data_ptr(), N, ws.data_ptr(), need,
                                         _lib.current_stream_ptr(self.device)), "dissc_mel_backward")
        return grad

    def _l1_grad(self, a, b, ns_dev, scale):
        h = self.handle()
        B = a.shape[0]
        total = torch.empty(B, dtype=torch.float64, device=self.device)
        grad = torch.empty_like(b)
        with torch.cuda.device(self.device):
            ws, need = self._grad_workspace(B, min(a.shape[1], b.shape[1]))
            check(lib.dissc_mel_l1_grad(h, a.data_ptr(), a.shape[1], b.data_ptr(), b.shape[1], ns_dev.data_ptr(), B,
                                        scale.data_ptr(), total.data_ptr(), grad.data_ptr(), b.shape[1], ws.data_ptr(), need,
                                        _lib.current_stream_ptr(self.device)), "dissc_mel_l1_grad")
        return total, grad

    def forward(self, wav, n_samples=None, linear=False):
        """wav f32 [B, N] (device or host), n_samples [B] (default: N) -> {"mel": f32 [B, num_mels, max frames] on the
        device, zero beyond an utterance's frames; "frames": int64 [B] (host)}; linear=True: the mel before the log.
        A wav that requires grad gives a mel with a grad_fn (backward: dissc_mel_backward; cotangent columns beyond an
        utterance's frames are ignored); any other input takes the plain path."""
        self.handle()
        tracked = torch.is_grad_enabled() and isinstance(wav, torch.Tensor) and wav.requires_grad
        wav = self._signal(wav, "wav")
        B, N = wav.shape
        ns, ns_dev = self._lengths(n_samples, B, N)
        frames = ns // self.hop_size
        mel = _MelFn.apply(wav, self, ns_dev, bool(linear)) if tracked else self._forward(wav, ns_dev, linear)
        return {"mel": mel[:, :, :max(int(frames.max()), 1)], "frames": torch.from_numpy(frames)}

    def backward(self, wav, g_mel, n_samples=None, linear=False):
        """the vector-Jacobian product of forward: g_mel f32 [B, num_mels, >= max frames] -> f32 [B, N] on the device,
        zero at and beyond an utterance's n_samples.  Bit-reproducible, independent of the rest of the batch."""
        self.handle()
        wav = self._signal(wav, "wav").detach()
        B, N = wav.shape
        _, ns_dev = self._lengths(n_samples, B, N)
        g_mel = torch.as_tensor(g_mel).to(self.device, torch.float32)
        ldF = max(N // self.hop_size, 1)
        if g_mel.dim() == 3 and g_mel.shape[2] != ldF:  # any width that holds the frames
            full = torch.zeros(B, self.num_mels, ldF, dtype=torch.float32, device=self.device)
            k = min(ldF, g_mel.shape[2])
            full[:, :, :k] = g_mel[:, :, :k]
            g_mel = full
        return self._backward(wav, ns_dev, g_mel, linear)

    __call__ = forward

    def l1(self, a, b, n_samples=None):
        """a, b f32 [B, Na], [B, Nb]; n_samples [B] counts for both (default: the shorter row) -> {"sum": f64 [B] of
        |logmel(a) - logmel(b)| over the utterance's cells, "cells": int64 [B] = frames * num_mels, "mean": sum / cells},
        all on the device.  Bit-reproducible; an utterance's figures do not depend on the rest of the batch."""
        h = self.handle()
        a, b = self._signal(a, "a"), self._signal(b, "b")
        if a.shape[0] != b.shape[0]:
            raise ValueError(f"l1: {a.shape[0]} and {b.shape[0]} utterances")
        B, N = a.shape[0], min(a.shape[1], b.shape[1])
        ns, ns_dev = self._lengths(n_samples, B, N)
        cells = torch.from_numpy((ns // self.hop_size) * self.num_mels).to(self.device)
        total = torch.empty(B, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            ws, need = self._workspace(B, N)
            check(lib.dissc_mel_l1(h, a.data_ptr(), a.shape[1], b.data_ptr(), b.shape[1], ns_dev.data_ptr(), B,
                                   total.data_ptr(), ws.data_ptr(), need, _lib.current_stream_ptr(self.device)),
                  "dissc_mel_l1")
        return {"sum": total, "cells": cells, "mean": total / cells}

    def l1_grad(self, a, b, n_samples=None, scale=None):
        """l1 and its gradient in one pass: {"sum", "cells", "mean"} as l1 gives them (the same bits), and "grad" f32
        [B, Nb] = scale_b * d sum_b / d b (scale f64 [B], default 1), zero beyond an utterance's samples"""
        self.handle()
        a, b = self._signal(a, "a").detach(), self._signal(b, "b").detach()
        if a.shape[0] != b.shape[0]:
            raise ValueError(f"l1_grad: {a.shape[0]} and {b.shape[0]} utterances")
        B, N = a.shape[0], min(a.shape[1], b.shape[1])
        ns, ns_dev = self._lengths(n_samples, B, N)
        scale = torch.ones(B, dtype=torch.float64) if scale is None else torch.as_tensor(scale, dtype=torch.float64).reshape(-1)
        if scale.shape[0] != B:
            raise ValueError(f"scale: need {B} factors")
        cells = torch.from_numpy((ns // self.hop_size) * self.num_mels).to(self.device)
        total, grad = self._l1_grad(a, b, ns_dev, scale.to(self.device).contiguous())
        return {"sum": total, "cells": cells, "mean": total / cells, "grad": grad}

    def l1_loss(self, target, y_hat, n_samples=None, reduction="mean"):
        """the mel loss of the reference's generator step as a scalar with a grad_fn: |logmel(target) - logmel(y_hat)|
        reduced by "mean" (all sums / all cells: F.l1_loss of the two mels for equal lengths), "utterance_mean" (the mean
        of the utterances' means, validate.py's figure) or "sum".  One dissc_mel_l1_grad call; neither mel is stored.
        The gradient goes to y_hat alone: a target that requires grad raises."""
        self.handle()
        if isinstance(target, torch.Tensor) and target.requires_grad:
            raise ValueError("l1_loss: the target gets no gradient; detach it")
        a, b = self._signal(target, "target"), self._signal(y_hat, "y_hat")
        if a.shape[0] != b.shape[0]:
            raise ValueError(f"l1_loss: {a.shape[0]} and {b.shape[0]} utterances")
        B, N = a.shape[0], min(a.shape[1], b.shape[1])
        ns, ns_dev = self._lengths(n_samples, B, N)
        cells = ((ns // self.hop_size) * self.num_mels).astype(np.float64)
        if reduction == "mean":
            scale = np.full(B, 1.0 / cells.sum())
        elif reduction == "utterance_mean":
            scale = 1.0 / (B * cells)
        elif reduction == "sum":
            scale = np.ones(B)
        else:
            raise ValueError(f"l1_loss: reduction {reduction!r} (mean, utterance_mean or sum)")
        return _L1LossFn.apply(b, self, a, ns_dev, torch.from_numpy(scale).to(self.device))


_cache = {}


def mel_spectrogram(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False):
    """the reference's signature (sr/dataset.py:46): y f32 [B, N] on an MI355X -> log-mel f32 [B, num_mels, N // hop_size],
    with a grad_fn when y requires grad (F.l1_loss on top of it trains as in the reference).
    One handle per parameter set and device (the reference keys its cache by fmax alone; that quirk is not reproduced)."""
    if center:
        raise NotImplementedError("mel_spectrogram: center=True is not implemented (the reference never uses it)")
    y = torch.as_tensor(y)
    if not y.is_cuda:
        raise _lib.DisscError("dissc_amd.mel.mel_spectrogram runs on an MI355X only")
    key = (int(n_fft), int(num_mels), int(sampling_rate), int(hop_size), int(win_size), float(fmin),
           float(fmax) if fmax else None, str(y.device))
    if key not in _cache:
        _cache[key] = MelSpectrogram(sampling_rate, n_fft, num_mels, hop_size, win_size, fmin, fmax).to(y.device)
    return _cache[key].forward(y)["mel"]
