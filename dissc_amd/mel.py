"""Log-mel spectrograms and their L1 distance on the MI355X: the figure the reference's vocoder trainer logs as
``validation/mel_spec_error`` (reference sr/train.py:231-269 on mel_spectrogram, sr/dataset.py:46-69).

    ms = MelSpectrogram.from_config(h).to('cuda:0')
    ms.forward(wav, n_samples)["mel"]          # f32 [B, num_mels, F], log(max(mel, 1e-5))
    ms.l1(gt, y_hat, n_samples)["mean"]        # f64 [B]: mean |logmel(gt) - logmel(y_hat)| per utterance

Kernels: csrc/mel.hip (C ABI ``dissc_mel_*``): the STFT as a GEMM on the fp32 matrix cores with the frames read straight
from the staged samples, magnitudes and the mel GEMM in registers, and for ``l1`` a fused reduction that stores neither
mel.  Restated for the tests in tests/mel_ref.py.  No torch compute op, no CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, lib

TILE_FRAMES = 64  # DISSC_MEL_TILE_FRAMES: frames per workgroup of the kernel (the tests straddle it)
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


_bind()


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
        self._h, self._ws = None, None

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

    def forward(self, wav, n_samples=None, linear=False):
        """wav f32 [B, N] (device or host), n_samples [B] (default: N) -> {"mel": f32 [B, num_mels, max frames] on the
        device, zero beyond an utterance's frames; "frames": int64 [B] (host)}; linear=True: the mel before the log"""
        h = self.handle()
        wav = self._signal(wav, "wav")
        B, N = wav.shape
        ns, ns_dev = self._lengths(n_samples, B, N)
        frames = ns // self.hop_size
        ldF = max(N // self.hop_size, 1)
        mel = torch.zeros(B, self.num_mels, ldF, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(lib.dissc_mel_forward(h, wav.data_ptr(), N, ns_dev.data_ptr(), B, mel.data_ptr(), ldF,
                                        _LINEAR if linear else 0, None, 0, _lib.current_stream_ptr(self.device)),
                  "dissc_mel_forward")
        return {"mel": mel[:, :, :max(int(frames.max()), 1)], "frames": torch.from_numpy(frames)}

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


_cache = {}


def mel_spectrogram(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False):
    """the reference's signature (sr/dataset.py:46): y f32 [B, N] on an MI355X -> log-mel f32 [B, num_mels, N // hop_size].
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
