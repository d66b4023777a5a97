"""mel_ref.mel on a TENSOR, so that torch's autograd runs through it: the oracle (float64) and the yardstick (float32, the
reference's precision) of the mel gradient's tests.  The same operations in the same order as mel_ref.mel, which takes
numpy input only; tests/test_mel_grad_cpu.py holds the two to equal bits.

Also the CPU model the bar's FACTOR was checked with: the kernel's arithmetic as an fp32 matmul DFT (model_vjp), and

    python tests/mel_grad_ref.py

re-reads its ratios (model's worst e over the float32 autograd's worst e, per parameter set, kind and mode, on the noisy
copies and full length lists of tests/test_gpu_mel_grad.py); the figures of record are in profiles/mel.md."""
import numpy as np
import torch

import mel_ref
from mel_cases import FACTOR, ref_kwargs


def mel_t(y, n_fft=1024, num_mels=80, sr=16000, hop=256, win=1024, fmin=0.0, fmax=None, log=True):
    """y tensor [N] or [B, N] of the dtype to compute in -> [B, num_mels, N // hop]"""
    if y.dim() == 1:
        y = y[None]
    basis = torch.from_numpy(mel_ref.mel_filterbank(sr, n_fft, num_mels, fmin, fmax)).float().to(y.dtype)
    window = torch.hann_window(win, dtype=y.dtype)
    p = (n_fft - hop) // 2
    y = torch.nn.functional.pad(y[:, None], (p, p), mode="reflect")[:, 0]
    spec = torch.view_as_real(torch.stft(y, n_fft, hop_length=hop, win_length=win, window=window, center=False,
                                         normalized=False, onesided=True, return_complex=True))
    out = torch.matmul(basis, torch.sqrt(spec.pow(2).sum(-1) + 1e-9))
    return torch.log(torch.clamp(out, min=mel_ref.CLIP)) if log else out


def vjp(w, cot, kw, dtype, log):
    """gradient of sum(cot * mel(w)) with respect to the samples: w float32 [N], cot [num_mels, F] -> float64 numpy [N]"""
    y = torch.from_numpy(np.asarray(w, np.float32)).to(dtype).requires_grad_(True)
    m = mel_t(y, log=log, **kw)[0]
    (m * torch.from_numpy(np.asarray(cot)).to(dtype)).sum().backward()
    return y.grad.double().numpy()


def model_vjp(w, cot, P, log):
    """the same gradient by the kernel's arithmetic in float32: windowed cosine / sine rows rounded once from float64,
    re / im as matmuls over the unfolded mirrored frames, torch's float32 autograd through it; P as in test_gpu_mel.py"""
    n_fft, hop, win = P["n_fft"], P["hop_size"], P["win_size"]
    pad, w_lo = (n_fft - hop) // 2, (n_fft - win) // 2
    fb = torch.from_numpy(mel_ref.mel_filterbank(P["sampling_rate"], n_fft, P["num_mels"], P["fmin"], P["fmax"])).float()
    wnd = np.zeros(n_fft)
    wnd[w_lo:w_lo + win] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win) / win)
    ph = 2 * np.pi * ((np.arange(n_fft // 2 + 1)[:, None] * np.arange(n_fft)[None, :]) % n_fft) / n_fft
    C, S = torch.from_numpy((wnd * np.cos(ph)).astype(np.float32)), torch.from_numpy((wnd * np.sin(ph)).astype(np.float32))
    y = torch.from_numpy(np.asarray(w, np.float32)).requires_grad_(True)
    frames = torch.nn.functional.pad(y[None, None], (pad, pad), mode="reflect")[0, 0].unfold(0, n_fft, hop).T
    re, im = C @ frames, S @ frames
    m = fb @ torch.sqrt(re * re + im * im + 1e-9)
    if log:
        m = torch.log(torch.clamp(m, min=mel_ref.CLIP))
    (m * torch.from_numpy(np.asarray(cot, np.float32))).sum().backward()
    return y.grad.double().numpy()


def noisy_of(waves):
    rs = np.random.RandomState(7)
    return [np.clip(w + 0.01 * rs.standard_normal(len(w)), -1, 1).astype(np.float32) for w in waves]


class GradRef:
    """float64 gradients of a set of signals for fixed cotangents, the float32 path's error on them, the bar"""

    def __init__(self, waves, P, log, cots=None, seed=11):
        kw, rs = ref_kwargs(P), np.random.RandomState(seed)
        self.waves, self.P, self.log = waves, P, log
        self.cots = cots or [rs.standard_normal((P["num_mels"], len(w) // P["hop_size"])).astype(np.float32) for w in waves]
        self.g64 = [vjp(w, c, kw, torch.float64, log) for w, c in zip(waves, self.cots)]
        g32 = [vjp(w, c, kw, torch.float32, log) for w, c in zip(waves, self.cots)]
        self.e32 = max(self.err(i, g) for i, g in enumerate(g32))
        self.bar = FACTOR * self.e32

    def err(self, i, g):
        return float(np.abs(np.asarray(g, np.float64) - self.g64[i]).max() / np.abs(self.g64[i]).max())


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import mel_cases as fwd
    for name, P, kinds in (("shipped", fwd.SHIPPED, fwd.KINDS), ("narrow", fwd.NARROW, ("iid", "speech_like")),
                           ("hop250", fwd.ODD_HOP, ("speech_like",))):
        for kind in kinds:
            for log in (False, True):
                ref = GradRef(noisy_of(fwd.ref_of(kind, P).waves), P, log)
                e = max(ref.err(i, model_vjp(w, c, P, log)) for i, (w, c) in enumerate(zip(ref.waves, ref.cots)))
                print(f"{name} {kind} {'log' if log else 'linear'}: e_torch32(set) {ref.e32:.2e} model {e:.2e} ratio {e / ref.e32:.2f}")
