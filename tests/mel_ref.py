"""CPU restatement of the reference's mel_spectrogram (sr/dataset.py:46-69, center=False) for the tests of dissc_amd.mel.

The reference module itself cannot be imported here: it needs librosa, which is not installed.  So the filterbank
librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax) builds with its defaults (Slaney scale, Slaney area normalisation) is
restated below from its published formula and pinned to a third party's implementation in tests/golden/mel_basis.npz
(tests/golden/make_mel_golden.py); everything after it is the reference's own arithmetic on torch.stft: reflection pad by
(n_fft - hop) / 2, torch.hann_window(win), magnitude sqrt(re^2 + im^2 + 1e-9), basis.float() @ magnitude,
log(clamp(min=1e-5)).  dtype=torch.float64 gives the oracle, dtype=torch.float32 the reference's own precision.
"""
import numpy as np
import torch

F_SP = 200.0 / 3.0
MIN_LOG_HZ = 1000.0
LOGSTEP = np.log(6.4) / 27.0
CLIP = 1e-5


def hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= MIN_LOG_HZ, MIN_LOG_HZ / F_SP + np.log(np.maximum(f, 1e-300) / MIN_LOG_HZ) / LOGSTEP, f / F_SP)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= MIN_LOG_HZ / F_SP, MIN_LOG_HZ * np.exp(LOGSTEP * (m - MIN_LOG_HZ / F_SP)), F_SP * m)


def mel_filterbank(sr, n_fft, num_mels, fmin=0.0, fmax=None):
    """float64 [num_mels, n_fft // 2 + 1]"""
    fmax = sr / 2.0 if not fmax else float(fmax)
    freqs = np.arange(n_fft // 2 + 1, dtype=np.float64) * sr / n_fft
    edges = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), num_mels + 2))
    fdiff = np.diff(edges)
    ramps = edges[:, None] - freqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper))
    return w * (2.0 / (edges[2:] - edges[:-2]))[:, None]


def frames(n_samples, hop):
    """frames torch.stft(center=False) gives on the padded signal: 1 + (n + n_fft - hop - n_fft) // hop"""
    return n_samples // hop if n_samples >= hop else 0


def mel(y, n_fft=1024, num_mels=80, sr=16000, hop=256, win=1024, fmin=0.0, fmax=None, dtype=torch.float64, log=True):
    """y [N] or [B, N] (float32 values) -> [B, num_mels, N // hop] in `dtype`, linear (log=False) or log"""
    y = torch.as_tensor(np.asarray(y)).to(dtype)
    if y.dim() == 1:
        y = y[None]
    basis = torch.from_numpy(mel_filterbank(sr, n_fft, num_mels, fmin, fmax)).float().to(dtype)  # .float(): as the reference
    window = torch.hann_window(win, dtype=dtype)
    p = (n_fft - hop) // 2
    y = torch.nn.functional.pad(y[:, None], (p, p), mode="reflect")[:, 0]
    spec = torch.view_as_real(torch.stft(y, n_fft, hop_length=hop, win_length=win, window=window, center=False,
                                         normalized=False, onesided=True, return_complex=True))
    mag = torch.sqrt(spec.pow(2).sum(-1) + 1e-9)
    out = torch.matmul(basis, mag)
    return torch.log(torch.clamp(out, min=CLIP)) if log else out
