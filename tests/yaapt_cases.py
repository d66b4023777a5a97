"""Shared by the F0 tests (tests/test_yaapt.py, test_gpu_yaapt.py, test_gpu_prosody_metrics.py; not a test module): signals with a
known F0, the check of a track against it, the reference speech fixtures and what any tracker must deliver on them."""
import os

import numpy as np

FS = 16000


def voiced(f0):
    """speech-like test signal: harmonics up to 3.5 kHz under a two-formant envelope, instantaneous F0 `f0`"""
    f0 = np.asarray(f0, dtype=np.float64)
    ph = 2 * np.pi * np.cumsum(f0) / FS
    x = np.zeros(len(f0))
    for k in range(1, 60):
        fk = k * f0
        env = 1.0 / (1 + ((fk - 500) / 400) ** 2) + 0.5 / (1 + ((fk - 1500) / 500) ** 2) + 0.05
        x += np.where(fk < 3500, env * np.sin(k * ph + 0.3 * k), 0)
    return 0.1 * x


def pulse_train(f0, n):
    """band-limited pulse train: all harmonics below 3.5 kHz at equal amplitude (a flat-spectrum 'buzz').
    (A 1/k sawtooth is NOT a fair target: squaring it leaves so little energy above the 2nd harmonic that the
    harmonic-product stage of YAAPT, built for speech spectra, locks an octave low -- observed with this
    restatement and recorded here as a known limitation.)"""
    t = np.arange(n) / FS
    return 0.02 * sum(np.cos(2 * np.pi * k * f0 * t) for k in range(1, int(3500 / f0)))


CASES = {"flat85": np.full(24000, 85.0), "flat120": np.full(24000, 120.0), "flat200": np.full(24000, 200.0),
         "flat330": np.full(24000, 330.0), "glide100-250": np.linspace(100, 250, 24000),
         "vibrato": 180 + 15 * np.sin(2 * np.pi * 5 * np.arange(24000) / FS)}


def check_track(f0, want_per_sample, p95=0.02, voiced_min=0.97):
    n = len(want_per_sample)
    want = want_per_sample[np.minimum(np.arange(len(f0)) * 80, n - 1)]
    core = slice(10, len(f0) - 10)  # the first / last 50 ms see the zero padding
    v = f0[core] > 0
    assert v.mean() >= voiced_min, v.mean()
    rel = np.abs(f0[core][v] - want[core][v]) / want[core][v]
    assert np.percentile(rel, 95) <= p95, (np.median(rel), np.percentile(rel, 95))
    return rel


def _speech(name):
    from scipy.io import wavfile
    sr, x = wavfile.read(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".wav"))
    assert sr == FS
    return x.astype(np.float32) / 32768.0


def speech_track_is_plausible(f0, what):
    """what any F0 tracker must deliver on a clean, mostly voiced read sentence of one speaker"""
    v = f0 > 0
    assert 0.5 <= v.mean() <= 0.95, (what, v.mean())
    assert f0[v].min() >= 60.0 and f0[v].max() <= 400.0, (what, f0[v].min(), f0[v].max())
    both = v[1:] & v[:-1]
    jumps = np.abs(np.diff(f0))[both] / f0[:-1][both]
    assert np.median(jumps) < 0.10, (what, np.median(jumps))          # the verdict's bar
    assert np.median(jumps) < 0.03 and (jumps < 0.25).mean() >= 0.9, (what, np.median(jumps))  # what is measured
    # one speaker: the bulk of the voiced frames lies within an octave around the median
    med = np.median(f0[v])
    assert ((f0[v] > med / 1.6) & (f0[v] < med * 1.6)).mean() >= 0.93, what
