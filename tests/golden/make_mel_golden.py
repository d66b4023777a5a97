"""Writes tests/golden/mel_basis.npz: the mel filterbank of a THIRD party (transformers.audio_utils.mel_filter_bank with
norm="slaney", mel_scale="slaney", transposed to librosa's [num_mels, bins]) for the two parameter sets the mel tests use.
Both dissc_mel_filterbank and tests/mel_ref.py are pinned to it, so neither is pinned to ourselves.

    python tests/golden/make_mel_golden.py
"""
import os

import numpy as np
from transformers.audio_utils import mel_filter_bank

# (sampling rate, n_fft, num_mels, fmin, fmax)
SETS = {"shipped": (16000, 1024, 80, 0.0, 8000.0), "narrow": (16000, 512, 40, 50.0, 7600.0)}


def main():
    out = {}
    for name, (sr, n_fft, num_mels, fmin, fmax) in SETS.items():
        fb = mel_filter_bank(n_fft // 2 + 1, num_mels, fmin, fmax, sr, norm="slaney", mel_scale="slaney").T
        out[name] = np.ascontiguousarray(fb, dtype=np.float64)
        out[name + "_params"] = np.array([sr, n_fft, num_mels, fmin, fmax], dtype=np.float64)
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "mel_basis.npz"), **out)


if __name__ == "__main__":
    main()
