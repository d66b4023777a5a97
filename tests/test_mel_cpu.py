"""Host side of dissc_amd.mel without a GPU: the filterbank, the frame counts and the argument checks of the C ABI
(dissc_mel_filterbank and dissc_mel_create compute on the host and launch nothing), and tests/mel_ref.py itself.

Filterbank bar: both sides are a handful of double operations per weight (two subtractions, a division, a product), so
they must agree with the third party's table in tests/golden/mel_basis.npz to 1e-12 of the largest weight.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import mel_ref


@pytest.fixture(scope="module")
def melmod():
    from dissc_amd import mel
    return mel


@pytest.fixture(scope="module")
def basis(golden_dir):
    return np.load(os.path.join(golden_dir, "mel_basis.npz"))


SETS = ("shipped", "narrow")


@pytest.mark.parametrize("name", SETS)
def test_filterbanks_equal_the_third_party_table(melmod, basis, name):
    want = basis[name]
    sr, n_fft, num_mels, fmin, fmax = basis[name + "_params"]
    sr, n_fft, num_mels = int(sr), int(n_fft), int(num_mels)
    assert want.shape == (num_mels, n_fft // 2 + 1)
    tol = 1e-12 * want.max()
    for got in (melmod.mel_filterbank(sr, n_fft, num_mels, fmin, fmax), mel_ref.mel_filterbank(sr, n_fft, num_mels, fmin, fmax)):
        assert got.shape == want.shape and np.abs(got - want).max() <= tol
    used = np.nonzero(want.any(axis=0))[0]
    # the DFT bins the kernel skips: exactly DC and Nyquist for the shipped set, bins 4 .. 486 at n_fft 1024 scale for the other
    assert (used.min(), used.max()) == ((1, 511) if name == "shipped" else (2, 243))
    if name == "shipped":  # fmax None means sr / 2
        assert np.array_equal(melmod.mel_filterbank(sr, n_fft, num_mels, fmin, None), melmod.mel_filterbank(sr, n_fft, num_mels, fmin, fmax))


@pytest.mark.parametrize("name", SETS)
def test_filterbanks_equal_transformers_directly(melmod, basis, name):
    audio_utils = pytest.importorskip("transformers.audio_utils")
    sr, n_fft, num_mels, fmin, fmax = basis[name + "_params"]
    sr, n_fft, num_mels = int(sr), int(n_fft), int(num_mels)
    want = audio_utils.mel_filter_bank(n_fft // 2 + 1, num_mels, fmin, fmax, sr, norm="slaney", mel_scale="slaney").T
    assert np.array_equal(want, basis[name])  # the committed table is what make_mel_golden.py writes
    assert np.abs(melmod.mel_filterbank(sr, n_fft, num_mels, fmin, fmax) - want).max() <= 1e-12 * want.max()


def test_frame_counts(melmod):
    ms = melmod.MelSpectrogram()  # 1024 / 256: no GPU is touched by creating the handle
    for n in (255, 256, 385, 1023, 1024, 10560):
        assert ms.frames(n) == mel_ref.frames(n, 256) == n // 256
        if n > 384:  # torch can mirror: the restatement's own frame count
            assert mel_ref.mel(np.zeros(n, np.float32)).shape == (1, 80, n // 256)
    assert melmod.TILE_FRAMES == 64


def test_bad_arguments_are_refused_without_a_gpu(melmod):
    L = melmod.lib
    h = ctypes.c_void_p()
    ok = dict(sr=16000, n_fft=1024, num_mels=80, hop=256, win=1024, fmin=0.0, fmax=0.0)

    def create(**kw):
        a = dict(ok, **kw)
        return L.dissc_mel_create(a["sr"], a["n_fft"], a["num_mels"], a["hop"], a["win"], a["fmin"], a["fmax"], ctypes.byref(h))

    assert create() == 0 and h.value
    L.dissc_mel_destroy(h)
    for bad in (dict(n_fft=1000), dict(n_fft=4096), dict(win=1025), dict(hop=1028), dict(hop=255), dict(hop=2),
                dict(num_mels=129), dict(num_mels=0), dict(fmin=9000.0), dict(fmax=9000.0), dict(sr=0),
                dict(n_fft=2048, win=2048, hop=2048)):  # the last: a 64-frame tile does not fit the LDS
        assert create(**bad) == -1 and h.value is None, bad
        assert b"dissc_mel_create" in L.dissc_last_error()
    assert L.dissc_mel_create(16000, 1024, 80, 256, 1024, 0.0, 0.0, None) == -1
    assert L.dissc_mel_filterbank(16000, 1024, 80, 0.0, 0.0, None) == -1
    assert L.dissc_mel_forward(None, None, 0, None, 0, None, 0, 0, None, 0, None) == -1
    assert L.dissc_mel_l1(None, None, 0, None, 0, None, 0, None, None, 0, None) == -1
    with pytest.raises(melmod._lib.DisscError):
        melmod.MelSpectrogram().to("cpu")
    with pytest.raises(melmod._lib.DisscError):
        melmod.MelSpectrogram().forward(np.zeros((1, 4000), np.float32))  # no device chosen: no CPU fallback
    with pytest.raises(NotImplementedError):
        melmod.mel_spectrogram(torch.zeros(1, 4000), 1024, 80, 16000, 256, 1024, 0, 8000, center=True)
    import dissc_amd
    assert dissc_amd.MelSpectrogram is melmod.MelSpectrogram and dissc_amd.mel_spectrogram is melmod.mel_spectrogram


def test_from_config_takes_the_loss_fmax(melmod):
    import synthdata as synth
    cfg = dict(synth.VCTK_CONFIG, n_fft=1024, num_mels=80, hop_size=256, win_size=1024, fmin=0, fmax=8000, fmax_for_loss=None,
               sampling_rate=16000)
    ms = melmod.MelSpectrogram.from_config(cfg)
    assert (ms.n_fft, ms.num_mels, ms.hop_size, ms.win_size, ms.fmax, ms.pad) == (1024, 80, 256, 1024, None, 384)
    assert melmod.MelSpectrogram.from_config(cfg, for_loss=False).fmax == 8000.0


def test_reference_restatement_is_self_consistent():
    """mel_ref's float32 path is the float64 path rounded: a few 1e-7 of a frame's largest cell"""
    rs = np.random.RandomState(0)
    x = (0.3 * rs.standard_normal(5000)).astype(np.float32)
    a, b = mel_ref.mel(x, dtype=torch.float64, log=False)[0].numpy(), mel_ref.mel(x, dtype=torch.float32, log=False)[0].numpy()
    assert a.shape == (80, 19) and (np.abs(a - b).max(axis=0) / a.max(axis=0)).max() < 2e-6
    # a frame equals the direct definition: mirrored signal, periodic Hann, DFT magnitude
    p = np.pad(x.astype(np.float64), (384, 384), mode="reflect")
    fr = p[3 * 256:3 * 256 + 1024] * (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(1024) / 1024))
    mag = np.sqrt(np.abs(np.fft.rfft(fr)) ** 2 + 1e-9)
    want = mel_ref.mel_filterbank(16000, 1024, 80).astype(np.float32).astype(np.float64) @ mag
    assert np.abs(a[:, 3] - want).max() <= 1e-12 * want.max()
