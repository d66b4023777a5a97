"""The signals, parameter sets and float64 yardstick that the mel tests share (tests/test_gpu_mel.py, test_gpu_mel_grad.py,
test_validate_cli.py, and tests/mel_grad_ref.py run as a script): why FACTOR is 8 and how the lengths are chosen is told in
tests/test_gpu_mel.py."""
import numpy as np
import torch

import mel_ref

KINDS = ("iid", "speech_like", "speech_dc", "dither")
SHIPPED = dict(sampling_rate=16000, n_fft=1024, num_mels=80, hop_size=256, win_size=1024, fmin=0.0, fmax=None)
NARROW = dict(sampling_rate=16000, n_fft=512, num_mels=40, hop_size=128, win_size=400, fmin=50.0, fmax=7600.0)
ODD_HOP = dict(sampling_rate=16000, n_fft=512, num_mels=40, hop_size=250, win_size=512, fmin=0.0, fmax=None)  # hop % 4 != 0
FACTOR = 8.0


def lengths_for(P, tile):
    hop = P["hop_size"]
    if P is SHIPPED:
        return [385, 640, 1023, 1024, hop * tile - 1, hop * tile, hop * tile + 1, 2 * hop * tile + 37, 10560]
    return [max((P["n_fft"] - hop) // 2 + 1, hop), hop * tile - 1, hop * tile + hop + 1]  # one frame; either side of the tile


def scaled(kind, n, seed):
    import synthdata as synth  # (at the repository root: on the path under pytest, and a script puts it there first)
    x = synth.synth_waveform(n, seed=seed, kind=kind).astype(np.float64)
    peak = np.abs(x).max()
    return (x * (0.95 / peak) if peak > 0 else x).astype(np.float32)


def batch_of(waves):
    out = np.zeros((len(waves), max(len(w) for w in waves)), np.float32)
    for i, w in enumerate(waves):
        out[i, :len(w)] = w
    return out, [len(w) for w in waves]


def ref_kwargs(P):
    return dict(n_fft=P["n_fft"], num_mels=P["num_mels"], sr=P["sampling_rate"], hop=P["hop_size"], win=P["win_size"],
                fmin=P["fmin"], fmax=P["fmax"])


class Ref:
    """float64 oracle of a set of signals, the float32 path's per-frame error on them, and the bars that follow"""

    def __init__(self, waves, P):
        kw = ref_kwargs(P)
        self.waves = waves
        self.lin = [mel_ref.mel(w, dtype=torch.float64, log=False, **kw)[0].numpy() for w in waves]
        lin32 = [mel_ref.mel(w, dtype=torch.float32, log=False, **kw)[0].numpy().astype(np.float64) for w in waves]
        self.top = [m.max(axis=0) for m in self.lin]  # per frame
        self.e32 = max(float((np.abs(a - m).max(axis=0) / t).max()) for a, m, t in zip(lin32, self.lin, self.top))
        self.bar = FACTOR * self.e32
        self.log = [np.log(np.maximum(m, 1e-5)) for m in self.lin]
        self.tol = [self.bar * t[None, :] / np.maximum(m, 1e-5) for m, t in zip(self.lin, self.top)]

    def worst(self, i, got_lin):
        return float((np.abs(got_lin.astype(np.float64) - self.lin[i]).max(axis=0) / self.top[i]).max())


_refs = {}


def ref_of(kind, P):
    key = (kind, P["n_fft"], P["hop_size"])
    if key not in _refs:
        from dissc_amd.mel import TILE_FRAMES
        waves = [scaled(kind, n, seed=100 + i) for i, n in enumerate(lengths_for(P, TILE_FRAMES))]
        _refs[key] = Ref(waves, P)
    return _refs[key]


def run_forward(ms, waves, linear):
    x, ns = batch_of(waves)
    out = ms.forward(x, ns, linear=linear)
    mel, frames = out["mel"].cpu().numpy(), out["frames"].numpy()
    assert list(frames) == [n // ms.hop_size for n in ns]
    return [mel[i, :, :frames[i]] for i in range(len(waves))]
