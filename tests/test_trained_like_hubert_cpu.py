"""The trained-like HuBERT checkpoint, waveforms and centres (synthdata kind="trained_like" / "speech_like") and the float64
oracle, on the CPU.

tests/golden/hubert_trainedlike.npz holds HF HubertModel's hidden_states[1..6] on them (tests/golden/make_golden.py
hubert_trained_like), in fp32 and with the module in float64, and the k-means centres fitted on the float64 oracle's layer-6
features.  These tests pin both oracle precisions to it per layer, prove the distribution really is harsh (so the GPU tests of
tests/test_gpu_hubert_trained_like.py are not measured on benign data), and keep kind="iid" byte-identical to the checkpoint every
other HuBERT fixture was made from."""
import hashlib
import os

import numpy as np
import pytest
import torch

from oracle import hubert_ref as hr
import synthdata as synth

HUBERT_IID_SHA256 = "5dabce539ad4ca43a800ee9958e11fd0d6b57882737b10efd9a17e4a1c842feb"  # kind="iid", 6 layers, seed 3
UTTS = (("speech_like", 32000, 31), ("speech_dc", 16000, 32), ("dither", 8000, 33))  # make_golden.HUBERT_TL_UTTS
FP32_FRAME_BAR = 2e-7  # fp32 oracle vs HF fp32, per frame (l2, relative): measured <= 5.2e-8 on every layer and utterance


def _sha(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.numpy().tobytes())
    return h.hexdigest()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "hubert_trainedlike.npz"))


@pytest.fixture(scope="module")
def sd():
    return synth.synth_hubert_state_dict(6, kind="trained_like")


@pytest.fixture(scope="module")
def runs(sd, gold):
    """per fixture utterance: (wav, float64 taps, fp32 taps, float64 logits per layer, float64 units, fp32 units)"""
    sd64 = hr.to_double(sd)
    c = torch.from_numpy(gold["centers"])
    out = {}
    for kind, n, seed in UTTS:
        wav = torch.from_numpy(synth.synth_waveform(n, seed=seed, kind=kind))[None]
        t64, t32, lg = [], [], []
        u64, _ = hr.encode(sd64, c, wav, taps=t64, logits=lg)
        u32, _ = hr.encode(sd, c, wav, taps=t32)
        out[kind] = (wav, [t[0] for t in t64], [t[0] for t in t32], lg, u64, u32)
    return out


def test_iid_hubert_checkpoint_and_waveform_are_unchanged():
    assert _sha(synth.synth_hubert_state_dict(6)) == HUBERT_IID_SHA256
    assert _sha(synth.synth_hubert_state_dict(6, seed=3, kind="iid")) == HUBERT_IID_SHA256
    np.testing.assert_array_equal(synth.synth_waveform(719, seed=719), synth.synth_waveform(719, seed=719, kind="iid"))
    with pytest.raises(ValueError):
        synth.synth_hubert_state_dict(6, kind="trained")
    with pytest.raises(ValueError):
        synth.synth_waveform(400, kind="speech")


def test_trained_like_layout_and_waveforms(sd):
    iid = synth.synth_hubert_state_dict(6)
    assert list(sd) == list(iid)
    for k in sd:
        assert sd[k].shape == iid[k].shape and sd[k].dtype == iid[k].dtype, k
    for kind in ("speech_like", "speech_dc", "dither"):
        w = synth.synth_waveform(40000, seed=1, kind=kind).astype(np.float64)
        q = w * 32768
        assert np.array_equal(q, np.round(q)) and np.abs(q).max() <= 32767  # int16-quantised
    w = synth.synth_waveform(48000, seed=1, kind="speech_like")
    assert (w[:2400] == 0).all() and (w[-2400:] == 0).all()                 # exact digital silence at both ends
    assert (w[16000:32000] == 0).all()                                       # a 1 s gap in the middle
    assert (np.abs(w) == np.float32(32767 / 32768)).sum() >= 20              # clipped bursts
    assert abs(float(synth.synth_waveform(40000, seed=1, kind="speech_dc").mean())) >= 0.04
    assert set(np.unique(synth.synth_waveform(4000, seed=1, kind="dither") * 32768)) == {-1.0, 0.0, 1.0}


def test_oracles_match_hf_per_layer(gold, runs):
    """float64 oracle == HF float64 to 1e-10 (relative, per frame and layer); fp32 oracle == HF fp32 within FP32_FRAME_BAR"""
    for kind, _, _ in UTTS:
        _, t64, t32, _, _, _ = runs[kind]
        f = gold[f"{kind}/frames"]
        hs32 = gold[f"{kind}/hs32"]
        hs64 = hs32.astype(np.float64) + gold[f"{kind}/hs64d"]
        for L in range(6):
            a64, a32 = t64[L].numpy()[f], t32[L].double().numpy()[f]
            assert t64[L].dtype == torch.float64 and t32[L].dtype == torch.float32
            r64 = (np.linalg.norm(a64 - hs64[L], axis=1) / np.linalg.norm(hs64[L], axis=1)).max()
            r32 = (np.linalg.norm(a32 - hs32[L], axis=1) / np.linalg.norm(hs32[L], axis=1)).max()
            print(f"{kind} layer {L + 1}: float64 oracle vs HF {r64:.1e}, fp32 oracle vs HF fp32 {r32:.1e}")
            assert r64 <= 1e-10, (kind, L, r64)
            assert r32 <= FP32_FRAME_BAR, (kind, L, r32)


def test_trained_like_distribution_is_hard(sd, gold, runs):
    """massive residual dimensions at 1e2 .. 1e3 after every layer; the largest head logit from < 1 to > 80 over the heads;
    dead feature-conv channels; silent frames; most frames ambiguous for the k-means at the fp32 oracle's own error"""
    md = synth.hubert_massive_dims()
    for i in range(7):
        w = sd[f"feature_extractor.conv_layers.{i}.0.weight"]
        assert int((w.reshape(512, -1).abs().sum(1) == 0).sum()) >= 20, i
    for kind, _, _ in UTTS:
        wav, t64, t32, lg, u64, u32 = runs[kind]
        for L in range(6):
            m = t64[L][:, md].abs()
            assert float(m.min()) >= 100 and float(m.max()) >= 900, (kind, L)
        heads = torch.stack(lg)
        assert float(heads.max()) >= 80 and float(heads.min()) <= 1, kind
        d64, d32 = t64[5], t32[5].double()
        eps = (d32 - d64).norm(dim=1)
        _, amb = hr.unit_flip_allowed(d64, gold["centers"], eps)
        T = d64.shape[0]
        silent = sum(1 for t in range(T) if not wav[0, 320 * t:320 * t + 400].any())
        print(f"{kind}: T {T}, silent frames {silent}, ambiguous {amb}, largest logit {float(heads.max()):.1f}, "
              f"fp32 oracle unit flips {int((u32 != u64).sum())}")
        assert amb >= T // 2, (kind, amb)
        if kind == "speech_like":
            assert silent >= 30
