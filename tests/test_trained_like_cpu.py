"""The trained-like checkpoint and inputs (synthdata kind="trained_like") and the float64 oracle, on the CPU.

tests/golden/gen_vctk_trainedlike.npz holds the reference CodeGenerator's waveforms on them (tests/golden/make_golden.py
generator_trained_like), in fp32 and with the folded module in float64.  These tests pin both oracle precisions to it, prove
the distribution really is harsh at every stage (so the GPU tests of tests/test_gpu_trained_like.py are not measured on benign
data), and keep kind="iid" byte-identical to the checkpoint every other fixture was made from."""
import hashlib
import os

import numpy as np
import pytest
import torch

from oracle import generator_ref as gr
import synthdata as synth

IID_SHA256 = "fdd86e27b0487f8829d94eaacdd05a30a375389c5281ff6ee958326f09f25a67"  # kind="iid", seed 0, as every fixture was made


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "gen_vctk_trainedlike.npz"))


@pytest.fixture(scope="module")
def folded():
    return gr.fold_state_dict(synth.synth_generator_state_dict(seed=0, kind="trained_like"))


@pytest.fixture(scope="module")
def run99(folded):
    """the float64 oracle on the T = 99 trained-like utterance: conv taps and the pre-tanh output"""
    w = gr.to_double(folded)
    code, f0, spkr, _ = synth.synth_generator_inputs(1, 99, seed=199, kind="trained_like")
    x = gr.embed_concat(w, torch.from_numpy(code), torch.from_numpy(f0), torch.from_numpy(spkr))
    conv_taps, pre = {}, {}
    y = gr.generator_forward(w, synth.VCTK_CONFIG, x, conv_taps=conv_taps, pre_tanh=pre)
    return conv_taps, pre["y"], y


def _sha(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.numpy().tobytes())
    return h.hexdigest()


def test_iid_checkpoint_is_unchanged():
    assert _sha(synth.synth_generator_state_dict(seed=0)) == IID_SHA256
    assert _sha(synth.synth_generator_state_dict(seed=0, kind="iid")) == IID_SHA256
    a, b = synth.synth_generator_inputs(3, 41, seed=21, ragged=True), synth.synth_generator_inputs(3, 41, seed=21, ragged=True,
                                                                                                   kind="iid")
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)
    with pytest.raises(ValueError):
        synth.synth_generator_state_dict(seed=0, kind="trained")


def test_trained_like_layout_and_statistics():
    iid = synth.synth_generator_state_dict(seed=0)
    sd = synth.synth_generator_state_dict(seed=0, kind="trained_like")
    assert list(sd) == list(iid) and len(sd) == 293
    for k in sd:
        assert sd[k].shape == iid[k].shape and sd[k].dtype == iid[k].dtype, k
    g = sd["resblocks.3.convs1.1.weight_g"].flatten().double()
    gi = iid["resblocks.3.convs1.1.weight_g"].flatten().double()
    assert 20 * np.log10(float(g.max() / g.min())) >= 30               # decades of per-channel gain
    assert (g > 10 * g.median()).sum() >= 2                             # outlier channels
    assert abs(float(g.pow(2).mean().sqrt() / gi.pow(2).mean().sqrt()) - 1) < 0.05  # the iid layer's RMS gain
    v = sd["resblocks.3.convs1.1.weight_v"].flatten().double()
    assert float(((v - v.mean()) ** 4).mean() / v.var() ** 2) - 3 >= 3  # heavy-tailed directions
    assert sd["ups.0.weight_g"].shape == (512, 1, 1)                    # per INPUT channel for ConvTranspose1d
    e = sd["dict.weight"].double()
    assert float(e.pow(2).mean(0).sqrt().max() / e.pow(2).mean(0).sqrt().median()) >= 5  # massive embedding dimensions
    code, f0, spkr, lengths = synth.synth_generator_inputs(4, 99, seed=5, kind="trained_like", ragged=True)
    for b in range(4):
        n = int(lengths[b])
        f = f0[b, 0, :n]
        assert np.abs(f).max() >= 6.0 and (f == 0).mean() >= 0.25        # f0 peaks at |6|, long exact-zero runs
        assert f[0] == 0 and f[n - 1] == 0 and code[b, 0] == code[b, n - 1] == synth.TL_SILENCE_CODE  # silence at both ends
        runs = np.diff(np.flatnonzero(np.diff(code[b, :n]) != 0))
        assert runs.size == 0 or runs.mean() >= 4                         # long code runs


@pytest.mark.parametrize("T", [33, 99])
def test_oracles_match_reference_on_trained_like(gold, folded, T):
    code, f0, spkr, _ = synth.synth_generator_inputs(1, T, seed=100 + T, kind="trained_like")
    y32 = gr.code_generator(folded, synth.VCTK_CONFIG, code, f0, spkr)
    y64 = gr.code_generator(gr.to_double(folded), synth.VCTK_CONFIG, code, f0, spkr)
    assert y32.dtype == torch.float32 and y64.dtype == torch.float64
    assert y64.shape == gold[f"T{T}/wav64"].shape == (1, 1, 320 * T)
    np.testing.assert_array_equal(y32.numpy(), gold[f"T{T}/wav"])     # the fp32 oracle: the reference's bits
    assert np.abs(y64.numpy() - gold[f"T{T}/wav64"]).max() <= 1e-12   # the float64 oracle: the reference run in float64
    # the fp32 path's own rounding on these weights: far inside the north-star bar, and measurable
    e = float((y32.double() - y64).pow(2).mean().sqrt())
    print(f"T={T}: fp32 oracle vs float64: rms {e:.3e}")
    assert 0 < e <= 1e-5


def test_float64_oracle_output_follows_its_weights(folded):
    """empty rows stay zero in the caller's dtype; taps come from utterance 0 only"""
    code, f0, spkr, _ = synth.synth_generator_inputs(2, 3, seed=1, kind="trained_like")
    taps = {}
    y = gr.code_generator(gr.to_double(folded), synth.VCTK_CONFIG, code, f0, spkr, lengths=np.array([3, 0]), conv_taps=taps)
    assert y.dtype == torch.float64 and not y[1].any()
    assert len(taps) == 15 * 3 * 4 and taps["resblocks.14.convs2.2"].shape == (1, 16, 960)
    assert taps["resblocks.0.convs1.0.x"].dtype == torch.float64


def _spread_db(a):
    r = np.sqrt((a.astype(np.float64) ** 2).mean(1))
    return 20 * np.log10(r.max() / max(r.min(), 1e-300))


def _excess_kurtosis(a):
    v = a.astype(np.float64).ravel()
    v = v - v.mean()
    return float((v ** 4).mean() / (v ** 2).mean() ** 2 - 3)


def test_trained_like_distribution_is_hard(run99):
    """at every stage: some ResBlock conv input with >= 30 dB of output-channel RMS spread and some with excess kurtosis >= 5;
    the waveform neither saturated (tanh would hide the GPU's errors) nor silent"""
    conv_taps, pre, y = run99
    for i in range(5):
        names = [f"resblocks.{3 * i + j}.convs{c}.{m}" for j in range(3) for c in (1, 2) for m in range(3)]
        spread = max(_spread_db(conv_taps[n][0].numpy()) for n in names)
        kurt = max(_excess_kurtosis(conv_taps[n][0].numpy()) for n in names)
        print(f"stage {i}: channel RMS spread {spread:.1f} dB, excess kurtosis {kurt:.1f}")
        assert spread >= 30, (i, spread)
        assert kurt >= 5, (i, kurt)
    p = pre.numpy().ravel()
    rms = float(np.sqrt(np.mean(p ** 2)))
    sat = float(np.mean(np.abs(y.numpy()) > 0.99))
    print(f"pre-tanh rms {rms:.3f}, |y| > 0.99 on {100 * sat:.2f} % of the samples")
    assert 0.05 <= rms <= 1.0
    assert sat < 0.01
