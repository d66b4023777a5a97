"""Deterministic synthetic checkpoints and inputs for tests, benchmarks and profiling.

Not part of the oracle and not part of the compute path: pure numpy/torch generators of
random-but-reproducible weights in the reference's checkpoint layouts and of input batches.

No real DISSC checkpoint exists offline (Google-Drive links, reference
README.md:76,93,117,142), so parity is pinned on synthetic weights laid out
exactly like the reference's checkpoints:

* vocoder  ``g_########`` = ``{'generator': state_dict}`` with 97 weight-normed
  conv layers x {bias, weight_g, weight_v} + ``dict.weight`` + ``spkr.weight``
  (reference sr/train.py:205-214, sr/models.py:72-96,125-135).
* predictors ``best_model.pth`` = plain ``state_dict`` (reference
  train_len_predictor.py:101-103, train_f0_predictor.py:98-100).

Everything is drawn from ``numpy.random.RandomState`` (frozen legacy stream) so
the same seed gives the same bytes in this container and on the GPU box.
"""
from collections import OrderedDict

import numpy as np
import torch

VCTK_CONFIG = {
    "resblock": "1",
    "upsample_rates": [5, 4, 4, 2, 2],
    "upsample_kernel_sizes": [11, 8, 8, 4, 4],
    "upsample_initial_channel": 512,
    "resblock_kernel_sizes": [3, 7, 11],
    "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]],
    "num_embeddings": 100,
    "embedding_dim": 128,
    "model_in_dim": 257,
    "code_hop_size": 320,
    "f0": True,
    "multispkr": "_",
    "f0_normalize": False,
    "sampling_rate": 16000,
}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a.astype(np.float32)))


def _wn_conv(rs, sd, name, shape, fan_in, gain, g_dim0):
    """weight_v ~ N(0,1); weight_g = ||v|| * N(1,0.1)*gain/sqrt(fan_in)*sqrt(numel/g_dim0)
    so the folded weight has std ~ gain/sqrt(fan_in)."""
    v = rs.standard_normal(shape)
    norm = np.sqrt((v.reshape(shape[0], -1) ** 2).sum(1))
    per = np.sqrt(np.prod(shape[1:]))
    g = (gain / np.sqrt(fan_in)) * per * (1.0 + 0.1 * rs.standard_normal(shape[0]))
    # g multiplies v/||v||: effective per-element std = g/per
    del norm
    sd[name + ".weight_g"] = _t(g.reshape((shape[0],) + (1,) * (len(shape) - 1)))
    sd[name + ".weight_v"] = _t(v)


# kind="trained_like": heavy-tailed statistics in the spirit of trained HiFi-GAN checkpoints (frozen; tuned until the checks of
# tests/test_trained_like_cpu.py hold): per-channel gains log-normal with sigma TL_GAIN_SIGMA (~40 dB of spread) and TL_OUTLIERS
# (2-4) channels per layer at TL_OUTLIER_GAIN x, renormalised so the layer's RMS gain is the iid value; directions Student-t with
# TL_T_DOF degrees of freedom; biases TL_BIAS_STD * N(0,1); TL_MASSIVE_DIMS embedding dimensions at TL_MASSIVE_SCALE x; conv_post
# at RMS gain TL_POST_GAIN (iid: 0.35) so the waveform stays off tanh saturation (pre-tanh RMS 0.24 / 0.36 at T = 99 / 33).
TL_GAIN_SIGMA = 1.2
TL_OUTLIERS = (2, 4)
TL_OUTLIER_GAIN = 30.0
TL_T_DOF = 3.0
TL_BIAS_STD = 0.3
TL_MASSIVE_DIMS = 3
TL_MASSIVE_SCALE = 10.0
TL_POST_GAIN = 0.12


def _wn_conv_trained_like(rs, sd, name, shape, fan_in, gain, g_dim0):
    """weight_v ~ Student-t(TL_T_DOF); weight_g = a per-channel gain (log-normal x outliers), RMS-renormalised to
    gain / sqrt(fan_in) * sqrt(numel / g_dim0) (the iid layer's RMS)."""
    v = rs.standard_t(TL_T_DOF, size=shape)
    per = np.sqrt(np.prod(shape[1:]))
    c = np.exp(TL_GAIN_SIGMA * rs.standard_normal(shape[0]))
    if shape[0] >= 16:
        n_out = rs.randint(TL_OUTLIERS[0], TL_OUTLIERS[1] + 1)
        c[rs.choice(shape[0], n_out, replace=False)] = TL_OUTLIER_GAIN * np.median(c)
    c /= np.sqrt(np.mean(c ** 2))
    g = (gain / np.sqrt(fan_in)) * per * c
    sd[name + ".weight_g"] = _t(g.reshape((shape[0],) + (1,) * (len(shape) - 1)))
    sd[name + ".weight_v"] = _t(v)


def _embedding_trained_like(rs, n, dim):
    e = rs.standard_normal((n, dim))
    e[:, rs.choice(dim, TL_MASSIVE_DIMS, replace=False)] *= TL_MASSIVE_SCALE
    return e


def synth_generator_state_dict(h=None, seed=0, kind="iid"):
    """State dict with the reference's 293 keys.

    kind "iid": N(0,1) directions, per-channel gains N(1, 0.1), biases 0.1 N(0,1) (every existing fixture);
    "trained_like": the heavy-tailed statistics above (same keys, layouts and per-layer RMS gains)."""
    if kind == "trained_like":
        return _synth_generator_state_dict_trained_like(h, seed)
    if kind != "iid":
        raise ValueError(f"kind {kind!r}: 'iid' or 'trained_like'")
    h = h or VCTK_CONFIG
    rs = np.random.RandomState(seed)
    sd = OrderedDict()
    c0 = h["upsample_initial_channel"]
    in_dim = h.get("model_in_dim", 128)
    # conv_pre: Conv1d(in_dim, c0, 7)
    sd["conv_pre.bias"] = _t(0.1 * rs.standard_normal(c0))
    _wn_conv(rs, sd, "conv_pre", (c0, in_dim, 7), in_dim * 7, 1.0, c0)
    # ups: ConvTranspose1d weight [Cin, Cout, k]; weight_g is per *input* channel
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        cin, cout = c0 // 2 ** i, c0 // 2 ** (i + 1)
        sd[f"ups.{i}.bias"] = _t(0.1 * rs.standard_normal(cout))
        _wn_conv(rs, sd, f"ups.{i}", (cin, cout, k), cin * k / u, 1.4, cin)
    # resblocks
    nk = len(h["resblock_kernel_sizes"])
    for i in range(len(h["upsample_rates"])):
        ch = c0 // 2 ** (i + 1)
        for j, k in enumerate(h["resblock_kernel_sizes"]):
            idx = i * nk + j
            for grp, gain in (("convs1", 1.4), ("convs2", 0.6)):
                for m in range(3):
                    name = f"resblocks.{idx}.{grp}.{m}"
                    sd[name + ".bias"] = _t(0.1 * rs.standard_normal(ch))
                    _wn_conv(rs, sd, name, (ch, ch, k), ch * k, gain, ch)
    ch = c0 // 2 ** len(h["upsample_rates"])
    sd["conv_post.bias"] = _t(0.05 * rs.standard_normal(1))
    _wn_conv(rs, sd, "conv_post", (1, ch, 7), ch * 7, 0.35, 1)
    sd["dict.weight"] = _t(rs.standard_normal((h["num_embeddings"], h["embedding_dim"])))
    sd["spkr.weight"] = _t(rs.standard_normal((200, h["embedding_dim"])))
    return sd


def _synth_generator_state_dict_trained_like(h, seed):
    h = h or VCTK_CONFIG
    rs = np.random.RandomState(seed)
    sd = OrderedDict()
    c0 = h["upsample_initial_channel"]
    in_dim = h.get("model_in_dim", 128)
    sd["conv_pre.bias"] = _t(TL_BIAS_STD * rs.standard_normal(c0))
    _wn_conv_trained_like(rs, sd, "conv_pre", (c0, in_dim, 7), in_dim * 7, 1.0, c0)
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        cin, cout = c0 // 2 ** i, c0 // 2 ** (i + 1)
        sd[f"ups.{i}.bias"] = _t(TL_BIAS_STD * rs.standard_normal(cout))
        _wn_conv_trained_like(rs, sd, f"ups.{i}", (cin, cout, k), cin * k / u, 1.4, cin)
    nk = len(h["resblock_kernel_sizes"])
    for i in range(len(h["upsample_rates"])):
        ch = c0 // 2 ** (i + 1)
        for j, k in enumerate(h["resblock_kernel_sizes"]):
            idx = i * nk + j
            for grp, gain in (("convs1", 1.4), ("convs2", 0.6)):
                for m in range(3):
                    name = f"resblocks.{idx}.{grp}.{m}"
                    sd[name + ".bias"] = _t(TL_BIAS_STD * rs.standard_normal(ch))
                    _wn_conv_trained_like(rs, sd, name, (ch, ch, k), ch * k, gain, ch)
    ch = c0 // 2 ** len(h["upsample_rates"])
    sd["conv_post.bias"] = _t(0.05 * rs.standard_normal(1))
    _wn_conv_trained_like(rs, sd, "conv_post", (1, ch, 7), ch * 7, TL_POST_GAIN, 1)
    sd["dict.weight"] = _t(_embedding_trained_like(rs, h["num_embeddings"], h["embedding_dim"]))
    sd["spkr.weight"] = _t(_embedding_trained_like(rs, 200, h["embedding_dim"]))
    return sd


# kind="trained_like" inputs (frozen, as above): f0 z-scores with TL_F0_PEAKS frames per utterance pushed to |6|, unvoiced runs of
# mean TL_UNVOICED_RUN frames (TL_UNVOICED_P of the runs), code runs of mean TL_CODE_RUN frames, and leading / trailing silence
# (code TL_SILENCE_CODE, f0 exactly 0) over TL_SILENCE_FRAC of the frames at each end.
TL_F0_PEAKS = 2
TL_UNVOICED_RUN = 25.0
TL_UNVOICED_P = 0.4
TL_CODE_RUN = 8.0
TL_SILENCE_CODE = 0
TL_SILENCE_FRAC = 0.15


def synth_generator_inputs(B, T, seed=1234, ragged=False, n_spk=108, n_codes=100, kind="iid"):
    """runs of a uniform symbol (geometric, mean 2.5 frames),
    f0 ~ N(0,1) with ~35% exact-zero unvoiced runs, spkr uniform.

    kind "trained_like": the harsher inputs above (long code runs, long exact-zero unvoiced runs, f0 peaks at |6|, silence at
    both ends of every utterance)."""
    if kind == "trained_like":
        return _synth_generator_inputs_trained_like(B, T, seed, ragged, n_spk, n_codes)
    if kind != "iid":
        raise ValueError(f"kind {kind!r}: 'iid' or 'trained_like'")
    rs = np.random.RandomState(seed)
    code = np.zeros((B, T), dtype=np.int64)
    f0 = np.zeros((B, 1, T), dtype=np.float32)
    for b in range(B):
        t = 0
        while t < T:
            run = rs.geometric(1 / 2.5)
            code[b, t:t + run] = rs.randint(0, n_codes)
            t += run
        f0[b, 0] = rs.standard_normal(T)
        t = 0
        while t < T:
            run = rs.geometric(1 / 12.0)
            if rs.rand() < 0.35:
                f0[b, 0, t:t + run] = 0.0
            t += run
    spkr = rs.randint(0, n_spk, size=(B, 1)).astype(np.int64)
    if ragged:
        lengths = rs.randint(max(1, T // 2), T + 1, size=B).astype(np.int32)
        lengths[0] = T
    else:
        lengths = np.full(B, T, dtype=np.int32)
    return code, f0, spkr, lengths


def _synth_generator_inputs_trained_like(B, T, seed, ragged, n_spk, n_codes):
    rs = np.random.RandomState(seed)
    code = np.zeros((B, T), dtype=np.int64)
    f0 = np.zeros((B, 1, T), dtype=np.float32)
    lengths = np.full(B, T, dtype=np.int32)
    if ragged:
        lengths = rs.randint(max(1, T // 2), T + 1, size=B).astype(np.int32)
        lengths[0] = T
    for b in range(B):
        n = int(lengths[b])
        t = 0
        while t < T:
            run = rs.geometric(1 / TL_CODE_RUN)
            code[b, t:t + run] = rs.randint(0, n_codes)
            t += run
        f0[b, 0] = rs.standard_normal(T)
        t = 0
        while t < T:
            run = rs.geometric(1 / TL_UNVOICED_RUN)
            if rs.rand() < TL_UNVOICED_P:
                f0[b, 0, t:t + run] = 0.0
            t += run
        s = int(round(TL_SILENCE_FRAC * n))  # silence at both ends of the utterance's own length
        peaks = rs.randint(s, max(s + 1, n - s), size=TL_F0_PEAKS)  # inside the voiced part
        f0[b, 0, peaks] = 6.0 * rs.choice([-1.0, 1.0], size=TL_F0_PEAKS)
        if s > 0:
            for sl in (slice(0, s), slice(n - s, n)):
                code[b, sl] = TL_SILENCE_CODE
                f0[b, 0, sl] = 0.0
    spkr = rs.randint(0, n_spk, size=(B, 1)).astype(np.int64)
    return code, f0, spkr, lengths


# ----------------------------------------------------------------------------------------------
# predictors (reference model/len_predictor.py, model/pitch_predictor.py)
# ----------------------------------------------------------------------------------------------
def _conv(rs, sd, name, cout, cin, k, gain=1.4):
    sd[name + ".weight"] = _t(rs.standard_normal((cout, cin, k)) * gain / np.sqrt(cin * k))
    sd[name + ".bias"] = _t(0.1 * rs.standard_normal(cout))


def _bn(rs, sd, name, c=128):
    sd[name + ".weight"] = _t(1.0 + 0.2 * rs.standard_normal(c))
    sd[name + ".bias"] = _t(0.1 * rs.standard_normal(c))
    sd[name + ".running_mean"] = _t(0.2 * rs.standard_normal(c))
    sd[name + ".running_var"] = _t(0.5 + rs.rand(c))
    sd[name + ".num_batches_tracked"] = torch.tensor(1000, dtype=torch.int64)


def synth_len_state_dict(n_tokens=100, n_speakers=108, seed=1):
    """53 keys: token_emb, spk_emb, cnn1/bn1, cnn11..16/bn11..16, cnn2."""
    rs = np.random.RandomState(seed)
    sd = OrderedDict()
    sd["token_emb.weight"] = _t(rs.standard_normal((n_tokens + 1, 32)))
    sd["spk_emb.weight"] = _t(rs.standard_normal((n_speakers, 32)))
    _conv(rs, sd, "cnn1", 128, 64, 3)
    _bn(rs, sd, "bn1")
    for i in range(1, 7):
        _conv(rs, sd, f"cnn1{i}", 128, 128, 3)
        _bn(rs, sd, f"bn1{i}")
    _conv(rs, sd, "cnn2", 1, 128, 3, gain=0.12)  # lens ~ 2.6 +- 0.5 for any seed / speaker count
    return sd


def synth_len_norm_stats():
    """len_norm_stats.pth = (mean, std) tensors (reference train_len_predictor.py:32)."""
    return torch.tensor(2.6), torch.tensor(1.7)


def synth_pitch_state_dict(kind="new", n_tokens=100, n_speakers=108, seed=2):
    """'new': 34 keys incl. buffer pe.pe [1,850,32]; 'base': 78 keys (BN after every conv but cnn2)."""
    rs = np.random.RandomState(seed)
    sd = OrderedDict()
    sd["token_emb.weight"] = _t(rs.standard_normal((n_tokens + 1, 32)))
    sd["spk_emb.weight"] = _t(rs.standard_normal((n_speakers + 1, 32)))
    if kind == "new":
        lin = torch.linspace(0, 1, 850).unsqueeze(-1)
        sd["pe.pe"] = torch.cat([lin.repeat_interleave(16, -1), torch.linspace(1, 0, 850).unsqueeze(-1)
                                 .repeat_interleave(16, -1)], -1).unsqueeze(0)
    names = ["cnn1"] + [f"cnn1{i}" for i in range(1, 8)]
    for n in names:
        _conv(rs, sd, n, 128, 64 if n == "cnn1" else 128, 3)
        if kind == "base":
            _bn(rs, sd, "bn" + n[3:])
    if kind == "new":
        _bn(rs, sd, "bn2")
    _conv(rs, sd, "cnn2", 128, 128, 3)
    _conv(rs, sd, "cnn_class1", 128, 128, 3)
    if kind == "base":
        _bn(rs, sd, "bn_c1")
    _conv(rs, sd, "cnn_class2", 1, 128, 1, gain=1.0)
    _conv(rs, sd, "cnn_reg1", 128, 128, 3)
    if kind == "base":
        _bn(rs, sd, "bn_r1")
    _conv(rs, sd, "cnn_reg2", 1, 128, 1, gain=1.0)
    return sd


def synth_unit_sequences(n, T_lo=60, T_hi=500, seed=99, n_codes=100):
    """Random unit sequences with geometric run lengths (mean 2.5), like encode output."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        T = int(rs.randint(T_lo, T_hi + 1))
        seq = np.zeros(T, dtype=np.int64)
        t = 0
        prev = -1
        while t < T:
            run = rs.geometric(1 / 2.5)
            c = int(rs.randint(0, n_codes))
            if c == prev:
                c = (c + 1) % n_codes
            seq[t:t + run] = c
            prev = c
            t += run
        out.append(seq)
    return out


# ----------------------------------------------------------------------------------------------
# HuBERT-base (fairseq checkpoint key names) + k-means centroids
# ----------------------------------------------------------------------------------------------
def synth_hubert_state_dict(n_layers=6, seed=3, kind="iid"):
    """fairseq HuBERT-base keys.  kind "iid": N(0,1) weights at unit RMS gain (q / k gain 1.5), LayerNorm gains N(1, 0.1) (every
    existing fixture); "trained_like": the heavy-tailed statistics of the HT_* constants below (same keys and layouts)."""
    if kind == "trained_like":
        return _synth_hubert_state_dict_trained_like(n_layers, seed)
    if kind != "iid":
        raise ValueError(f"kind {kind!r}: 'iid' or 'trained_like'")
    rs = np.random.RandomState(seed)
    sd = OrderedDict()
    convs = [(512, 1, 10)] + [(512, 512, 3)] * 4 + [(512, 512, 2)] * 2
    for i, (co, ci, k) in enumerate(convs):
        sd[f"feature_extractor.conv_layers.{i}.0.weight"] = _t(rs.standard_normal((co, ci, k)) * 1.6 / np.sqrt(ci * k))
    sd["feature_extractor.conv_layers.0.2.weight"] = _t(1.0 + 0.2 * rs.standard_normal(512))
    sd["feature_extractor.conv_layers.0.2.bias"] = _t(0.1 * rs.standard_normal(512))

    def ln(name, c):
        sd[name + ".weight"] = _t(1.0 + 0.1 * rs.standard_normal(c))
        sd[name + ".bias"] = _t(0.05 * rs.standard_normal(c))

    def lin(name, co, ci, gain=1.0):
        sd[name + ".weight"] = _t(rs.standard_normal((co, ci)) * gain / np.sqrt(ci))
        sd[name + ".bias"] = _t(0.05 * rs.standard_normal(co))

    ln("layer_norm", 512)
    lin("post_extract_proj", 768, 512)
    v = rs.standard_normal((768, 48, 128))
    sd["encoder.pos_conv.0.weight_v"] = _t(v)
    sd["encoder.pos_conv.0.weight_g"] = _t((np.sqrt((v ** 2).sum((0, 1), keepdims=True))
                                            * 1.2 / np.sqrt(48 * 128)) * (1 + 0.1 * rs.standard_normal((1, 1, 128))))
    sd["encoder.pos_conv.0.bias"] = _t(0.05 * rs.standard_normal(768))
    ln("encoder.layer_norm", 768)
    for i in range(n_layers):
        p = f"encoder.layers.{i}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            lin(p + "self_attn." + n, 768, 768, 1.5 if n in ("q_proj", "k_proj") else 1.0)
        ln(p + "self_attn_layer_norm", 768)
        lin(p + "fc1", 3072, 768)
        lin(p + "fc2", 768, 3072)
        ln(p + "final_layer_norm", 768)
    return sd


# kind="trained_like" HuBERT (frozen; tuned until the checks of tests/test_trained_like_hubert_cpu.py hold):
#  * feature convs: Student-t(HT_T_DOF) directions, per-output-channel gains log-normal with sigma HT_GAIN_SIGMA, HT_OUTLIERS channels
#    at HT_OUTLIER_GAIN x the median gain and HT_DEAD_FRAC all-zero (dead) channels, RMS-renormalised to the iid layer's gain;
#    GroupNorm gamma log-normal (sigma HT_GN_SIGMA) with HT_GN_NEAR_ZERO gammas at HT_GN_ZERO_GAMMA, beta HT_GN_BETA_STD * N(0,1);
#  * massive activations: HT_MASSIVE residual dimensions whose beta is HT_MASSIVE_BETA (signs random) in every encoder LayerNorm and
#    whose out_proj / fc2 bias is HT_MASSIVE_BIAS_FRAC x that beta, so |x| stays at 1e2 .. 1e3 after every LayerNorm; the other
#    dimensions' gamma is log-normal (sigma HT_LN_SIGMA), and x HT_LN_GAMMA in the LayerNorms of the layers: there the massive
#    dimensions dominate the LayerNorm's variance and would otherwise squash the rest to ~1e-2.  Every projection reading the residual stream sees the massive
#    dimensions' columns scaled by HT_MASSIVE_COL (they act as a bias, as in trained models);
#  * attention: per-head q / k gains geometric over HT_QK_GAIN (order shuffled), so the largest |logit| spans ~1 .. ~80 over the
#    heads; head HT_SINK_HEAD of every layer is a sink whose query is dominated by a bias of norm HT_SINK_QBIAS (every query picks the
#    same few keys);
#  * fc1 / fc2: Student-t rows; pos_conv weight_g spread over HT_POS_DECADES decades across the 128 kernel positions.
HT_T_DOF = 3.0
HT_GAIN_SIGMA = 1.0
HT_OUTLIERS = 3
HT_OUTLIER_GAIN = 30.0
HT_DEAD_FRAC = 0.05
HT_GN_SIGMA = 0.5
HT_GN_NEAR_ZERO = 4
HT_GN_ZERO_GAMMA = 1e-3
HT_GN_BETA_STD = 0.5
HT_MASSIVE = 4
HT_MASSIVE_BETA = (150.0, 300.0, 600.0, 1000.0)
HT_MASSIVE_BIAS_FRAC = 0.5
HT_MASSIVE_COL = 0.001
HT_LN_GAMMA = 40.0
HT_LN_SIGMA = 0.3
HT_QK_GAIN = (0.4, 4.0)
HT_SINK_HEAD = 11
HT_SINK_QBIAS = 60.0
HT_POS_DECADES = 3.0


def hubert_massive_dims(seed=3):
    """the residual dimensions kind="trained_like" makes massive (a function of the seed only)"""
    return np.sort(np.random.RandomState(seed + 1000).choice(768, HT_MASSIVE, replace=False))


def _t_rows(rs, co, ci, gain, shape=None):
    """Student-t directions at the iid RMS gain gain / sqrt(fan_in)"""
    w = rs.standard_t(HT_T_DOF, size=shape or (co, ci))
    return w * (gain / np.sqrt(ci) / np.sqrt(np.mean(w ** 2)))


def _synth_hubert_state_dict_trained_like(n_layers, seed):
    rs = np.random.RandomState(seed)
    sd = OrderedDict()
    convs = [(512, 1, 10)] + [(512, 512, 3)] * 4 + [(512, 512, 2)] * 2
    for i, (co, ci, k) in enumerate(convs):
        w = rs.standard_t(HT_T_DOF, size=(co, ci, k))
        w /= np.sqrt((w.reshape(co, -1) ** 2).mean(1))[:, None, None]
        c = np.exp(HT_GAIN_SIGMA * rs.standard_normal(co))
        c[rs.choice(co, HT_OUTLIERS, replace=False)] = HT_OUTLIER_GAIN * np.median(c)
        c[rs.choice(co, int(round(HT_DEAD_FRAC * co)), replace=False)] = 0.0
        c /= np.sqrt(np.mean(c ** 2))
        sd[f"feature_extractor.conv_layers.{i}.0.weight"] = _t(w * (c * 1.6 / np.sqrt(ci * k))[:, None, None])
    g = np.exp(HT_GN_SIGMA * rs.standard_normal(512))
    g[rs.choice(512, HT_GN_NEAR_ZERO, replace=False)] = HT_GN_ZERO_GAMMA
    sd["feature_extractor.conv_layers.0.2.weight"] = _t(g)
    sd["feature_extractor.conv_layers.0.2.bias"] = _t(HT_GN_BETA_STD * rs.standard_normal(512))
    mdims = hubert_massive_dims(seed)
    mbeta = np.asarray(HT_MASSIVE_BETA) * rs.choice([-1.0, 1.0], size=HT_MASSIVE)

    def ln(name, c, massive, gain=HT_LN_GAMMA):
        gm = np.exp(HT_LN_SIGMA * rs.standard_normal(c))
        bt = 0.05 * rs.standard_normal(c)
        if massive:
            gm *= gain
            gm[mdims] = 1.0
            bt[mdims] = mbeta
        sd[name + ".weight"] = _t(gm)
        sd[name + ".bias"] = _t(bt)

    def lin(name, co, ci, gain=1.0, reads_x=True, massive_bias=False):
        w = _t_rows(rs, co, ci, gain)
        if reads_x and ci == 768:
            w[:, mdims] *= HT_MASSIVE_COL
        b = 0.05 * rs.standard_normal(co)
        if massive_bias:
            b[mdims] = HT_MASSIVE_BIAS_FRAC * mbeta
        sd[name + ".weight"] = _t(w)
        sd[name + ".bias"] = _t(b)
        return w, b

    ln("layer_norm", 512, False)
    lin("post_extract_proj", 768, 512, reads_x=False)
    v = rs.standard_normal((768, 48, 128))
    spread = 10.0 ** (HT_POS_DECADES * (rs.rand(128) - 0.5))
    spread /= np.sqrt(np.mean(spread ** 2))
    sd["encoder.pos_conv.0.weight_v"] = _t(v)
    sd["encoder.pos_conv.0.weight_g"] = _t(np.sqrt((v ** 2).sum((0, 1), keepdims=True)) * 1.2 / np.sqrt(48 * 128)
                                           * spread[None, None, :])
    sd["encoder.pos_conv.0.bias"] = _t(0.1 * rs.standard_normal(768))
    ln("encoder.layer_norm", 768, True, gain=1.0)  # its input has no massive dimensions yet
    for i in range(n_layers):
        p = f"encoder.layers.{i}."
        hg = np.exp(np.linspace(np.log(HT_QK_GAIN[0]), np.log(HT_QK_GAIN[1]), 12))[rs.permutation(12)]
        for n in ("q_proj", "k_proj"):
            w, b = lin(p + "self_attn." + n, 768, 768)
            w *= np.repeat(hg, 64)[:, None]
            if n == "q_proj":
                u = rs.standard_normal(64)
                b[HT_SINK_HEAD * 64:(HT_SINK_HEAD + 1) * 64] = HT_SINK_QBIAS * u / np.linalg.norm(u)
            sd[p + "self_attn." + n + ".weight"] = _t(w)
            sd[p + "self_attn." + n + ".bias"] = _t(b)
        lin(p + "self_attn.v_proj", 768, 768)
        lin(p + "self_attn.out_proj", 768, 768, massive_bias=True)
        ln(p + "self_attn_layer_norm", 768, True)
        lin(p + "fc1", 3072, 768)
        lin(p + "fc2", 768, 3072, reads_x=False, massive_bias=True)
        ln(p + "final_layer_norm", 768, True)
    return sd


def synth_kmeans_centers(k=100, dim=768, seed=4):
    return _t(np.random.RandomState(seed).standard_normal((k, dim)) * 0.7)


# kind="speech_like" waveforms (frozen): a harmonic-plus-noise source (f0 WF_F0 Hz with a slow glide, WF_HARMONICS harmonics at
# 1/k, noise WF_NOISE of the harmonic RMS) under a syllabic envelope (WF_SYLLABLE_HZ) spanning WF_ENV_DB dB, peak WF_PEAK; exact
# digital silence over WF_EDGE_S seconds at both ends and one gap in the middle (WF_GAP_S seconds, or a third of a short
# utterance); WF_BURSTS short bursts driven into clipping at +-32767/32768; int16-quantised (k / 32768).  kind "speech_dc": the same
# plus a DC offset of WF_DC (silence included); kind "dither": 1-LSB dither only (samples in {-1, 0, 1} / 32768).
WF_F0 = (90.0, 240.0)
WF_HARMONICS = 12
WF_NOISE = 0.3
WF_SYLLABLE_HZ = 4.0
WF_ENV_DB = 40.0
WF_PEAK = 0.3
WF_EDGE_S = 0.15
WF_GAP_S = 1.0
WF_BURSTS = 2
WF_DC = 0.05


def _speech_like(n, rs):
    t = np.arange(n) / 16000.0
    f0 = WF_F0[0] + (WF_F0[1] - WF_F0[0]) * rs.rand()
    f = f0 * (1.0 + 0.15 * np.sin(2 * np.pi * (0.3 + 0.4 * rs.rand()) * t + 2 * np.pi * rs.rand()))
    ph = 2 * np.pi * np.cumsum(f) / 16000.0
    x = sum(np.sin(k * ph + 2 * np.pi * rs.rand()) / k for k in range(1, WF_HARMONICS + 1))
    x = x / np.sqrt(np.mean(x ** 2)) + WF_NOISE * rs.standard_normal(n)
    env_db = -WF_ENV_DB * 0.5 * (1.0 - np.cos(2 * np.pi * WF_SYLLABLE_HZ * t + 2 * np.pi * rs.rand()))
    x = WF_PEAK * x * 10.0 ** (env_db / 20.0) / 3.0
    for _ in range(WF_BURSTS):
        a = rs.randint(0, max(1, n - 800))
        x[a:a + 800] *= 40.0
    edge = min(int(WF_EDGE_S * 16000), n // 8)
    gap = int(WF_GAP_S * 16000) if n >= 3 * int(WF_GAP_S * 16000) else n // 3
    x[:edge] = 0.0
    x[n - edge:] = 0.0
    g0 = (n - gap) // 2
    x[g0:g0 + gap] = 0.0
    return x


def synth_waveform(n, seed=0, kind="iid"):
    """kind "iid": N(0,0.1) noise + a few tones, clipped to [-1,1] (every existing fixture); "speech_like",
    "speech_dc", "dither": the int16-quantised waveforms above."""
    if kind == "iid":
        return _synth_waveform_iid(n, seed)
    rs = np.random.RandomState(seed)
    if kind == "dither":
        q = rs.randint(-1, 2, size=n).astype(np.float64)
    elif kind in ("speech_like", "speech_dc"):
        x = _speech_like(n, rs)
        if kind == "speech_dc":
            x = x + WF_DC
        q = np.clip(np.round(x * 32768.0), -32767, 32767)
    else:
        raise ValueError(f"kind {kind!r}: 'iid', 'speech_like', 'speech_dc' or 'dither'")
    return (q / 32768.0).astype(np.float32)


def _synth_waveform_iid(n, seed):
    """N(0,0.1) noise + a few tones, clipped to [-1,1]"""
    rs = np.random.RandomState(seed)
    t = np.arange(n) / 16000.0
    x = 0.1 * rs.standard_normal(n) + 0.2 * np.sin(2 * np.pi * (110 + 40 * rs.rand()) * t) \
        + 0.1 * np.sin(2 * np.pi * (900 + 300 * rs.rand()) * t)
    return np.clip(x, -1, 1).astype(np.float32)
