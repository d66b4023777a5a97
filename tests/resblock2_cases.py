"""Shared by the ResBlock2 tests (tests/test_resblock2_cpu.py, tests/test_gpu_resblock2.py) and the fixture recipe
tests/golden/make_resblock2_golden.py (not a test module): the HiFi-GAN V3 block table, configs with it, a seeded state dict in
the reference's ResBlock2 key layout (resblocks.{n}.convs.{0,1}.*), the generator as a float64 / float32 torch composition with
optional leaky-ReLU branch decisions (gen_train_ref's _forward for this block type), and a hand count of the model's FLOPs.
Block outputs are stored and compared on edge_cols() only."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

import synthdata as synth
from conv_grad_ref import _lrelu
from oracle import generator_ref as G

SLOPE = G.LRELU_SLOPE
POST_SLOPE = 0.01

# (k; d0, d1) of HiFi-GAN V3's three blocks; (7; 3, 12) has the widest taps: (k - 1) d1 = 72 columns
V3_BLOCKS = [(3, (1, 2)), (5, (2, 6)), (7, (3, 12))]
# The gain of every ResBlock2 conv: x + conv(lrelu(x)) twice per block; with 0.5 the reference's own waveforms of the fixture
# inputs peak at 0.86 (the recipe prints and asserts max |wav| < 0.99), off tanh saturation
RB2_GAIN = 0.5
GOLDEN_T = (1, 2, 7, 33, 99)
RAGGED_LENGTHS = [40, 23, 9, 1]
# block outputs at T = 7 are stored on these columns from either end of a row (all of a row no longer than twice that): both
# edges of every stage, with the 45-column reach of the (7; 3, 12) block inside, in a file below the size limit
EDGE_COLS = 96


def config(base):
    """`base` with the three V3 blocks"""
    return dict(base, resblock="2", resblock_kernel_sizes=[k for k, _ in V3_BLOCKS],
                resblock_dilation_sizes=[list(d) for _, d in V3_BLOCKS])


def vctk_config():
    return config(synth.VCTK_CONFIG)  # stage widths 256, 128, 64, 32, 16


def conv_names(h):
    """the weight-normed conv layers in the reference's parameter order"""
    nk, nu = len(h["resblock_kernel_sizes"]), len(h["upsample_rates"])
    names = ["conv_pre"] + [f"ups.{i}" for i in range(nu)]
    names += [f"resblocks.{n}.convs.{m}" for n in range(nu * nk) for m in range(2)]
    return names + ["conv_post"]


def state_dict(h, seed=0):
    """synthdata.synth_generator_state_dict's statistics in the ResBlock2 layout (a stream of its own: other keys, other draws)"""
    rs = np.random.RandomState(seed)
    sd = OrderedDict()
    c0, in_dim = h["upsample_initial_channel"], h.get("model_in_dim", 128)
    sd["conv_pre.bias"] = synth._t(0.1 * rs.standard_normal(c0))
    synth._wn_conv(rs, sd, "conv_pre", (c0, in_dim, 7), in_dim * 7, 1.0, c0)
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        cin, cout = c0 // 2 ** i, c0 // 2 ** (i + 1)
        sd[f"ups.{i}.bias"] = synth._t(0.1 * rs.standard_normal(cout))
        synth._wn_conv(rs, sd, f"ups.{i}", (cin, cout, k), cin * k / u, 1.4, cin)
    nk = len(h["resblock_kernel_sizes"])
    for i in range(len(h["upsample_rates"])):
        ch = c0 // 2 ** (i + 1)
        for j, k in enumerate(h["resblock_kernel_sizes"]):
            for m in range(2):
                name = f"resblocks.{i * nk + j}.convs.{m}"
                sd[name + ".bias"] = synth._t(0.1 * rs.standard_normal(ch))  # non-zero: bias + conv(zeros) is not zero padding
                synth._wn_conv(rs, sd, name, (ch, ch, k), ch * k, RB2_GAIN, ch)
    ch = c0 // 2 ** len(h["upsample_rates"])
    sd["conv_post.bias"] = synth._t(0.05 * rs.standard_normal(1))
    synth._wn_conv(rs, sd, "conv_post", (1, ch, 7), ch * 7, 0.35, 1)
    sd["dict.weight"] = synth._t(rs.standard_normal((h["num_embeddings"], h["embedding_dim"])))
    sd["spkr.weight"] = synth._t(rs.standard_normal((200, h["embedding_dim"])))
    return sd


def fold(sd, dtype=torch.float32):
    """{folded key: tensor}: weight = torch._weight_norm(weight_v, weight_g, 0), what remove_weight_norm leaves"""
    out = {}
    for k, v in sd.items():
        if k.endswith(".weight_g"):
            out[k[:-2]] = torch._weight_norm(sd[k[:-2] + "_v"].to(dtype), v.to(dtype), 0)
        elif not k.endswith(".weight_v"):
            out[k] = v.to(dtype)
    return out


def edge_cols(n):
    """the stored columns of a block output of n columns"""
    return np.arange(n) if n <= 2 * EDGE_COLS else np.concatenate([np.arange(EDGE_COLS), np.arange(n - EDGE_COLS, n)])


def resblock2_ref(w, prefix, x, k, dil, masks=None, taps=None):
    """reference sr/models.py:60-65 on folded weights w[prefix + "convs.<m>.weight" / ".bias"]; masks: an iterator of branch
    decisions (or None: x's own sign), one per conv input; taps receives the conv inputs"""
    for m, d in enumerate(dil):
        if taps is not None:
            taps.append(x.detach())
        xt = _lrelu(x, SLOPE, None if masks is None else next(masks))
        x = F.conv1d(xt, w[f"{prefix}convs.{m}.weight"], w[f"{prefix}convs.{m}.bias"], padding=G.get_padding(k, d), dilation=d) + x
    return x


def _forward(w, h, x, masks, taps):
    it = iter(masks) if masks is not None else None
    nxt = (lambda: None) if it is None else (lambda: next(it))

    def tap(t):
        if taps is not None:
            taps.append(t.detach())
        return t

    nk = len(h["resblock_kernel_sizes"])
    nxt()  # conv_pre has no activation in front
    x = F.conv1d(tap(x), w["conv_pre.weight"], w["conv_pre.bias"], padding=3)
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        x = _lrelu(tap(x), SLOPE, nxt())
        x = F.conv_transpose1d(x, w[f"ups.{i}.weight"], w[f"ups.{i}.bias"], stride=u, padding=(k - u) // 2)
        xs = None
        for j, (rk, rd) in enumerate(zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])):
            r = resblock2_ref(w, f"resblocks.{i * nk + j}.", x, rk, rd[:2], it, taps)
            xs = r if xs is None else xs + r
        x = xs / nk
    x = _lrelu(tap(x), POST_SLOPE, nxt())
    x = F.conv1d(x, w["conv_post.weight"], w["conv_post.bias"], padding=3)
    return torch.tanh(x)


def conv_input_rates(h):
    """columns per frame of every conv input, in call order"""
    nk = len(h["resblock_kernel_sizes"])
    out, m = [1], 1
    for u in h["upsample_rates"]:
        out.append(m)
        m *= u
        out += [m] * (2 * nk)
    return out + [m]


def generator_ref(sd, h, code, f0, spkr, lengths, dtype, gwav=None, masks=None, taps=None):
    """gen_train_ref.generator_ref for a ResBlock2 config: the generator on the UNFOLDED state dict in ``dtype`` on the CPU, every
    utterance alone on its valid length.  masks: per conv input (call order) a boolean tensor [B, C, >= its length]; taps receives
    this run's own conv inputs [B, C, L], zero beyond the lengths.  -> wav [B, 1, hop T], with gwav (wav, {key: gradient of
    sum(wav gwav)}) for every key of sd."""
    code, f0, spkr = torch.as_tensor(code), torch.as_tensor(f0), torch.as_tensor(spkr)
    P = {k: v.detach().to("cpu", dtype).requires_grad_(gwav is not None) for k, v in sd.items()}
    w = fold(P, dtype)
    B, T = code.shape
    hop = int(np.prod(h["upsample_rates"]))
    rates = conv_input_rates(h)
    wav = torch.zeros(B, 1, hop * T, dtype=dtype)
    loss, first = 0, taps is not None and not taps
    for b in range(B):
        n = int(lengths[b])
        if n <= 0:
            continue
        x = G.embed_concat(w, code[b:b + 1, :n], f0[b:b + 1, :, :n].to(dtype), spkr[b:b + 1])
        mb = None if masks is None else [m[b:b + 1, :, :r * n].cpu() for m, r in zip(masks, rates)]
        assert masks is None or len(masks) == len(rates)
        tb = [] if taps is not None else None
        y = _forward(w, h, x, mb, tb)
        wav[b, :, :hop * n] = y[0].detach()
        if taps is not None:
            if first:
                taps.extend(torch.zeros(B, t.shape[1], t.shape[2] // n * T, dtype=dtype) for t in tb)
                first = False
            for dst, t in zip(taps, tb):
                dst[b, :, :t.shape[2]] = t[0]
        if gwav is not None:
            loss = loss + (y * gwav[b:b + 1, :, :hop * n].detach().to("cpu", dtype)).sum()
    if gwav is None:
        return wav
    if torch.is_tensor(loss):
        loss.backward()
    return wav, {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in P.items()}


def flops_per_frame(h):
    """2 x the multiply-adds of one code frame, counted by hand from the config: conv_pre, per stage the upsampler (at its input
    rate) and two C x C x k convs per block (at its output rate), conv_post"""
    c0, macs, mul = h["upsample_initial_channel"], h["model_in_dim"] * h["upsample_initial_channel"] * 7, 1
    for i, (u, ku) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        cin, cout = c0 >> i, c0 >> (i + 1)
        macs += cin * cout * ku * mul
        mul *= u
        macs += sum(2 * cout * cout * k for k in h["resblock_kernel_sizes"]) * mul
    return 2 * (macs + (c0 >> len(h["upsample_rates"])) * 7 * mul)
