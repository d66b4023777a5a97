"""Shared by tests/test_gen_train_cpu.py and tests/test_gpu_gen_train.py (not a test module): float64 / float32 CPU
restatements, under torch autograd, of what dissc_amd.nn adds for the generator's training step -- weight norm
(torch._weight_norm, the primitive the reference's hook evaluates), the embeddings (oracle.generator_ref.embed_concat), the
whole generator on the reference's UNFOLDED state dict (oracle.generator_ref.generator_forward's ops in its order), with
optional leaky-ReLU branch decisions per conv input as conv_grad_ref._lrelu takes them.  Every utterance is run alone on its
valid length, as the reference does."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import generator_ref as G
from conv_grad_ref import _lrelu

SLOPE = G.LRELU_SLOPE
POST_SLOPE = 0.01  # F.leaky_relu's default (reference sr/models.py:110)

SMALL_CONFIG = {
    "resblock": "1", "upsample_rates": [4, 2], "upsample_kernel_sizes": [8, 4], "upsample_initial_channel": 64,
    "resblock_kernel_sizes": [3, 7], "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5]], "num_embeddings": 20,
    "embedding_dim": 16, "model_in_dim": 33, "f0": True, "multispkr": "_",
}
TINY_CONFIG = dict(SMALL_CONFIG, upsample_rates=[2], upsample_kernel_sizes=[4], upsample_initial_channel=4,
                   resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1, 3, 5]], num_embeddings=5, embedding_dim=2, model_in_dim=5)


def weight_norm_ref(v, g, gw, dtype):
    """v [rows, ...], g [rows] (any shape with rows elements), gw like v (or None) -> (w, gv, gg): w = g v / ||v|| over every
    dim but 0 and the gradients of sum(w gw)"""
    v = v.detach().to("cpu", dtype).requires_grad_(True)
    g = g.detach().to("cpu", dtype).reshape((v.shape[0],) + (1,) * (v.dim() - 1)).requires_grad_(True)
    w = torch._weight_norm(v, g, 0)
    if gw is None:
        return w.detach(), torch.zeros_like(v), torch.zeros(v.shape[0], dtype=dtype)
    (w * gw.detach().to("cpu", dtype).reshape(v.shape)).sum().backward()
    return w.detach(), v.grad, g.grad.reshape(-1)


def embed_ref(dict_w, spkr_w, code, f0, spkr, lengths, gx, dtype):
    """x [B, C, T] (zero beyond lengths) and the dense gradients (g_dict, g_spkr) of sum(x gx); code i64 [B, T], f0 [B, T],
    spkr i64 [B], already at one rate; ids clamped into the tables as the engine does"""
    w = {"dict.weight": dict_w.detach().to("cpu", dtype).requires_grad_(True),
         "spkr.weight": spkr_w.detach().to("cpu", dtype).requires_grad_(True)}
    code = code.cpu().clamp(0, dict_w.shape[0] - 1)
    spkr = spkr.cpu().clamp(0, spkr_w.shape[0] - 1)
    B, T = code.shape
    E = dict_w.shape[1]
    x = torch.zeros(B, 2 * E + 1, T, dtype=dtype)
    loss = 0
    for b in range(B):
        n = int(lengths[b])
        if n <= 0:
            continue
        xb = G.embed_concat(w, code[b:b + 1, :n], f0[b:b + 1, None, :n].cpu().to(dtype), spkr[b:b + 1].reshape(1, 1))
        x[b, :, :n] = xb[0].detach()
        if gx is not None:
            loss = loss + (xb * gx[b:b + 1, :, :n].detach().to("cpu", dtype)).sum()
    if torch.is_tensor(loss):
        loss.backward()
    z = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    return x, z(w["dict.weight"]), z(w["spkr.weight"])


def _forward(w, h, x, masks, taps):
    """oracle.generator_ref.generator_forward with each leaky ReLU's branch from ``masks`` (a list in conv call order:
    conv_pre's input, per stage the upsampler's and its ResBlocks' six each, conv_post's; None: x's own sign).  taps: a list
    that receives this evaluation's own conv inputs in the same order."""
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
            p = f"resblocks.{i * nk + j}"
            r = x
            for m, d in enumerate(rd):
                xt = _lrelu(tap(r), SLOPE, nxt())
                xt = F.conv1d(xt, w[f"{p}.convs1.{m}.weight"], w[f"{p}.convs1.{m}.bias"], padding=G.get_padding(rk, d), dilation=d)
                xt = _lrelu(tap(xt), SLOPE, nxt())
                xt = F.conv1d(xt, w[f"{p}.convs2.{m}.weight"], w[f"{p}.convs2.{m}.bias"], padding=G.get_padding(rk, 1))
                r = xt + r
            xs = r if xs is None else xs + r
        x = xs / nk
    x = _lrelu(tap(x), POST_SLOPE, nxt())
    x = F.conv1d(x, w["conv_post.weight"], w["conv_post.bias"], padding=3)
    return torch.tanh(x)


def generator_ref(sd, h, code, f0, spkr, lengths, dtype, gwav=None, masks=None, taps=None):
    """the generator on the UNFOLDED state dict ``sd`` in ``dtype`` on the CPU.  code i64 [B, T], f0 [B, 1, T], spkr i64
    [B, 1], lengths [B].  masks: per conv input (call order) a boolean tensor [B, C, >= its length] -- the branch decisions to
    use; taps: receives this run's own conv inputs as [B, C, L] tensors, zero beyond the lengths.  Returns wav [B, 1, hop T],
    or with gwav (wav, {key: gradient of sum(wav gwav)}) for every key of sd."""
    code, f0, spkr = torch.as_tensor(code), torch.as_tensor(f0), torch.as_tensor(spkr)
    P = {k: v.detach().to("cpu", dtype).requires_grad_(gwav is not None) for k, v in sd.items()}
    w = {}
    for k, v in P.items():
        if k.endswith(".weight_g"):
            w[k[:-2]] = torch._weight_norm(P[k[:-2] + "_v"], v, 0)
        elif not k.endswith(".weight_v"):
            w[k] = v
    B, T = code.shape
    hop = int(np.prod(h["upsample_rates"]))
    wav = torch.zeros(B, 1, hop * T, dtype=dtype)
    loss, first = 0, taps is not None and not taps
    for b in range(B):
        n = int(lengths[b])
        if n <= 0:
            continue
        x = G.embed_concat(w, code[b:b + 1, :n], f0[b:b + 1, :, :n].to(dtype), spkr[b:b + 1])
        mb = None if masks is None else [m[b:b + 1] for m in masks]
        if mb is not None:  # cut every mask to this utterance's length at that conv
            mb = _cut_masks(mb, h, n)
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


def conv_input_rates(h):
    """columns per frame of every conv input, in call order"""
    nk = len(h["resblock_kernel_sizes"])
    out, m = [1], 1
    for u in h["upsample_rates"]:
        out.append(m)
        m *= u
        out += [m] * (6 * nk)
    return out + [m]


def _cut_masks(mb, h, n):
    rates = conv_input_rates(h)
    assert len(rates) == len(mb), (len(rates), len(mb))
    return [m[:, :, :r * n].cpu() for m, r in zip(mb, rates)]
