"""Shared by tests/test_gan_loss_cpu.py and tests/test_gpu_mpd.py (not a test module): the MultiPeriodDiscriminator of reference
sr/models.py:228-286 restated as a torch module of weight_norm(Conv2d) layers under the reference's checkpoint keys, in any dtype,
run per utterance on its valid samples (conv_strided_ref.disc_p_conv2d) and laid out as dissc_amd.nn.MultiPeriodDiscriminator's
paired maps; seeded checkpoints; and both steps of the reference's loop (sr/train.py:157-190, the period side) on top of it."""
import numpy as np
import torch
from torch.nn.utils import weight_norm

import conv_strided_ref as R
import gan_loss_ref as GL

PERIODS = (2, 3, 5, 7, 11)  # reference sr/models.py:267
LAYERS = [("convs.0", 1, 32, 5), ("convs.1", 32, 128, 5), ("convs.2", 128, 512, 5), ("convs.3", 512, 1024, 5),
          ("convs.4", 1024, 1024, 5), ("conv_post", 1024, 1, 3)]  # (name, Cin, Cout, k), reference sr/models.py:233-239


def expected_shapes(periods=PERIODS):
    """{checkpoint key: shape}: 18 tensors per period, Conv2d's shapes"""
    out = {}
    for i in range(len(periods)):
        for name, cin, cout, k in LAYERS:
            pre = f"discriminators.{i}.{name}"
            out[pre + ".bias"] = (cout,)
            out[pre + ".weight_g"] = (cout, 1, 1, 1)
            out[pre + ".weight_v"] = (cout, cin, k, 1)
    return out


def mpd_state_dict(seed, periods=PERIODS):
    """a seeded checkpoint: weight_v uniform / sqrt(Cin k), weight_g = ||v|| times a factor in [0.7, 1.3] (not the norm itself:
    a module that dropped g would show), bias uniform / sqrt(Cin k)"""
    rs = np.random.RandomState(seed)
    sd = {}
    for i in range(len(periods)):
        for name, cin, cout, k in LAYERS:
            pre = f"discriminators.{i}.{name}"
            v = (rs.uniform(-1, 1, (cout, cin, k, 1)) / np.sqrt(cin * k)).astype(np.float32)
            norm = np.sqrt((v.astype(np.float64) ** 2).sum(axis=(1, 2, 3), keepdims=True))
            sd[pre + ".bias"] = torch.from_numpy((rs.uniform(-1, 1, cout) / np.sqrt(cin * k)).astype(np.float32))
            sd[pre + ".weight_g"] = torch.from_numpy((norm * rs.uniform(0.7, 1.3, (cout, 1, 1, 1))).astype(np.float32))
            sd[pre + ".weight_v"] = torch.from_numpy(v)
    return sd


class DiscP(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.convs = torch.nn.ModuleList([weight_norm(torch.nn.Conv2d(cin, cout, (k, 1), (3, 1) if j < 4 else 1, padding=((k - 1) // 2, 0)))
                                          for j, (_, cin, cout, k) in enumerate(LAYERS[:5])])
        _, cin, cout, k = LAYERS[5]
        self.conv_post = weight_norm(torch.nn.Conv2d(cin, cout, (k, 1), 1, padding=((k - 1) // 2, 0)))


class TorchMPD(torch.nn.Module):
    """state_dict keys and shapes as the reference's MultiPeriodDiscriminator; forward(y, y_hat, lengths) -> per period the six
    paired PRE-activation maps [2 B p, C, ld] (rows of y first), every utterance alone on its valid samples"""

    def __init__(self, periods=PERIODS):
        super().__init__()
        self.periods = tuple(periods)
        self.discriminators = torch.nn.ModuleList([DiscP() for _ in self.periods])

    def folded(self, i):
        """discriminator i's weights g v / ||v|| under nn.discriminator_p's keys, with the graph to weight_g / weight_v"""
        d = self.discriminators[i]
        w = {}
        for name, conv in [(f"convs.{j}", c) for j, c in enumerate(d.convs)] + [("conv_post", d.conv_post)]:
            w[name + ".weight"] = torch._weight_norm(conv.weight_v, conv.weight_g, 0)
            w[name + ".bias"] = conv.bias
        return w

    def forward(self, y, y_hat, lengths=None):
        out = []
        for i, p in enumerate(self.periods):
            w = self.folded(i)
            a, b = R.disc_p_conv2d(w, y, p, lengths), R.disc_p_conv2d(w, y_hat, p, lengths)
            out.append([torch.cat([ma, mb], 0) for ma, mb in zip(a, b)])
        return out


def torch_mpd(sd, dtype, periods=PERIODS):
    m = TorchMPD(periods).to(dtype)
    m.load_state_dict({k: v.to(dtype) for k, v in sd.items()}, strict=True)
    return m


def map_lens(T, lengths, B, period):
    """the six maps' per-row lengths [B p] (one half) as lists of ints"""
    masks = R.map_masks(T, period, lengths, B)
    return [[int(v) for v in m[:, 0].sum(1)] for m in masks]


def losses(maps, T, lengths, B, periods=PERIODS):
    """(loss_d, r_losses, g_losses, loss_fm, loss_gen, gen_losses) of TorchMPD's output by gan_loss_ref's ragged forms"""
    r_losses, g_losses, gen_losses = [], [], []
    loss_d = loss_fm = loss_gen = 0
    for fm, p in zip(maps, periods):
        lens = map_lens(T, lengths, B, p)
        r, g = GL.map_values(GL.DISC, fm[5], lens[5], B * p)
        loss_d = loss_d + (r + g)
        r_losses.append(r)
        g_losses.append(g)
        ge, _ = GL.map_values(GL.GEN, fm[5], lens[5], B * p)
        loss_gen = loss_gen + ge
        gen_losses.append(ge)
        for j, m in enumerate(fm):
            loss_fm = loss_fm + GL.map_values(GL.FM, m, lens[j], B * p, GL.SLOPE if j < 5 else 1.0)[0]
    return loss_d, r_losses, g_losses, loss_fm, loss_gen, gen_losses


def d_step_ref(sd, y, y_hat, lengths, dtype, periods=PERIODS):
    """the discriminator's step: (module after backward, loss_d, r_losses, g_losses); the gradients are on the module's parameters"""
    m = torch_mpd(sd, dtype, periods)
    y, y_hat = y.detach().to("cpu", dtype), y_hat.detach().to("cpu", dtype)
    B, T = y.shape[0], y.shape[-1]
    loss_d, r_losses, g_losses, _, _, _ = losses(m(y, y_hat, lengths), T, lengths, B, periods)
    loss_d.backward()
    return m, loss_d.detach(), torch.stack(r_losses).detach(), torch.stack(g_losses).detach()


def g_step_ref(sd, y, y_hat, lengths, dtype, periods=PERIODS):
    """the generator's period-side terms: (feature_loss, generator_loss, gen_losses, gradient of their sum to y_hat)"""
    m = torch_mpd(sd, dtype, periods)
    y = y.detach().to("cpu", dtype)
    y_hat = y_hat.detach().to("cpu", dtype).requires_grad_(True)
    B, T = y.shape[0], y.shape[-1]
    _, _, _, loss_fm, loss_gen, gen_losses = losses(m(y, y_hat, lengths), T, lengths, B, periods)
    (loss_fm + loss_gen).backward()
    return loss_fm.detach(), loss_gen.detach(), torch.stack(gen_losses).detach(), y_hat.grad


def wav_pair(seed, B, T):
    rs = np.random.RandomState(seed)
    return tuple(torch.from_numpy(rs.uniform(-1, 1, (B, 1, T)).astype(np.float32)) for _ in range(2))
