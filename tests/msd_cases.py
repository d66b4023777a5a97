"""Shared by tests/test_msd_cpu.py, tests/test_gpu_msd.py and tests/golden/make_msd_golden.py (not a test module): the
MultiScaleDiscriminator of reference sr/models.py:285-333 restated as a torch module of spectral_norm(Conv1d) (discriminator 0) and
weight_norm(Conv1d) (discriminators 1 and 2) layers under the reference's checkpoint keys, in any dtype; seeded checkpoints with
unit-norm power-iteration buffers; the ragged paired composition dissc_amd.nn.MultiScaleDiscriminator runs (every utterance alone
on its valid samples, conv_grouped_ref.disc_s_ragged and pool_ref); both steps of the reference's loop (sr/train.py:157-190, the
scale side); and spectral norm written out by hand in float64 (snorm_ref) with its gradient formula and seeded defects.

The two-sigma rule: torch's spectral_norm runs one power iteration in every training-mode forward of a wrapped conv, and the
reference calls d(y) and then d(y_hat): one module forward performs two iterations, y sees W / sigma_1 and y_hat sees W / sigma_2.
TorchMSD.forward folds discriminator 0 twice, by torch's own SpectralNorm.compute_weight, once in front of each half."""
import numpy as np
import torch
import torch.nn.functional as F
from torch.nn.utils import spectral_norm, weight_norm

import conv_grouped_ref as R
import gan_loss_ref as GL

# (name, Cin, Cout, k, stride, groups) of DiscriminatorS's eight layers, reference sr/models.py:289-295
LAYERS = [(f"convs.{i}", cin, cout, k, s, g) for i, (cin, cout, k, s, g) in enumerate(R.DISC_S)] + \
         [("convs.6", 1024, 1024, 5, 1, 1), ("conv_post", 1024, 1, 3, 1, 1)]
SN_SHAPES = [(cout, cin // g * k) for _, cin, cout, k, _, g in LAYERS]  # weight_orig as [Cout, Cin / g * k]
EPS = 1e-12  # F.normalize's, as torch's spectral_norm passes it


def expected_shapes():
    """{checkpoint key: shape}: Conv1d's shapes; discriminator 0's weight_u [Cout] and weight_v [Cin / g * k] are buffers"""
    out = {}
    for i in range(3):
        for name, cin, cout, k, _, g in LAYERS:
            pre = f"discriminators.{i}.{name}"
            out[pre + ".bias"] = (cout,)
            if i == 0:
                out[pre + ".weight_orig"] = (cout, cin // g, k)
                out[pre + ".weight_u"] = (cout,)
                out[pre + ".weight_v"] = (cin // g * k,)
            else:
                out[pre + ".weight_g"] = (cout, 1, 1)
                out[pre + ".weight_v"] = (cout, cin // g, k)
    return out


def _unit(rs, n):
    x = rs.randn(n)
    return torch.from_numpy((x / np.sqrt((x * x).sum())).astype(np.float32))


def msd_state_dict(seed):
    """a seeded checkpoint: weights uniform / sqrt(fan-in); weight_g = ||v|| times a factor in [0.7, 1.3]; weight_u / weight_v of
    discriminator 0 seeded unit vectors (float32 roundings of them), NOT singular vectors: sigma moves from iteration to iteration"""
    rs = np.random.RandomState(seed)
    sd = {}
    for i in range(3):
        for name, cin, cout, k, _, g in LAYERS:
            pre = f"discriminators.{i}.{name}"
            fan = cin // g * k
            w = (rs.uniform(-1, 1, (cout, cin // g, k)) / np.sqrt(fan)).astype(np.float32)
            sd[pre + ".bias"] = torch.from_numpy((rs.uniform(-1, 1, cout) / np.sqrt(fan)).astype(np.float32))
            if i == 0:
                sd[pre + ".weight_orig"] = torch.from_numpy(w)
                sd[pre + ".weight_u"] = _unit(rs, cout)
                sd[pre + ".weight_v"] = _unit(rs, fan)
            else:
                norm = np.sqrt((w.astype(np.float64) ** 2).sum(axis=(1, 2), keepdims=True))
                sd[pre + ".weight_g"] = torch.from_numpy((norm * rs.uniform(0.7, 1.3, (cout, 1, 1))).astype(np.float32))
                sd[pre + ".weight_v"] = torch.from_numpy(w)
    return sd


class DiscS(torch.nn.Module):
    def __init__(self, use_spectral_norm=False):
        super().__init__()
        norm_f = spectral_norm if use_spectral_norm else weight_norm
        convs = [norm_f(torch.nn.Conv1d(cin, cout, k, s, groups=g, padding=(k - 1) // 2)) for _, cin, cout, k, s, g in LAYERS]
        self.convs = torch.nn.ModuleList(convs[:7])
        self.conv_post = convs[7]

    def named_convs(self):
        return [(f"convs.{j}", c) for j, c in enumerate(self.convs)] + [("conv_post", self.conv_post)]


def _sn_hook(conv):
    return next(h for h in conv._forward_pre_hooks.values() if type(h).__name__ == "SpectralNorm")


class TorchMSD(torch.nn.Module):
    """state_dict keys and shapes as the reference's MultiScaleDiscriminator; forward(y, y_hat, lengths) -> per scale the eight
    paired PRE-activation maps [2 B, C, ld] (rows of y first), every utterance alone on its valid samples.  In train() mode each
    forward runs TWO power iterations on discriminator 0, one in front of each half; in eval() none.  self.sigmas: the [2][8]
    values u . (W v) the last forward's halves used; one_sigma=True (a defect) folds once and uses that weight for both halves."""

    def __init__(self):
        super().__init__()
        self.discriminators = torch.nn.ModuleList([DiscS(True), DiscS(), DiscS()])
        self.sigmas = None

    def folded(self, i, iterate=None):
        """discriminator i's folded weights under nn.discriminator_s's keys, with the graph to the parameters; for i = 0 by torch's
        own SpectralNorm.compute_weight, which advances weight_u / weight_v in place when it iterates (default: self.training)"""
        w, sig = {}, []
        for name, conv in self.discriminators[i].named_convs():
            if i == 0:
                wt = _sn_hook(conv).compute_weight(conv, do_power_iteration=self.training if iterate is None else iterate)
                wm = conv.weight_orig.detach().reshape(conv.weight_orig.shape[0], -1)
                sig.append(torch.dot(conv.weight_u, torch.mv(wm, conv.weight_v)))
            else:
                wt = torch._weight_norm(conv.weight_v, conv.weight_g, 0)
            w[name + ".weight"] = wt
            w[name + ".bias"] = conv.bias
        return (w, torch.stack(sig)) if i == 0 else w

    def forward(self, y, y_hat, lengths=None, one_sigma=False, decisions=None):
        """decisions (Decisions, optional): the branch of every leaky ReLU is taken from its masks, not from the map's own sign"""
        B, T = y.shape[0], y.shape[-1]
        ln = [T] * B if lengths is None else [int(n) for n in lengths]
        mk = lambda i, h: None if decisions is None else [m[h * B:(h + 1) * B] for m in decisions.masks[i]]
        halves, sig = [], []
        for h, wav in enumerate((y, y_hat)):
            if h == 0 or not one_sigma:
                w, s = self.folded(0)
            sig.append(s)
            halves.append(disc_s_ragged(w, wav, ln, mk(0, h)))
        self.sigmas = torch.stack(sig).detach()
        out = [[torch.cat([a, b], 0) for a, b in zip(*halves)]]
        for i in (1, 2):
            y, y_hat = pool_ragged(y, ln), pool_ragged(y_hat, ln)
            ln = [R.pool_len(n) for n in ln]
            w = self.folded(i)
            a, b = disc_s_ragged(w, y, ln, mk(i, 0)), disc_s_ragged(w, y_hat, ln, mk(i, 1))
            out.append([torch.cat([ma, mb], 0) for ma, mb in zip(a, b)])
        self.maps = [[t.detach() for t in fm] for fm in out]  # the last forward's, for Decisions
        return out


class Decisions:
    """The branch decisions of one forward, read from a set of paired PRE-activation maps [scale][map]: masks[i][j] = x > 0 of map
    j < 7 (the leaky ReLU in front of the next layer and of the feature loss), signs[i][j] = sign(lrelu(real) - lrelu(gen)) of all
    eight (the feature loss's |.|).  The step's gradients are DISCONTINUOUS in these: every batch has map elements nearer to a
    kink or a tie than float32 resolves (measured on the float64 reference: the nearest of 1.2 M elements lies 1e-9 .. 1e-7 of
    its map's rms away, whatever the seed), where the branch is decided by rounding and a whole element of the gradient follows
    it.  As tests/conv_grad_ref.resblock1_ref does with its masks, the float64 and float32 references are therefore evaluated
    with the ENGINE's decisions: what is compared is the smooth function on the branch the engine took."""

    def __init__(self, fmaps):
        self.masks = [[m.detach().cpu() > 0 for m in fm[:7]] for fm in fmaps]
        self.signs = []
        for fm in fmaps:
            row = []
            for j, m in enumerate(fm):
                m = m.detach().cpu()
                B = m.shape[0] // 2
                a = F.leaky_relu(m, GL.SLOPE) if j < 7 else m
                row.append(torch.sign(a[:B] - a[B:]))
            self.signs.append(row)


def lrelu_by(x, mask):
    """leaky ReLU whose branch comes from ``mask`` (True: identity) when given, else from x's own sign"""
    return F.leaky_relu(x, GL.SLOPE) if mask is None else torch.where(mask, x, x * GL.SLOPE)


def disc_s_ragged(weights, wav, lengths, masks=None):
    """conv_grouped_ref.disc_s_ragged (the eight PRE-activation maps [B, C, ld], every utterance alone on its valid samples, zero
    beyond) with the leaky ReLUs' branches from ``masks`` (seven boolean [B, C, ld]) where given; without, it IS that function"""
    if masks is None:
        return R.disc_s_ragged(weights, wav, lengths)
    wav = wav.reshape(wav.shape[0], 1, -1)
    B, _, T = wav.shape
    lds = R.map_lds(T)
    per_map = [[] for _ in lds]
    for i in range(B):
        n = int(lengths[i])
        if n <= 0:
            for j, ld in enumerate(lds):
                per_map[j].append(torch.zeros(1, R.DISC_S_CHANNELS[j], ld, dtype=wav.dtype))
            continue
        x, lens = wav[i:i + 1, :, :n], R.map_lengths(n)
        for j, (name, (s, g, k)) in enumerate(zip(R.layer_names(), R.layer_params())):
            xin = x if j == 0 else lrelu_by(x, masks[j - 1][i:i + 1, :, :lens[j - 1]])
            x = F.conv1d(xin, weights[name + ".weight"], weights[name + ".bias"], stride=s, padding=(k - 1) // 2, groups=g)
            assert x.shape[2] == lens[j]
            per_map[j].append(F.pad(x, (0, lds[j] - x.shape[2])))
    return [torch.cat(ms, 0) for ms in per_map]


def fm_value(x, lens, B, j, decisions=None, i=0):
    """the feature loss's term of paired PRE-activation map j of scale i: 2 mean |lrelu(real) - lrelu(gen)| over the valid
    positions (map 7 as it is); with decisions, the leaky ReLU's branch and the sign of the difference are theirs"""
    if decisions is None:
        return GL.map_values(GL.FM, x, lens, B, GL.SLOPE if j < 7 else 1.0)[0]
    act = lrelu_by(x, decisions.masks[i][j]) if j < 7 else x
    real, gen = GL.valid_halves(act, lens, B)
    if real is None:
        return torch.zeros((), dtype=x.dtype)
    sg = decisions.signs[i][j].to(x.dtype)
    sign, _ = GL.valid_halves(torch.cat([sg, sg], 0), lens, B)
    return 2 * torch.mean(sign * (real - gen))


def pool_ragged(wav, lengths):
    """AvgPool1d(4, 2, padding=2) (reference sr/models.py:315) of every utterance alone on its valid samples, under autograd, laid
    out as nn.mean_pool's: [B, 1, ceil4(T // 2 + 1)], zero beyond n // 2 + 1.  conv_grouped_ref.pool_ref without the graph."""
    wav = wav.reshape(wav.shape[0], 1, -1)
    B, _, T = wav.shape
    ld = R.ceil4(T // 2 + 1)
    rows = []
    for i in range(B):
        n = int(lengths[i])
        if n <= 0:
            rows.append(torch.zeros(1, 1, ld, dtype=wav.dtype))
            continue
        p = F.avg_pool1d(wav[i:i + 1, :, :n], 4, 2, padding=2)
        assert p.shape[2] == R.pool_len(n)
        rows.append(F.pad(p, (0, ld - p.shape[2])))
    return torch.cat(rows, 0)


def torch_msd(sd, dtype, train=True):
    m = TorchMSD().to(dtype)
    m.load_state_dict({k: v.to(dtype) for k, v in sd.items()}, strict=True)
    return m.train(train)


def scale_lengths(lengths, B, T):
    """per scale the input lengths of its rows (one half): n, n // 2 + 1, and that again"""
    ln = [T] * B if lengths is None else [int(n) for n in lengths]
    out = [ln]
    for _ in range(2):
        out.append([R.pool_len(n) for n in out[-1]])
    return out


def map_lens(lengths, B, T):
    """[scale][map] -> the B per-row lengths (one half) of the 24 maps"""
    return [[[R.map_lengths(n)[j] if n > 0 else 0 for n in ln] for j in range(8)] for ln in scale_lengths(lengths, B, T)]


def losses(maps, T, lengths, B, decisions=None):
    """(loss_d, r_losses, g_losses, loss_fm, loss_gen, gen_losses) of TorchMSD's output by gan_loss_ref's ragged forms"""
    r_losses, g_losses, gen_losses = [], [], []
    loss_d = loss_fm = loss_gen = 0
    for i, (fm, lens) in enumerate(zip(maps, map_lens(lengths, B, T))):
        r, g = GL.map_values(GL.DISC, fm[7], lens[7], B)
        loss_d = loss_d + (r + g)
        r_losses.append(r)
        g_losses.append(g)
        ge, _ = GL.map_values(GL.GEN, fm[7], lens[7], B)
        loss_gen = loss_gen + ge
        gen_losses.append(ge)
        for j, m in enumerate(fm):
            loss_fm = loss_fm + fm_value(m, lens[j], B, j, decisions, i)
    return loss_d, r_losses, g_losses, loss_fm, loss_gen, gen_losses


def buffers(m):
    """{key: clone} of discriminator 0's weight_u / weight_v as the module holds them now"""
    return {k: v.detach().clone() for k, v in m.state_dict().items() if k.endswith(("weight_u", "weight_v")) and k.startswith("discriminators.0.")}


def d_step_ref(sd, y, y_hat, lengths, dtype, forwards_before=0, one_sigma=False, decisions=None):
    """the discriminator's step after ``forwards_before`` earlier training-mode forwards (which advance the buffers): (module
    after backward, loss_d, r_losses, g_losses); the gradients are on the module's parameters, module.sigmas the step's [2, 8];
    decisions: a Decisions whose branches replace the maps' own"""
    m = torch_msd(sd, dtype)
    y, y_hat = y.detach().to("cpu", dtype), y_hat.detach().to("cpu", dtype)
    B, T = y.shape[0], y.shape[-1]
    with torch.no_grad():
        for _ in range(forwards_before):
            m.folded(0), m.folded(0)
    loss_d, r_losses, g_losses, _, _, _ = losses(m(y, y_hat, lengths, one_sigma=one_sigma, decisions=decisions), T, lengths, B)
    loss_d.backward()
    return m, loss_d.detach(), torch.stack(r_losses).detach(), torch.stack(g_losses).detach()


def g_step_ref(sd, y, y_hat, lengths, dtype, forwards_before=0, decisions=None):
    """the generator's scale-side terms after ``forwards_before`` earlier forwards: (feature_loss, generator_loss, gen_losses,
    gradient of their sum to y_hat, module)"""
    m = torch_msd(sd, dtype)
    y = y.detach().to("cpu", dtype)
    y_hat = y_hat.detach().to("cpu", dtype).requires_grad_(True)
    B, T = y.shape[0], y.shape[-1]
    with torch.no_grad():
        for _ in range(forwards_before):
            m.folded(0), m.folded(0)
    _, _, _, loss_fm, loss_gen, gen_losses = losses(m(y, y_hat, lengths, decisions=decisions), T, lengths, B, decisions)
    (loss_fm + loss_gen).backward()
    return loss_fm.detach(), loss_gen.detach(), torch.stack(gen_losses).detach(), y_hat.grad, m


def wav_pair(seed, B, T):
    rs = np.random.RandomState(seed)
    return tuple(torch.from_numpy(rs.uniform(-1, 1, (B, 1, T)).astype(np.float32)) for _ in range(2))


# ---- spectral norm by hand, float64 -------------------------------------------------------------------------------------------
DEFECTS = ("skip_second_normalize", "sigma_from_u_in", "drop_uv_term", "float_reciprocal", "one_sigma")


def _normalize(x):
    return x / max(float(torch.sqrt((x * x).sum())), EPS)


def snorm_ref(W, u, v, iterate, gw=None, defect=None):
    """torch.nn.utils.spectral_norm's weight in float64 -> (w, u, v, sigma, gW or None).  W [rows, cols], u [rows], v [cols].
    iterate: v = normalize(W^T u), u = normalize(W v); else u and v as given.  sigma = u . (W v), w = W / sigma (a division).
    With gw (the gradient of w): gW = gw / sigma - (sum gw o W / sigma^2) u v^T, u and v constants.
    Defects (each caught by the assertion named in tests/test_msd_cpu.py): "skip_second_normalize" (u = W v as it is),
    "sigma_from_u_in" (sigma = u_in . (W v)), "drop_uv_term" (gW = gw / sigma), "float_reciprocal" (w = W * float32(1 / sigma)).
    ("one_sigma" is a defect of the module, TorchMSD.forward's.)"""
    W, u_in, v_in = W.double(), u.double(), v.double()
    u, v = u_in, v_in
    if iterate:
        v = _normalize(W.t() @ u_in)
        u = W @ v
        if defect != "skip_second_normalize":
            u = _normalize(u)
    sigma = torch.dot(u_in if defect == "sigma_from_u_in" else u, W @ v)
    if defect == "float_reciprocal":
        w = W * (1.0 / sigma).float().double()
    else:
        w = W / sigma
    gW = None
    if gw is not None:
        gw = gw.double()
        gW = gw / sigma
        if defect != "drop_uv_term":
            gW = gW - ((gw * W).sum() / sigma ** 2) * torch.outer(u, v)
    return w, u, v, sigma, gW


def snorm_torch(W, u, v, iterate, gw, dtype):
    """the same by torch's own operations in ``dtype``, in the order torch.nn.utils.spectral_norm applies them (F.normalize of
    torch.mv, torch.dot, weight / sigma, autograd for the gradient): the float32 yardstick of the GPU tests.
    -> (w, u, v, sigma, gW)"""
    W = W.detach().to("cpu", dtype).requires_grad_(True)
    u, v = u.detach().to("cpu", dtype), v.detach().to("cpu", dtype)
    if iterate:
        with torch.no_grad():
            v = F.normalize(torch.mv(W.t(), u), dim=0, eps=EPS)
            u = F.normalize(torch.mv(W, v), dim=0, eps=EPS)
    sigma = torch.dot(u, torch.mv(W, v))
    w = W / sigma
    (w * gw.detach().to("cpu", dtype)).sum().backward()
    return w.detach(), u, v, sigma.detach(), W.grad


def sigmas_after(sd, dtype, forwards):
    """[forward] -> the [2, 8] sigmas of discriminator 0's two folds in each of ``forwards`` training-mode forwards from ``sd``,
    and the buffers after each"""
    m = torch_msd(sd, dtype)
    out = []
    with torch.no_grad():
        for _ in range(forwards):
            s = torch.stack([m.folded(0)[1], m.folded(0)[1]])
            out.append((s, buffers(m)))
    return out

