"""Stage-by-stage restatement of one predictor TRAINING step (TEST INFRASTRUCTURE).

oracle/train_ref.py states the step as forward + torch autograd; this file states it the way dissc_amd/csrc/train.hip
computes it: one plain torch function per kernel (or per kernel pair), each taking the tensors that kernel reads and
returning what it writes, with the backward passes written out by hand.  Every function is dtype-generic: float64 is the
reference, float32 on the CPU is the yardstick the engine's error is measured against.

``run`` strings the stages together.  Without ``taps`` every stage reads what the stage before it produced (a whole
step: tests/test_train_stages_cpu.py holds that chain to oracle.train_ref.train_step in float64).  With ``taps`` (the
engine's own buffers, Trainer.tap / grads / state_dict / adam_state) every stage reads the ENGINE's inputs to that
stage, so no upstream rounding and no LeakyReLU branch decision enters a comparison: the derivative rule is the
engine's, ``!(a > 0) -> slope``, applied to the engine's own ``a``.

Keys of the result (and of ``taps``): 'x0', 'dx0', '<conv>/z|a|da|dz|mean|invstd', 'loss', 'grad/<param>',
'after/<param or running statistic>', 'm/<param>', 'v/<param>'.
"""
import torch
import torch.nn.functional as F

BN_EPS, BN_MOM, SLOPE, E = 1e-5, 0.1, 0.01, 32
ADAM_B1, ADAM_B2 = 0.9, 0.999


def layers(kind):
    """the conv layers in the engine's order: trunk, head branches, scalar heads (cout 1).  inp: producing layer, -1 = x0"""
    def lay(conv, bn, cin, cout, k, leaky, inp):
        return dict(conv=conv, bn=bn, cin=cin, cout=cout, k=k, leaky=leaky, inp=inp)
    if kind == "len":
        return [lay("cnn1", "bn1", 2 * E, 128, 3, True, -1)] + \
               [lay(f"cnn1{i}", f"bn1{i}", 128, 128, 3, True, i - 1) for i in range(1, 7)] + \
               [lay("cnn2", None, 128, 1, 3, False, 6)]
    base = kind == "base"
    return [lay("cnn1", "bn1" if base else None, 2 * E, 128, 3, True, -1)] + \
           [lay(f"cnn1{i}", f"bn1{i}" if base else None, 128, 128, 3, True, i - 1) for i in range(1, 8)] + \
           [lay("cnn2", None if base else "bn2", 128, 128, 3, True, 7),
            lay("cnn_class1", "bn_c1" if base else None, 128, 128, 3, True, 8),
            lay("cnn_reg1", "bn_r1" if base else None, 128, 128, 3, True, 8),
            lay("cnn_class2", None, 128, 1, 1, False, 9),
            lay("cnn_reg2", None, 128, 1, 1, False, 10)]


def trainable_keys(kind):
    keys = ["token_emb.weight", "spk_emb.weight"]
    for l in layers(kind):
        keys += [l["conv"] + ".weight", l["conv"] + ".bias"]
        if l["bn"]:
            keys += [l["bn"] + ".weight", l["bn"] + ".bias"]
    return keys


# ---------------------------------------------------------------------------------------------------------
# the stages
# ---------------------------------------------------------------------------------------------------------
def embed(seq, spk, keep, pe_mult, tok, spe, pe):
    """x0 [B, 2E, L]: rows < E = keep * token_emb[seq]; rows >= E = (spk_emb[spk] (+ pe[t])) (* pe_mult)"""
    B, L = seq.shape
    xt = tok[seq] * keep[:, :, None]
    xs = spe[spk][:, None, :].expand(B, L, E)
    if pe is not None:
        xs = xs + pe.reshape(-1, E)[:L][None]
    if pe_mult is not None:
        xs = xs * pe_mult
    return torch.cat([xt, xs], dim=-1).transpose(1, 2).contiguous()


def conv_fwd(x, w, b):
    """'same' Conv1d; a scalar head (one output row) returns [B, L]"""
    z = F.conv1d(x, w, b, padding=(w.shape[2] - 1) // 2)
    return z[:, 0] if w.shape[0] == 1 else z


def bn_stats(z, run_mean, run_var, unbiased_n=None):
    """batch mean / 1/sqrt(biased var + eps) over (batch, time) and the updated running statistics"""
    n = z.shape[0] * z.shape[2]
    mean = z.mean(dim=(0, 2))
    var = ((z - mean[None, :, None]) ** 2).mean(dim=(0, 2))
    invstd = 1.0 / torch.sqrt(var + BN_EPS)
    div = max(n - 1, 1) if unbiased_n is None else unbiased_n
    return mean, invstd, (1 - BN_MOM) * run_mean + BN_MOM * mean, (1 - BN_MOM) * run_var + BN_MOM * (var * n / div)


def act(z, mean, invstd, gamma, beta, leaky):
    v = z
    if mean is not None:
        v = (z - mean[None, :, None]) * invstd[None, :, None] * gamma[None, :, None] + beta[None, :, None]
    return torch.where(v > 0, v, v * SLOPE) if leaky else v


def len_loss(hz, tgt, pad, nmean, nstd):
    """LenSumLoss on pred = hz * nstd + nmean: masked squared error + 0.5 * squared sum of the differences over each
    complete group of four positions that holds no padding.  Returns (loss, d loss / d hz)."""
    B, L = hz.shape
    diff = (hz * nstd + nmean) - tgt
    mask = (tgt != pad).to(hz.dtype)
    loss = (mask * diff * diff).sum()
    g = 2 * mask * diff
    ng = L // 4
    if ng:
        s = diff[:, :4 * ng].reshape(B, ng, 4).sum(-1)
        m4 = (~(tgt[:, :4 * ng].reshape(B, ng, 4) == pad).any(-1)).to(hz.dtype)
        loss = loss + 0.5 * (m4 * s * s).sum()
        g = g.clone()
        g[:, :4 * ng] += (m4 * s)[:, :, None].expand(B, ng, 4).reshape(B, 4 * ng)
    return loss, g * nstd


def pitch_loss(cls, reg, tgt, spk, id2mean, id2std, pad):
    """PitchLoss: 100 * masked BCE-with-logits(cls, tgt != 0) + masked, voiced-only L1 between de-normalised values.
    Returns (loss, d/d cls, d/d reg, d): d = the signed L1 argument, whose sign is the one decision of this stage."""
    mask, voiced = tgt != pad, tgt != 0
    y = voiced.to(cls.dtype)
    bce = cls.clamp(min=0) - cls * y + torch.log1p(torch.exp(-cls.abs()))
    mean, sd = id2mean[spk][:, None], id2std[spk][:, None]
    d = (mean + sd * reg) - (mean + sd * tgt)
    mv = (mask & voiced).to(cls.dtype)
    loss = 100 * (mask.to(cls.dtype) * bce).sum() + (mv * d.abs()).sum()
    return loss, 100 * mask.to(cls.dtype) * (torch.sigmoid(cls) - y), mv * sd * torch.sign(d), d


def wgrad(dz, a_in, k):
    """dw[co][ci][j] = sum_{b,t} dz[b][co][t] * a_in[b][ci][t + j - pad],  db[co] = sum_{b,t} dz[b][co][t]"""
    B, Co, L = dz.shape
    pad = (k - 1) // 2
    ap = F.pad(a_in, (pad, pad))
    dzf = dz.permute(1, 0, 2).reshape(Co, B * L)
    dw = torch.stack([dzf @ ap[:, :, j:j + L].permute(1, 0, 2).reshape(-1, B * L).t() for j in range(k)], dim=-1)
    return dw, dz.sum(dim=(0, 2))


def bwd_data(dz, w):
    """gradient w.r.t. the conv's input: the same 'same' conv with W transposed and its taps flipped"""
    return F.conv1d(dz, w.transpose(0, 1).flip(2), padding=(w.shape[2] - 1) // 2)


def leaky_bwd(da, a, leaky):
    return torch.where(a > 0, da, da * SLOPE) if leaky else da  # the engine's rule: !(a > 0) -> slope


def bn_bwd_reduce(da, a, z, mean, invstd, leaky):
    """(dgamma, dbeta) = (sum dy * xhat, sum dy), dy = da * leaky'(a)"""
    dy = leaky_bwd(da, a, leaky)
    xh = (z - mean[None, :, None]) * invstd[None, :, None]
    return (dy * xh).sum(dim=(0, 2)), dy.sum(dim=(0, 2))


def bn_bwd_apply(da, a, z, mean, invstd, gamma, dgamma, dbeta, leaky):
    """dz = gamma * invstd * (dy - dbeta / N - xhat * dgamma / N)  (no BatchNorm: dz = dy)"""
    dy = leaky_bwd(da, a, leaky)
    if mean is None:
        return dy
    n = z.shape[0] * z.shape[2]
    c = lambda v: v[None, :, None]
    xh = (z - c(mean)) * c(invstd)
    return c(gamma) * c(invstd) * (dy - c(dbeta) / n - xh * c(dgamma) / n)


def emb_grads(dx0, seq, spk, keep, pe_mult, n_tok, n_spk, spk_pad_row):
    """token / speaker embedding gradients; the padding rows (last token row; last speaker row of the pitch models)
    stay exactly zero"""
    B, L = seq.shape
    g = dx0[:, :E].permute(0, 2, 1) * keep[:, :, None]
    dtok = torch.zeros(n_tok, E, dtype=dx0.dtype).index_add_(0, seq.reshape(-1), g.reshape(B * L, E))
    dtok[n_tok - 1] = 0
    gs = dx0[:, E:].permute(0, 2, 1)
    if pe_mult is not None:
        gs = gs * pe_mult
    dspk = torch.zeros(n_spk, E, dtype=dx0.dtype).index_add_(0, spk, gs.sum(1))
    if spk_pad_row:
        dspk[n_spk - 1] = 0
    return dtok, dspk


def adam(p, g, m, v, step, lr, eps=1e-8):
    """torch.optim.Adam (amsgrad False, weight_decay 0); step = 1 for the first update.  Returns (p, m, v) after."""
    m = m + (1 - ADAM_B1) * (g - m)
    v = ADAM_B2 * v + (1 - ADAM_B2) * g * g
    denom = v.sqrt() / (1 - ADAM_B2 ** step) ** 0.5 + eps
    return p - (lr / (1 - ADAM_B1 ** step)) * (m / denom), m, v


# ---------------------------------------------------------------------------------------------------------
# one step, stage by stage
# ---------------------------------------------------------------------------------------------------------
def run(kind, sd, opt, batch, hp, dtype, taps=None, forward_only=False):
    """sd: state dict BEFORE the step; opt: {'m': {..}, 'v': {..}, 'step': steps already taken}; batch: seq [B,L],
    spk [B] or [B,1], tgt, keep, pe_mult (or None); hp: lr, pad, norm=(mean, std), stats=(id2mean, id2std), eps.
    Returns (out, aux): out as described in the module docstring; aux['pitch/d'], aux['pitch/scale'] for the one
    capped exclusion of the pitch loss (|d| below 8 * 2^-24 * scale: the sign of d is not decided in fp32)."""
    ls = layers(kind)
    out, aux = {}, {}
    T = lambda x: x.to(dtype)
    src = lambda key: T(taps[key] if taps is not None else out[key])
    P = lambda key: T(sd[key])
    seq, spk = batch["seq"].long(), batch["spk"].long().reshape(-1)
    tgt, keep = T(batch["tgt"]), T(batch["keep"])
    pm = T(batch["pe_mult"]) if kind == "new" and batch.get("pe_mult") is not None else None
    tok, spe = P("token_emb.weight"), P("spk_emb.weight")
    name = lambda i: ls[i]["conv"]
    inp = lambda l: src("x0") if l["inp"] < 0 else src(name(l["inp"]) + "/a")

    # ---- forward ----
    out["x0"] = embed(seq, spk, keep, pm, tok, spe, P("pe.pe") if kind == "new" else None)
    for l in ls:
        n, bn = l["conv"], l["bn"]
        out[n + "/z"] = conv_fwd(inp(l), P(n + ".weight"), P(n + ".bias"))
        if l["cout"] == 1:
            continue
        if bn:
            out[n + "/mean"], out[n + "/invstd"], out[f"after/{bn}.running_mean"], out[f"after/{bn}.running_var"] = \
                bn_stats(src(n + "/z"), P(bn + ".running_mean"), P(bn + ".running_var"))
            out[n + "/a"] = act(src(n + "/z"), src(n + "/mean"), src(n + "/invstd"), P(bn + ".weight"), P(bn + ".bias"),
                                l["leaky"])
        else:
            out[n + "/a"] = act(src(n + "/z"), None, None, None, None, l["leaky"])
    # ---- loss ----
    if kind == "len":
        out["loss"], out["cnn2/dz"] = len_loss(src("cnn2/z"), tgt, hp["pad"], hp["norm"][0], hp["norm"][1])
    else:
        id2mean, id2std = T(hp["stats"][0]), T(hp["stats"][1])
        out["loss"], out["cnn_class2/dz"], out["cnn_reg2/dz"], aux["pitch/d"] = \
            pitch_loss(src("cnn_class2/z"), src("cnn_reg2/z"), tgt, spk, id2mean, id2std, hp["pad"])
        aux["pitch/scale"] = (id2mean[spk][:, None].abs() + (id2std[spk][:, None] * tgt).abs())
        aux["pitch/voiced"] = (tgt != hp["pad"]) & (tgt != 0)
    if forward_only:
        return out, aux
    # ---- backward ----
    def sent_back(j):  # what layer j sends to the layer (or embedding) that feeds it
        dz = src(name(j) + "/dz")
        return bwd_data(dz[:, None] if ls[j]["cout"] == 1 else dz, P(name(j) + ".weight"))

    for i in reversed(range(len(ls))):
        l, n, bn = ls[i], ls[i]["conv"], ls[i]["bn"]
        if l["cout"] > 1:
            users = [j for j in range(len(ls)) if ls[j]["inp"] == i]
            da = None
            for j in reversed(users):  # the engine's order: the later layer stores, the earlier one adds
                da = sent_back(j) if da is None else da + sent_back(j)
            out[n + "/da"] = da
            a, z = src(n + "/a"), src(n + "/z")
            if bn:
                mean, invstd = src(n + "/mean"), src(n + "/invstd")
                out[f"grad/{bn}.weight"], out[f"grad/{bn}.bias"] = bn_bwd_reduce(src(n + "/da"), a, z, mean, invstd, l["leaky"])
                out[n + "/dz"] = bn_bwd_apply(src(n + "/da"), a, z, mean, invstd, P(bn + ".weight"),
                                              src(f"grad/{bn}.weight"), src(f"grad/{bn}.bias"), l["leaky"])
            else:
                out[n + "/dz"] = bn_bwd_apply(src(n + "/da"), a, z, None, None, None, None, None, l["leaky"])
        dz = src(n + "/dz")
        dw, db = wgrad(dz[:, None] if l["cout"] == 1 else dz, inp(l), l["k"])
        out[f"grad/{n}.weight"], out[f"grad/{n}.bias"] = dw, db
    out["dx0"] = sent_back(0)
    out["grad/token_emb.weight"], out["grad/spk_emb.weight"] = \
        emb_grads(src("dx0"), seq, spk, keep, pm, tok.shape[0], spe.shape[0], kind != "len")
    # ---- Adam ----
    for k in trainable_keys(kind):
        out["after/" + k], out["m/" + k], out["v/" + k] = \
            adam(P(k), src("grad/" + k), T(opt["m"][k]), T(opt["v"][k]), opt["step"] + 1, hp["lr"], hp.get("eps", 1e-8))
    return out, aux


# ---------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------
EPS32 = 2.0 ** -24


def channel_axis(key, ndim):
    """activations [B, C, L]: per channel; weights / embeddings and their Adam state [rows, ...]: per row; else none"""
    if ndim == 3 and "/" in key and key.split("/")[0] not in ("grad", "after", "m", "v"):
        return 1
    if ndim == 3 and key in ("x0", "dx0"):
        return 1
    if ndim >= 2 and key.split("/")[0] in ("grad", "after", "m", "v"):
        return 0
    return None


def compare(key, y, r64, r32, skip=None):
    """e_gpu = rms(y - r64), e_cpu = rms(r32 - r64) over the whole tensor; ratio = e_gpu / max(e_cpu, 2^-24 rms(r64)).
    Per channel / weight row: worst relative error, the channel's reference RMS floored at 1e-3 of the tensor's;
    ch_ratio = worst(y) / max(worst(r32), 2^-24).  skip: boolean mask of elements left out (pitch loss only)."""
    y, r64, r32 = y.double(), r64.double(), r32.double()
    assert y.shape == r64.shape == r32.shape, (key, y.shape, r64.shape, r32.shape)
    finite = bool(torch.isfinite(y).all())
    eg, ec = y - r64, r32 - r64
    if skip is not None:
        keepm = (~skip).double()
        eg, ec, r64 = eg * keepm, ec * keepm, r64 * keepm
    n = max(r64.numel() - (int(skip.sum()) if skip is not None else 0), 1)
    rms = lambda t: float((t.pow(2).sum() / n).sqrt())
    e_gpu, e_cpu, ref = rms(eg), rms(ec), rms(r64)
    den = max(e_cpu, EPS32 * ref)
    m = dict(key=key, finite=finite, e_gpu=e_gpu, e_cpu=e_cpu, ref=ref,
             ratio=(e_gpu / den if den > 0 else (0.0 if e_gpu == 0 else float("inf"))), ch_ratio=0.0)
    ax = channel_axis(key, r64.dim())
    if ax is not None and ref > 0 and skip is None:
        dims = [d for d in range(r64.dim()) if d != ax]
        ch = lambda t: t.pow(2).mean(dim=dims).sqrt()
        ch_ref = ch(r64).clamp(min=1e-3 * ref)
        w_gpu, w_cpu = float((ch(eg) / ch_ref).max()), float((ch(ec) / ch_ref).max())
        m["ch_ratio"] = w_gpu / max(w_cpu, EPS32)
    return m
