"""Shared by tests/test_predictor_cases_cpu.py and tests/test_gpu_predictors_tiles.py (not a test module): the inference
predictors restated in one dtype argument, their state dicts (iid, trained-like, and the two derived pitch dicts that expose
what (cls > 0) * reg hides), the tile-edge rows, the edge mask, the bars and the decision rule.  No GPU, no fixture.

  forward            LenPredictor.forward / PitchPredictor(.Base).infer_freq, the structure of oracle/predictors_ref.py, in
                     float32 or float64 (the float32 state dict promoted; BatchNorm stays F.batch_norm), returning the parts
  state_dict         "iid" = synthdata's own; "trained_like" = BatchNorm statistics as training leaves them (below)
  reg_exposed / cls_exposed
  rows / batch       one row per length of EDGE (pitch: + 850), token ids beyond a row's length 10**9
  edge_mask          frames within 12 of a multiple of 64 or of the row's end
  reference / measure / violations
                     the bar e_gpu <= K max(e_torch_fp32, 2^-24 rms(ref64)) over (a) all frames, (b) the worst utterance,
                     (c) the edge frames, and the rule that says where a voiced / unvoiced disagreement is legitimate
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import synthdata as synth

KINDS = ("len", "new", "base")
WEIGHTS = ("iid", "trained_like")
N_TOKENS, N_SPEAKERS = 100, 108
EPS32 = 2.0 ** -24
NEVER_READ = 10 ** 9  # the token id beyond a row's length

TRUNK = {"len": ["cnn1"] + [f"cnn1{i}" for i in range(1, 7)],
         "new": ["cnn1"] + [f"cnn1{i}" for i in range(1, 8)] + ["cnn2"],
         "base": ["cnn1"] + [f"cnn1{i}" for i in range(1, 8)] + ["cnn2"]}
BN = {"len": {"cnn1": "bn1", **{f"cnn1{i}": f"bn1{i}" for i in range(1, 7)}},
      "new": {"cnn2": "bn2"},
      "base": {"cnn1": "bn1", **{f"cnn1{i}": f"bn1{i}" for i in range(1, 8)}, "cnn_class1": "bn_c1", "cnn_reg1": "bn_r1"}}

# the tile widths of the direct convs are 64 / 128 / 256 columns, the embed and head kernels run 128-thread blocks
EDGE = [0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 385, 511, 513]
T_PE = 850           # the last row of pe.pe ("new"); run by both pitch variants
REACH = 12           # receptive half-width of the deepest stack (11 layers of k = 3), plus one

# ---- the bars -----------------------------------------------------------------------------------------------------------
# e_gpu <= K * max(e_torch_fp32, 2^-24 rms(ref64)), e_* = rms error against float64, K = 4: the rule of this conv family
# (tests/train_stage_cases.py).  An exception is granted per (kind, weight set, bar) only, at 2 x the measured worst ratio
# rounded up and never above K_CAP = min(32, max(4, sqrt(384))): one output of a 128-channel k = 3 layer is one fp32 chain
# of 384 products.
K = 4.0
K_CAP = 19.0
BAND = 8.0           # a voiced / unvoiced disagreement is allowed where |cls64| <= BAND * max_t |cls32 - cls64| of the utterance
EXCLUDED_CAP = 0.002  # ... and such frames are at most this share of a case's valid frames

LEN_NORM = (torch.tensor(2.6), torch.tensor(1.7))     # synthdata's
LEN_NORM_2 = (torch.tensor(3.3), torch.tensor(2.1))   # the pair a live handle is switched to


def pitch_stats():
    rs = np.random.RandomState(7)
    return (torch.from_numpy(rs.uniform(90, 250, N_SPEAKERS).astype(np.float32)),
            torch.from_numpy(rs.uniform(15, 50, N_SPEAKERS).astype(np.float32)))


# ---- the restatement ----------------------------------------------------------------------------------------------------
def promote(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def _bn_eval(x, sd, name, eps=1e-5):
    return F.batch_norm(x, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"], sd[name + ".bias"],
                        False, 0.0, eps)


def _embed(kind, sd, seq, spk):
    T = seq.shape[-1]
    emb_seq = F.embedding(seq, sd["token_emb.weight"])
    emb_spk = F.embedding(spk, sd["spk_emb.weight"]).repeat_interleave(T, dim=1)
    if kind == "new":
        emb_spk = emb_spk + sd["pe.pe"][:, :T]
    return torch.cat([emb_seq, emb_spk], dim=-1).transpose(1, 2)


@torch.no_grad()
def forward(kind, sd, seq, spk, dtype=torch.float32, len_norm=LEN_NORM, norm=True, stats=None, trunk=None, hook=None,
            skip_bn=(), skip_len_norm=False):
    """One utterance: seq int [T], spk int -> dict(h = the trunk's output [1, 128, T], lens [T]) for "len",
    dict(h, cls, reg, out) for the pitch kinds, in `dtype`.  trunk: a cached h of the same (kind, weights, row, dtype), so
    that dicts which differ in their heads alone share it.  The rest is for the seeded defects of the CPU test:
    hook(name, x_in, y) replaces a conv's output, skip_bn names BatchNorm layers left out, skip_len_norm the length head's
    * std + mean."""
    sd = promote(sd, dtype)
    seq = torch.as_tensor(seq).long().view(1, -1)
    spk = torch.as_tensor(spk).long().view(1, 1)

    def conv(x, name, pad, bn=True):
        y = F.conv1d(x, sd[name + ".weight"], sd[name + ".bias"], padding=pad)
        if hook is not None:
            y = hook(name, x, y)
        if bn and name in BN[kind] and BN[kind][name] not in skip_bn:
            y = _bn_eval(y, sd, BN[kind][name])
        return y

    if trunk is None:
        x = _embed(kind, sd, seq, spk)
        for n in TRUNK[kind]:
            x = F.leaky_relu(conv(x, n, 1))
    else:
        x = trunk.to(dtype)
    if kind == "len":
        y = conv(x, "cnn2", 1).squeeze(1)
        if not skip_len_norm:
            y = y * len_norm[1].to(dtype) + len_norm[0].to(dtype)
        return dict(h=x, lens=y[0])
    c = conv(x, "cnn_class1", 1)
    r = conv(x, "cnn_reg1", 1)
    cls = conv(F.leaky_relu(c), "cnn_class2", 0).squeeze(1)
    reg = conv(F.leaky_relu(r), "cnn_reg2", 0).squeeze(1)
    if not norm:
        mean, std = stats
        reg = mean.to(dtype)[spk] + reg * std.to(dtype)[spk]
    return dict(h=x, cls=cls[0], reg=reg[0], out=((cls > 0) * reg)[0])


# ---- rows ---------------------------------------------------------------------------------------------------------------
def _unit_row(rs, n, runs):
    """n units: geometric run lengths of mean 2.5 (synthdata.synth_unit_sequences; frame rate, the pitch predictors' input) or,
    runs = False, no unit twice in a row (dedup'd, the length predictor's input)"""
    seq = np.zeros(n, dtype=np.int64)
    t, prev = 0, -1
    while t < n:
        run = int(rs.geometric(1 / 2.5)) if runs else 1
        c = int(rs.randint(0, N_TOKENS))
        if c == prev:
            c = (c + 1) % N_TOKENS
        seq[t:t + run] = c
        prev = c
        t += run
    return seq


@functools.lru_cache(maxsize=None)
def rows(kind):
    """(lengths, [units of row i], [speaker of row i]): one row per edge length, every row another speaker"""
    lengths = EDGE + ([T_PE] if kind != "len" else [])
    rs = np.random.RandomState(5 + KINDS.index(kind))
    seqs = [_unit_row(rs, n, runs=kind != "len") for n in lengths]
    spk = [int(s) for s in rs.permutation(N_SPEAKERS - 1)[:len(lengths)]]
    return lengths, seqs, spk


def batch(seqs, spk, index):
    """the rows `index` as (seq i64 [B, Tmax] with NEVER_READ beyond each length, spk i64 [B, 1], lengths i32 [B])"""
    n = [len(seqs[i]) for i in index]
    seq = torch.full((len(index), max(max(n), 1)), NEVER_READ, dtype=torch.int64)
    for b, i in enumerate(index):
        seq[b, :n[b]] = torch.from_numpy(seqs[i])
    return seq, torch.tensor([[spk[i]] for i in index], dtype=torch.int64), torch.tensor(n, dtype=torch.int32)


def big_batch_index(kind, B=70, seed=3):
    """B rows out of the edge rows of at most 513 frames: each at least twice, empty rows in between (one of them at index 64,
    where the ragged walk's prefix sum starts its second round), shuffled"""
    lengths, _, _ = rows(kind)
    short = [i for i, n in enumerate(lengths) if n <= 513]
    rs = np.random.RandomState(seed)
    idx = short * 3 + [lengths.index(0)] * (B - 3 * len(short))
    assert len(idx) == B
    idx = [idx[i] for i in rs.permutation(B)]
    j = next(j for j, i in enumerate(idx) if lengths[i] == 0)
    idx[64], idx[j] = idx[j], idx[64]
    for at in (63, 65):  # ... with rows that are not empty on both sides of it
        if lengths[idx[at]] == 0:
            j = next(j for j, i in enumerate(idx) if lengths[i] > 100 and j not in (63, 64, 65))
            idx[at], idx[j] = idx[j], idx[at]
    return idx


def mid_batch_index(kind):
    """the batch that reaches the middle tile of each step list: pitch: the 17 edge rows of at most 385 frames and three of them
    again (B = 20, Tmax = 385: the 256-row head on id 2); "len": every edge row twice and two of them a third time (B = 40,
    Tmax = 513: the 128-row layers on id 2)"""
    lengths, _, _ = rows(kind)
    if kind == "len":
        return list(range(len(lengths))) * 2 + [lengths.index(513), lengths.index(64)]
    short = [i for i, n in enumerate(lengths) if n <= 385]
    return short + [lengths.index(385), lengths.index(0), lengths.index(129)]


def edge_mask(lengths, Tmax):
    """bool [B, Tmax]: the frames of each row within REACH of a multiple of 64 or of the row's end"""
    t = np.arange(Tmax)
    near = (t % 64 < REACH) | (t % 64 >= 64 - REACH)
    m = np.zeros((len(lengths), Tmax), dtype=bool)
    for i, n in enumerate(lengths):
        n = int(n)
        m[i, :n] = near[:n] | (t[:n] >= n - REACH)
    return m


# ---- state dicts --------------------------------------------------------------------------------------------------------
def _iid(kind):
    return synth.synth_len_state_dict(N_TOKENS, N_SPEAKERS) if kind == "len" else synth.synth_pitch_state_dict(kind, N_TOKENS, N_SPEAKERS)


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64).astype(np.float32))


DEAD_MEAN = 0.03  # where a dead channel sits: x * alpha and mean * alpha are then 9.5 gamma each and cancel


def _trained_like(kind, seed=23):
    """BatchNorm as training leaves it, layer by layer on one calibration utterance in float64: running_var log-uniform over
    [1e-4, 10] with about 5 % of the channels at 1e-8 (dead: constant at a non-zero mean), the conv's rows scaled so that the
    channel really has that variance and running_mean is its mean up to a third of a standard deviation; gamma Student-t
    (3 degrees of freedom, x 0.7, clipped at 6), beta uniform in [-3, 3].  cnn12 and cnn15 x 30 (tests/train_stage_cases.harshen):
    behind a BatchNorm the statistics follow (mean x 30, variance x 900), without one (the trunk of "new") the activations
    grow 900-fold up to bn2."""
    rs = np.random.RandomState(seed + KINDS.index(kind))
    sd = {k: v.clone() for k, v in _iid(kind).items()}
    crs = np.random.RandomState(seed)
    seq = torch.from_numpy(_unit_row(crs, 300, runs=kind != "len")).view(1, -1)
    x = _embed(kind, promote(sd, torch.float64), seq, torch.tensor([[5]]))

    def layer(conv, x):
        w, b = sd[conv + ".weight"].double(), sd[conv + ".bias"].double()
        big = 30.0 if conv in ("cnn12", "cnn15") else 1.0
        bn = BN[kind].get(conv)
        if bn is None:
            w = w * big
        else:
            y = F.conv1d(x, w, b, padding=1)
            m, v = y.mean((0, 2)), y.var((0, 2), unbiased=False)
            C = m.numel()
            tau = np.exp(rs.uniform(np.log(1e-4), np.log(10.0), C))
            dead = rs.rand(C) < 0.05
            tau[dead] = 1e-8
            off = torch.from_numpy(np.where(dead, DEAD_MEAN, 0.0))
            s = torch.from_numpy(np.sqrt(tau)) / v.sqrt()
            w, b = w * s[:, None, None] * big, (b * s + off) * big
            mean = (m * s + off + torch.from_numpy(0.3 * np.sqrt(tau) * rs.standard_normal(C))) * big
            sd[bn + ".running_mean"], sd[bn + ".running_var"] = _t(mean), _t(tau * big * big)
            sd[bn + ".weight"] = _t(np.clip(0.7 * rs.standard_t(3, C), -6.0, 6.0))
            sd[bn + ".bias"] = _t(rs.uniform(-3.0, 3.0, C))
        sd[conv + ".weight"], sd[conv + ".bias"] = _t(w), _t(b)
        p = promote(sd, torch.float64)
        y = F.conv1d(x, p[conv + ".weight"], p[conv + ".bias"], padding=1)
        return F.leaky_relu(y if bn is None else _bn_eval(y, p, bn))

    for conv in TRUNK[kind]:
        x = layer(conv, x)
    if kind == "base":
        layer("cnn_class1", x)
        layer("cnn_reg1", x)
    if kind != "len":  # both decisions in every utterance: the class logit's median over four speakers is moved to zero
        cls = torch.cat([forward(kind, sd, seq[0], k, torch.float64)["cls"] for k in (0, 30, 60, 90)])
        sd["cnn_class2.bias"] = _t(sd["cnn_class2.bias"].double() - cls.median())
    return sd


@functools.lru_cache(maxsize=None)
def state_dict(kind, weights):
    return {"iid": _iid, "trained_like": _trained_like}[weights](kind)


def reg_exposed(sd):
    """cls = 1 exactly at every frame: the output is the regression, everywhere"""
    sd = {k: v.clone() for k, v in sd.items()}
    sd["cnn_class2.weight"] = torch.zeros_like(sd["cnn_class2.weight"])
    sd["cnn_class2.bias"] = torch.ones_like(sd["cnn_class2.bias"])
    return sd


def cls_exposed(sd):
    """the regression branch is a copy of the class branch: the output is (cls > 0) * cls = max(cls, 0), continuous through
    zero; rows 0-127 and 128-255 of the stacked head carry the same weights"""
    sd = {k: v.clone() for k, v in sd.items()}
    for src, dst in (("cnn_class1", "cnn_reg1"), ("bn_c1", "bn_r1"), ("cnn_class2", "cnn_reg2")):
        for k in [k for k in sd if k.startswith(src + ".")]:
            sd[dst + k[len(src):]] = sd[k].clone()
    return sd


EXPOSED = {"natural": lambda sd: sd, "reg_exposed": reg_exposed, "cls_exposed": cls_exposed}


# ---- references and bars ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _trunks(kind, weights, dtype):
    _, seqs, spk = rows(kind)
    sd = state_dict(kind, weights)
    return [forward(kind, sd, s, k, dtype)["h"] if len(s) else None for s, k in zip(seqs, spk)]


def reference(kind, weights, exposed="natural", second_norm=False):
    return _reference(kind, weights, exposed, second_norm)


@functools.lru_cache(maxsize=None)
def _reference(kind, weights, exposed, second_norm):
    """per edge row (None for the empty one) the parts in float64 and in float32, as float64 numpy arrays:
    [(parts64, parts32)]; the pitch parts carry `out` (z-scored) and `out_hz` (with pitch_stats()); second_norm: "len" with
    LEN_NORM_2 in place of LEN_NORM"""
    _, seqs, spk = rows(kind)
    sd = EXPOSED[exposed](state_dict(kind, weights))
    res = []
    for i, (s, k) in enumerate(zip(seqs, spk)):
        if len(s) == 0:
            res.append(None)
            continue
        both = []
        for dtype in (torch.float64, torch.float32):
            h = _trunks(kind, weights, dtype)[i]
            p = forward(kind, sd, s, k, dtype, trunk=h, len_norm=LEN_NORM_2 if second_norm else LEN_NORM)
            if kind != "len":
                p["out_hz"] = forward(kind, sd, s, k, dtype, trunk=h, norm=False, stats=pitch_stats())["out"]
            both.append({key: v.double().numpy() for key, v in p.items() if key != "h"})
        res.append(tuple(both))
    return res


def _rms(x):
    return float(np.sqrt(np.mean(np.square(x)))) if x.size else 0.0


def _ratio(got, r64, r32):
    e_gpu, e_cpu = _rms(got - r64), _rms(r32 - r64)
    den = max(e_cpu, EPS32 * _rms(r64))
    return (e_gpu / den if den > 0 else (0.0 if e_gpu == 0 else float("inf"))), e_gpu, e_cpu


def band_frames(p64, p32):
    """the frames of one utterance where fp32 cannot decide the sign of the class logit: |cls64| <= BAND max_t |cls32 - cls64|.
    Torch's fp32 evaluation sets the scale, never the kernel."""
    return np.abs(p64["cls"]) <= BAND * np.max(np.abs(p32["cls"] - p64["cls"]))


def measure(got, ref, key, lengths, natural_pitch=False, frames=None):
    """got: [B, Tmax] array, row b against ref[b] = (parts64, parts32) or None; key: the part compared ("lens", "out",
    "out_hz"; for the exposed dicts the target may be given as a function of the parts).  natural_pitch: apply the decision
    rule -- the band frames are left out, a disagreement with float64 outside them is counted in `flips_outside`.
    frames: bool [B, Tmax], restricts everything to those frames.  Returns dict(a, b, c = the three ratios, e_gpu, e_cpu (of
    (a)), valid, excluded, excluded_cpu_flips, flips_inside, flips_outside, finite, worst_row)."""
    pick = key if callable(key) else (lambda p: p[key])
    Tmax = got.shape[1]
    edge = edge_mask(lengths, Tmax)
    G, R64, R32, E, per_row = [], [], [], [], []
    m = dict(valid=0, excluded=0, excluded_cpu_flips=0, flips_inside=0, flips_outside=0, finite=bool(np.isfinite(got).all()))
    for b, n in enumerate(lengths):
        n = int(n)
        if n == 0:
            continue
        p64, p32 = ref[b]
        keep = np.ones(n, dtype=bool) if frames is None else frames[b, :n].copy()
        g, r64, r32 = got[b, :n].astype(np.float64), pick(p64), pick(p32)
        m["valid"] += int(keep.sum())
        if natural_pitch:
            band = band_frames(p64, p32)
            flip = (g != 0) != (p64["cls"] > 0)
            m["excluded"] += int((band & keep).sum())
            m["excluded_cpu_flips"] += int((band & keep & ((p32["cls"] > 0) != (p64["cls"] > 0))).sum())
            m["flips_inside"] += int((flip & band & keep).sum())
            m["flips_outside"] += int((flip & ~band & keep).sum())
            keep &= ~band
        if not keep.any():
            continue
        G.append(g[keep]); R64.append(r64[keep]); R32.append(r32[keep]); E.append(edge[b, :n][keep])
        per_row.append((_ratio(G[-1], R64[-1], R32[-1])[0], b, n))
    G, R64, R32, E = (np.concatenate(x) for x in (G, R64, R32, E))
    m["a"], m["e_gpu"], m["e_cpu"] = _ratio(G, R64, R32)
    m["b"], m["worst_row"] = max(per_row)[0], max(per_row)[1:]
    m["c"] = _ratio(G[E], R64[E], R32[E])[0]
    m["edge_frames"] = int(E.sum())
    return m


def violations(m, k=(K, K, K)):
    """the broken conditions of one measured case, [] = pass; k = the bars of (a), (b), (c)"""
    bad = []
    if not m["finite"]:
        bad.append("not finite")
    for what, kk in zip("abc", k):
        assert kk <= K_CAP, ("a bar above the cap", what, kk)
        if not m[what] <= kk:
            bad.append((f"bar ({what})", m[what], kk))
    if m["flips_outside"]:
        bad.append(("voiced / unvoiced decisions differ from float64 where fp32 can decide", m["flips_outside"]))
    if m["excluded"] > EXCLUDED_CAP * m["valid"]:
        bad.append(("excluded frames above the cap", m["excluded"], EXCLUDED_CAP * m["valid"]))
    return bad


def line(tag, m):
    return (f"PE {tag:44s} a {m['a']:6.3f} b {m['b']:6.3f} (row {m['worst_row'][0]}, T {m['worst_row'][1]}) c {m['c']:6.3f} | "
            f"e_gpu {m['e_gpu']:.3e} e_cpu {m['e_cpu']:.3e} | frames {m['valid']} edge {m['edge_frames']} excluded {m['excluded']} "
            f"(torch flips {m['excluded_cpu_flips']}) flips in/out {m['flips_inside']}/{m['flips_outside']}")
