"""Shared by tests/test_train_stages_cpu.py and tests/test_gpu_train_stages.py (not a test module): the batches and
weights of the stage-wise training checks, the bars, and the function that holds one step's stage outputs to them."""
import numpy as np
import torch

from oracle import train_stages_ref as S

PAD = {"len": -1.0, "new": -100.0, "base": -100.0}
MASKING = {"len": 0.2, "new": 0.4, "base": 0.4}
F32 = lambda x: float(np.float32(x))  # the engine takes its scalars as fp32
NORM = (F32(3.3), F32(2.1))
LR = F32(3e-4)

# ---- the bars: e_gpu <= K * max(e_cpu, 2^-24 rms(ref)) per stage output, over the whole tensor (K_WHOLE) and for the
# worst channel / weight row (K_CH).  K is a margin over torch's fp32 CPU evaluation of the same stage on the same
# inputs, never over the engine's own figures: 4 everywhere (the bar the MFMA conv family is held to elsewhere in this
# suite), except where the kernel's summation order legitimately differs from torch's blocked sums; there K = 2 x the
# measured worst ratio rounded up, never above min(32, max(4, sqrt(chain length n))).
# Measured on an MI355X over every shape of tests/test_gpu_train_stages.py (whole tensor / worst channel; the full
# table is profiles/train_stage_error.md):
#   embed 0 / 0 (exact)        conv_fwd 2.86 / 10.69      bn_stats 0.91 / -          act 0.77 / 1.26
#   head_fwd 2.53 / -          loss 1.00                  loss_grad 1.00 / -         head_wgrad 0.76 / 0.56
#   head_bwd_data 0.64 / 1.24  bn_bwd_reduce 0.78 / -     bn_bwd_apply 1.00 / 1.00   wgrad 2.07 / 2.22
#   bias_grad 0.57 / -         bwd_data 2.70 / 3.40       tok_grad 0.73 / 1.09       spk_grad 3.02 / 3.29
#   adam 1.00 / 1.00 (exp_avg_sq: 216 before 1 - beta2 was rounded once from double, see train_adam_kernel)
# The one exception, per channel only: conv_fwd (conv_mfma32_kernel).  Every output element is ONE fp32 chain of
# n = cin * k products in a matrix-core accumulator (384; 192 for cnn1), where torch sums in SIMD-wide blocks.  Its
# whole-tensor error stays inside 4 (2.86); the worst single channel does not: 10.69 for cnn1 (B = 1, L = 1: one
# element per channel), 8.17 for the 128-channel layers (len 1 x 1), 5.58 at the multi-column shapes (the
# BatchNorm-free trunk of "new", whose activations have a non-zero mean, so the partial sums grow along the chain).
#   128-channel layers: 2 x 8.17 -> 17 <= sqrt(384) = 19.6;   cnn1: 2 x 10.69 -> 22, capped at sqrt(192) = 13.9 -> 13
K_WHOLE = 4.0
K_CH = 4.0
K_CH_CONV_FWD = {192: 13.0, 384: 17.0}  # by chain length n = cin * k


def bar(kind, stage, key, what="ratio"):
    if what == "ch_ratio" and stage == "conv_fwd":
        l = {l["conv"]: l for l in S.layers(kind)}[key.split("/")[0]]
        return K_CH_CONV_FWD[l["cin"] * l["k"]]
    return K_CH if what == "ch_ratio" else K_WHOLE


def pitch_stats():
    rs = np.random.RandomState(7)
    return (torch.from_numpy(rs.uniform(90, 250, 108).astype(np.float32)),
            torch.from_numpy(rs.uniform(15, 50, 108).astype(np.float32)))


def make_batch(kind, B, L, seed):
    """a ragged batch: row 0 has the full length, the others end anywhere in [L/4, L]; targets beyond a row's end hold
    the kind's pad value, tokens the pad token.  Pitch targets are continuous (z-scored values, 0 = unvoiced)."""
    rs = np.random.RandomState(seed)
    seq = np.full((B, L), 100, dtype=np.int64)
    tgt = np.full((B, L), PAD[kind], dtype=np.float32)
    for b in range(B):
        n = L if b == 0 else int(rs.randint(max(1, L // 4), L + 1))
        seq[b, :n] = rs.randint(0, 100, size=n)
        if kind == "len":
            tgt[b, :n] = rs.randint(1, 9, size=n)
        else:
            tgt[b, :n] = np.where(rs.rand(n) < 0.65, rs.randn(n), 0.0)
    batch = dict(seq=torch.from_numpy(seq), spk=torch.from_numpy(rs.randint(0, 107, size=(B, 1)).astype(np.int64)),
                 tgt=torch.from_numpy(tgt),
                 keep=torch.from_numpy((rs.rand(B, L) <= 1.0 - MASKING[kind]).astype(np.float32)), pe_mult=None)
    if kind == "new":
        batch["pe_mult"] = torch.from_numpy(((rs.rand(B, L, 32) >= 0.4) / np.float32(0.6)).astype(np.float32))
    return batch


def hyper(kind):
    return dict(lr=LR, pad=PAD[kind], norm=NORM, stats=pitch_stats(), eps=F32(1e-8))


def harshen(kind, sd, seed=11):
    """conv weights of two layers x 30; one BatchNorm layer's gamma log-uniform in [1e-3, 30], beta in [-10, 10]"""
    rs = np.random.RandomState(seed)
    sd = {k: v.clone() for k, v in sd.items()}
    for n in ("cnn12", "cnn15"):
        sd[n + ".weight"] = sd[n + ".weight"] * 30
    bn = "bn2" if kind == "new" else "bn13"
    c = sd[bn + ".weight"].numel()
    sd[bn + ".weight"] = torch.from_numpy(np.exp(rs.uniform(np.log(1e-3), np.log(30), c)).astype(np.float32))
    sd[bn + ".bias"] = torch.from_numpy(rs.uniform(-10, 10, c).astype(np.float32))
    return sd


def stage_of(kind, key):
    ls = {l["conv"]: l for l in S.layers(kind)}
    bns = {l["bn"] for l in ls.values() if l["bn"]}
    feeds_head = {S.layers(kind)[l["inp"]]["conv"] for l in ls.values() if l["cout"] == 1}
    if key in ("x0", "loss"):
        return {"x0": "embed", "loss": "loss"}[key]
    if key == "dx0":
        return "bwd_data"
    head, _, tail = key.partition("/")
    if head in ("after", "m", "v"):
        return "bn_stats" if tail.endswith(("running_mean", "running_var")) else "adam"
    if head == "grad":
        mod, what = tail.rsplit(".", 1)
        if mod in bns:
            return "bn_bwd_reduce"
        if mod == "token_emb":
            return "tok_grad"
        if mod == "spk_emb":
            return "spk_grad"
        if ls[mod]["cout"] == 1:
            return "head_wgrad"
        return "wgrad" if what == "weight" else "bias_grad"
    l = ls[head]
    if l["cout"] == 1:
        return {"z": "head_fwd", "dz": "loss_grad"}[tail]
    if tail in ("mean", "invstd"):
        return "bn_stats"
    if tail == "da":
        return "head_bwd_data" if head in feeds_head else "bwd_data"
    return {"z": "conv_fwd", "a": "act", "dz": "bn_bwd_apply"}[tail]


def pitch_skip(aux64):
    """the capped exclusion of the pitch loss: voiced positions whose |d| in float64 is below 8 * 2^-24 * (|mean| +
    |sd g|), where fp32 cannot decide the sign of d.  Returns (mask, voiced positions, cap)."""
    voiced = aux64["pitch/voiced"]
    skip = voiced & (aux64["pitch/d"].abs() < 8 * S.EPS32 * aux64["pitch/scale"])
    nv = int(voiced.sum())
    return skip, nv, min(50, int(0.002 * nv))


def check_step(kind, Y, R64, R32, aux64, tag, verbose=True):
    """every stage output of one step against the float64 restatement; prints one line per stage (its worst tensor),
    returns the list of violations ((stage, key, what, value, bar) tuples; empty = pass)"""
    bad, worst = [], {}
    assert set(Y) >= set(R64), sorted(set(R64) - set(Y))
    skip = None
    if kind != "len":
        skip, nv, cap = pitch_skip(aux64)
        if int(skip.sum()) > cap:
            bad.append(("loss_grad", "cnn_reg2/dz", "excluded positions", int(skip.sum()), cap))
    for key in R64:
        stage = stage_of(kind, key)
        if key == "loss":
            y, r64, r32 = float(Y[key]), float(R64[key]), float(R32[key])
            den = max(abs(r32 - r64), S.EPS32 * abs(r64))
            m = dict(key=key, finite=bool(np.isfinite(y)), e_gpu=abs(y - r64), e_cpu=abs(r32 - r64), ref=abs(r64),
                     ratio=abs(y - r64) / den if den > 0 else (0.0 if y == r64 else float("inf")), ch_ratio=0.0)
        else:
            m = S.compare(key, Y[key], R64[key], R32[key], skip=skip if key == "cnn_reg2/dz" and kind != "len" else None)
        if not m["finite"]:
            bad.append((stage, key, "not finite", float("inf"), 1.0))
        w = worst.setdefault(stage, {})
        for what in ("ratio", "ch_ratio"):
            k = bar(kind, stage, key, what)
            if not m[what] <= k:
                bad.append((stage, key, what, m[what], k))
            if what not in w or m[what] / k > w[what][0][what] / w[what][1]:
                w[what] = (m, k)
    if verbose:
        for stage, w in worst.items():
            (m, k), (mc, kc) = w["ratio"], w["ch_ratio"]
            print(f"TS {tag:20s} {stage:14s} e_gpu {m['e_gpu']:.3e} e_cpu {m['e_cpu']:.3e} ratio {m['ratio']:6.3f} bar {k:g} "
                  f"({m['key']}) | worst channel {mc['ch_ratio']:6.3f} bar {kc:g} ({mc['key']})")
    return bad, worst
