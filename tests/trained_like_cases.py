"""Shared by the trained-like tests (tests/test_gpu_trained_like.py, tests/pair_harness.py and through it test_gpu_pairs_*.py; not a
test module): the bars, the adversarial rows (input (b) of tests/test_gpu_trained_like.py), the e_rms / e_ch / leak accumulator, the
check of one layer against the bars, the form the default plan runs a conv in, and the `tl` module fixture."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

DEV = "cuda:0"
U = 2.0 ** -24
SLOPE = 0.1
STAGES = (256, 128, 64, 32, 16)
KS = (3, 7, 11)
DILS = (1, 3, 5)
BURST_STEP = 211  # burst starts advance by a prime: their residues cover every tile width x dilation (widths 2..6, d 1..5)
BURST_LEN = 37

# bars: ceilings, tightened to ~2x of the measured worst case where that is below them (profiles/trained_like_error.md)
DIRECT_VS_CPU = 4.0    # direct GPU kernel e_rms <= this x CPU fp32 F.conv1d's (measured <= 2.96 over (a) + (b))
TD_RMS = 3.0           # the plan's transform-domain e_rms <= this x the direct GPU kernel's, same input (measured <= 2.98)
TD_CH = 10.0           # transform-domain e_ch <= this x the direct GPU kernel's (measured <= 5.03)
LEAK = 4.0             # transform-domain leak <= this (ceiling 64; measured <= 1.79, a wrong tile or halo: ~1e5)
GUARD_FACTOR = 3.0     # fp32 guard: error vs float64 <= max(FP32_GUARD_RMS, this x the fp32 oracle's own)


@pytest.fixture(scope="module")
def tl():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pair_harness as ph  # (it imports this module)
    return ph.tl_context()  # (one per process, shared with the files that import this fixture)


# ------------------------------------------------------------------------------------------------------------------------
# inputs (b) and metrics
# ------------------------------------------------------------------------------------------------------------------------
def _adversarial_rows(tap, tiles, seed):
    """tap [C, n] fp32 -> list of (row [C, len] fp32, loud mask [len] bool or None); tiles: the tile widths x dilation in use"""
    rs = np.random.RandomState(seed)
    C, n = tap.shape
    ch_rms = tap.double().pow(2).mean(1).sqrt().float()
    rows = []
    # bursts of the tap's own columns after exact silence; start (and end) residues cover every offset modulo each tile
    nb = max(tiles)
    r = torch.zeros(C, 64 + nb * BURST_STEP)
    loud = np.zeros(r.shape[1], bool)
    for i in range(nb):
        s = 64 + i * BURST_STEP
        c0 = rs.randint(0, max(1, n - BURST_LEN))
        seg = tap[:, c0:c0 + BURST_LEN]
        r[:, s:s + seg.shape[1]] = seg
        loud[s:s + seg.shape[1]] = True
    rows.append((r, loud))
    # isolated spikes at 100x each channel's RMS on a random third of the channels, on silence
    r = torch.zeros(C, 64 + 16 * BURST_STEP)
    loud = np.zeros(r.shape[1], bool)
    for i in range(16):
        s = 64 + i * BURST_STEP + rs.randint(0, 7)
        chans = rs.choice(C, max(1, C // 3), replace=False)
        r[chans, s] = 100.0 * ch_rms[chans] * torch.from_numpy(rs.choice([-1.0, 1.0], len(chans))).float()
        loud[s] = True
    rows.append((r, loud))
    # ragged lengths on the tap's columns: 1, tile +- 1, the work tiles of the kernels (300..512 outputs) +- 1, long
    lens = {1, 315, 316, 383, 384, 385, 499, 500, 501, 509, n}
    for t in tiles:
        lens |= {t - 1, t, t + 1, 2 * t + 1}
    for ln in sorted(lens):
        c0 = rs.randint(0, max(1, n - ln + 1))
        seg = tap[:, c0:c0 + ln]
        if seg.shape[1] < ln:  # (the tap is shorter: wrap around)
            seg = tap[:, np.arange(c0, c0 + ln) % n]
        rows.append((seg.clone(), None))
    return rows


def _batch(rows):
    L = max(r.shape[1] for r, _ in rows)
    L = (L + 3) // 4 * 4
    x = torch.zeros(len(rows), rows[0][0].shape[0], L)
    for i, (r, _) in enumerate(rows):
        x[i, :, :r.shape[1]] = r
    return x, [r.shape[1] for r, _ in rows]


def _quiet(loud, pad):
    """outputs whose receptive field [t - pad, t + pad] holds no loud sample"""
    c = np.concatenate([[0], np.cumsum(loud)])
    n = len(loud)
    t = np.arange(n)
    return (c[np.minimum(t + pad + 1, n)] - c[np.maximum(t - pad, 0)]) == 0


class _Acc:
    """e_rms / e_ch accumulated over rows; leak over the rows with a loud mask"""

    def __init__(self, C):
        self.e2 = torch.zeros(C, dtype=torch.float64)
        self.r2 = torch.zeros(C, dtype=torch.float64)
        self.n = 0
        self.leak = 0.0

    def add(self, y, ref, loud=None, pad=0, unit=None):
        e = y.double() - ref
        self.e2 += e.pow(2).sum(1)
        self.r2 += ref.pow(2).sum(1)
        self.n += ref.shape[1]
        if loud is not None:
            q = torch.from_numpy(_quiet(loud, pad))
            if q.any():
                self.leak = max(self.leak, float((e[:, q].abs() / unit[:, None]).max()))

    def metrics(self):
        layer = float((self.r2.sum() / (self.n * len(self.r2))).sqrt())
        ch_ref = (self.r2 / self.n).sqrt().clamp(min=1e-3 * layer)
        return dict(e_rms=float((self.e2.sum() / (self.n * len(self.e2))).sqrt()),
                    e_ch=float(((self.e2 / self.n).sqrt() / ch_ref).max()), leak=self.leak, rms=layer, n=self.n)


def _report(name, form, ma, mb, ratios=""):
    print(f"TL {name:24s} {form:8s} (a) e_rms {ma['e_rms']:.3e} e_ch {ma['e_ch']:.3e} | (b) e_rms {mb['e_rms']:.3e} "
          f"e_ch {mb['e_ch']:.3e} leak {mb['leak']:.3g} {ratios}")


def _check(name, forms, res, plan_form):
    """the bars of one layer; returns the broken ones (every layer and form is measured before a test fails).  plan_form: the
    form the default plan runs this layer in -- a transform-domain form above TD_RMS x the direct kernel's e_rms must not be it
    (gen_plan.hip falls back to a safer form there); the e_ch and leak bars hold for every form"""
    bad = []
    (ca, cb), (da, db) = res["cpu"], res["direct"]
    _report(name, "cpu-fp32", ca, cb)
    # the direct kernel against CPU fp32 over all valid outputs of the layer's inputs, (a) and (b) together
    e_dir = ((da["e_rms"] ** 2 * da["n"] + db["e_rms"] ** 2 * db["n"]) / (da["n"] + db["n"])) ** 0.5
    e_cpu = ((ca["e_rms"] ** 2 * ca["n"] + cb["e_rms"] ** 2 * cb["n"]) / (ca["n"] + cb["n"])) ** 0.5
    _report(name, "direct", da, db, f"direct/cpu {da['e_rms'] / ca['e_rms']:.2f} {db['e_rms'] / cb['e_rms']:.2f} "
                                    f"all {e_dir / e_cpu:.2f}")
    if e_dir > DIRECT_VS_CPU * e_cpu:
        bad.append((name, "direct", "e_rms vs CPU fp32", e_dir / e_cpu))
    for form in forms[1:]:
        fa, fb = res[form]
        ra, rb = fa["e_rms"] / da["e_rms"], fb["e_rms"] / db["e_rms"]
        ha, hb = fa["e_ch"] / da["e_ch"], fb["e_ch"] / db["e_ch"]
        tag = " [plan]" if form == plan_form else ""
        _report(name, form, fa, fb, f"x direct: e_rms {ra:.2f} {rb:.2f} e_ch {ha:.2f} {hb:.2f}{tag}")
        if max(ra, rb) > TD_RMS and form == plan_form:
            bad.append((name, form, "e_rms x direct", ra, rb))
        if max(ha, hb) > TD_CH:
            bad.append((name, form, "e_ch x direct", ha, hb))
        if fb["leak"] > LEAK:
            bad.append((name, form, "leak", fb["leak"]))
    return bad


def _plan_conv_form(lib, C, k, d):
    """gen_plan.hip td_conv_form under the current option defaults (the ResBlock convs of the C >= 64 stages)"""
    opt = {}
    for key in ("wino", "wino8", "wino8_mask", "wino8_r4", "wino8_r4_mask"):
        v = ctypes.c_int(0)
        assert lib.dissc_get_option(key.encode(), ctypes.byref(v)) == 0
        opt[key] = v.value
    if not opt["wino"]:
        return "direct"
    bit = 9 * (2 if C >= 256 else 1 if C >= 128 else 0) + 3 * KS.index(k) + DILS.index(d)
    if not opt["wino8"] or not (opt["wino8_mask"] >> bit) & 1 or not (k in (7, 11) or (C == 64 and d == 1)):
        return "F(4,3)"
    return "F(5,4)" if opt["wino8_r4"] and k in (7, 11) and (opt["wino8_r4_mask"] >> bit) & 1 else "F(6,3)"


def _ref_pair(x, w1, b1, w2, b2, k, d, dtype):
    x = x.to(dtype)[None]
    t = F.conv1d(F.leaky_relu(x, SLOPE), w1.to(dtype), b1.to(dtype), padding=(k - 1) * d // 2, dilation=d)
    return (x + F.conv1d(F.leaky_relu(t, SLOPE), w2.to(dtype), b2.to(dtype), padding=(k - 1) // 2))[0]
