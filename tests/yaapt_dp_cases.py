"""Constructed inputs for the YAAPT device stages (csrc/yaapt_dp.hip: spec-track and final-track; the candidate logic at
the end of yaapt_nccf_kernel in csrc/yaapt.hip), shared by tests/test_yaapt_dp_cases_cpu.py and tests/test_gpu_yaapt_dp.py
(not a test module).  Three families of cases, each fed to its entry directly:

  spec cases   energy f32 [f], cand_pitch / cand_merit f32 [f, 4], n_tda, median_value   -> YaaptTracker.spec_track
  final cases  en_norm f64 [t], vuv u8 [t], spec f64 [t], spec_std, 2 x (pitch, merit) f32 [t, 3] -> final_track_device
  the NCCF case  rows of a float32 signal with per-frame lag ranges                      -> YaaptTracker.nccf

The references restate nothing: dissc_amd.f0.spectral_track / lag_ranges / merge_candidates / final_track with the
normalisation lines of YaaptTracker._host_stages for the two DP kernels, oracle.yaapt_ref.crs_corr / cmp_rate in float64
on the float32 signal for the NCCF.  `branches(case)` names the branches a case takes, from the reference's own
intermediate values (its medfilt / _viterbi / pchip calls are recorded while it runs); `margins(case)` says whether
float64 numpy and the device can be compared exactly on it (see there).  Everything is seeded RandomState or literal.
"""
import contextlib
import inspect

import numpy as np
from scipy import interpolate as _sp_interp

from dissc_amd import f0 as f0m
from oracle import yaapt_ref as yr

FS = 16000
TDA, HOP, FLEN = 400, 80, 320      # tda_frame_length / frame_space / frame_length in samples at 16 kHz
P = dict(f0m.DEFAULTS)
# yaapt_dp.hip keeps the Viterbi back-pointers in LDS while they fit in kLdsBack = 150 KiB: 4 bytes per frame in the
# spec-track kernel, 8 in the final-track kernel.  The first F that moves each into the global workspace follows.
LDS_BACK = 150 * 1024
F_SPEC_WS = LDS_BACK // 4 + 1      # 38 401
F_FINAL_WS = LDS_BACK // 8 + 1     # 19 201
MEDIANS = (3, 7, 9)


def params(median=7):
    return dict(P, median_value=int(median))


# ---------------------------------------------------------------------------------------------------------------
# recording the reference's intermediate values
# ---------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def traced(mod=f0m):
    """record every medfilt / _viterbi / pchip call that dissc_amd.f0's stages make while the block runs"""
    rec = {"medfilt": [], "viterbi": [], "pchip": []}
    orig = (mod.medfilt, mod._viterbi, mod._interp)

    def med(x, k):
        out = orig[0](x, k)
        rec["medfilt"].append((np.array(x), int(k), np.array(out)))
        return out

    def vit(local, trans):
        path = orig[1](local, trans)
        rec["viterbi"].append((np.array(local), np.array(trans), np.array(path)))
        return path

    class Interp:
        @staticmethod
        def pchip(x, y):
            rec["pchip"].append((np.array(x), np.array(y)))
            return orig[2].pchip(x, y)

    mod.medfilt, mod._viterbi, mod._interp = med, vit, Interp
    try:
        yield rec
    finally:
        mod.medfilt, mod._viterbi, mod._interp = orig


# ---------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------
def spec_reference(case, mod=f0m):
    """what YaaptTracker._host_stages computes for one utterance before the NCCF (its lines, on the case's tables)"""
    p = params(case["median"])
    f, t = case["f"], case["n_tda"]
    en = case["energy"].astype(np.float64)[:f]
    cp, cm = case["cand_pitch"], case["cand_merit"]
    mean = en.mean() if f else 1.0
    en = en / mean if mean > 0 else en
    vuv = en > p["nlfer_thresh1"]
    pit = np.where(vuv[None, :], cp[:f].T, 0.0)
    mer = np.where(vuv[None, :], cm[:f].T, 1.0)
    spec, std = mod.spectral_track(pit, mer, p) if f else (np.zeros(0), 1.0)
    lo, hi = mod.lag_ranges(spec[:t], std, FS, p)
    return {"en_norm": en, "vuv": vuv, "spec": spec, "spec_std": float(std), "lag_min": lo, "lag_max": hi,
            "pit": pit, "mer": mer, "mean": float(mean)}


def final_reference(case, mod=f0m):
    """YaaptTracker._host_stages after the NCCF: merge_candidates + final_track -> f0 float64 [t]"""
    p = params(case["median"])
    t = case["t"]
    if t <= 0:
        return np.zeros(0)
    rp, rm = mod.merge_candidates(case["tp1"][:t].T, case["tm1"][:t].T, case["tp2"][:t].T, case["tm2"][:t].T,
                                  case["spec"], case["spec_std"], case["en_norm"], case["vuv"].astype(bool), p)
    return mod.final_track(rp, rm, case["en_norm"], p)


def nccf_frame_reference(row, fr):
    """oracle crs_corr / cmp_rate in float64 on the float32 samples of frame `fr` -> (phi [TDA], pitch [3], merit [3]).
    A range with lag_max >= TDA has no correlation window: the oracle asserts there, the kernel documents it as skipped
    (phi = 0, no candidate), which is the expectation used."""
    lmin, lmax = (int(v) for v in row["lags"][fr])
    if lmax >= TDA:
        return np.zeros(TDA), np.zeros(3), np.full(3, 0.001)
    x = row["sig"][fr * HOP:fr * HOP + TDA].astype(np.float64)
    phi = yr.crs_corr(x, lmin, lmax)
    pit, mer = yr.cmp_rate(phi, FS, 3, lmin, lmax)
    return phi, pit, mer


def nccf_frames(row):
    """time-domain frames of a row, as yaapt_frames_kernel counts them (capped by the lag table's length)"""
    return min(max(row["ns"] - (TDA - HOP), 0) // HOP, len(row["lags"]))


# ---------------------------------------------------------------------------------------------------------------
# builders: spec-track
# ---------------------------------------------------------------------------------------------------------------
def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def spec_case(name, energy, cp, cm, n_tda=None, median=7, exact_mean1=False):
    energy, cp, cm = _f32(energy).reshape(-1), _f32(cp).reshape(-1, 4), _f32(cm).reshape(-1, 4)
    f = len(energy)
    assert cp.shape == cm.shape == (f, 4)
    return {"kind": "spec", "name": name, "f": f, "n_tda": max(f - 1, 0) if n_tda is None else n_tda, "energy": energy,
            "cand_pitch": cp, "cand_merit": cm, "median": median, "exact_mean1": exact_mean1}


def _padded(values, merit=0.5):
    """SHC rows as the padding rule leaves them when one peak was found: slots 1..3 are copies of slot 0"""
    v = np.asarray(values, dtype=np.float64).reshape(-1, 1)
    return np.repeat(v, 4, axis=1), np.where(v > 0, merit, 1.0) * np.ones((1, 4))


def _on_off(f, voiced_at, hi=2.0, lo=0.125):
    e = np.full(f, lo)
    e[list(voiced_at)] = hi
    return e


def _placed(f, voiced_at, values, **kw):
    """f frames, voiced (high energy, one padded candidate) at `voiced_at` with the given pitches, silence elsewhere"""
    cp, cm = np.zeros((f, 4)), np.ones((f, 4))
    p, m = _padded(values)
    cp[list(voiced_at)], cm[list(voiced_at)] = p, m
    return _on_off(f, voiced_at), cp, cm


def random_spec(name, f, seed, p_voiced=0.15, n_tda=None, median=7, p_pad=0.1):
    """random SHC tables: a frame is loud with probability p_voiced; a frame carries 4 distinct candidates or, with
    probability p_pad, 1..3 and copies of slot 0 in the rest (as the SHC stage pads), a tenth none at all; quiet frames
    carry candidates too.  (A padded copy next to its median-smoothed original makes two paths of exactly equal cost,
    'move now' and 'move one frame later', which rounding decides: margin (b) rejects such draws, so p_pad stays small
    here and the literal cases carry the padded rows.)"""
    rs = np.random.RandomState(seed)
    loud = rs.rand(f) < p_voiced
    energy = np.where(loud, rs.uniform(1.5, 3.0, f), rs.uniform(0.0, 0.2, f)) * 37.0
    centre = 150.0 + 60.0 * np.sin(np.arange(f) / 23.0 + rs.uniform(0, 6))
    cp = np.clip(centre[:, None] * rs.choice([0.5, 1.0, 1.0, 2.0], (f, 4)) + 12.0 * rs.standard_normal((f, 4)), 61, 399)
    cm = np.sort(rs.uniform(0.05, 1.0, (f, 4)), axis=1)[:, ::-1]
    ncand = np.where(rs.rand(f) < p_pad, rs.randint(1, 4, f), 4)
    for k in range(1, 4):
        pad = ncand <= k
        cp[pad, k], cm[pad, k] = cp[pad, 0], cm[pad, 0]
    empty = rs.rand(f) < 0.1
    cp[empty], cm[empty] = 0.0, 1.0
    return spec_case(name, energy, cp, cm, n_tda, median)


def _spec_literals():
    out = []
    z4, o4 = np.zeros((0, 4)), np.ones((0, 4))
    out.append(spec_case("f0", np.zeros(0), z4, o4, n_tda=0))
    out.append(spec_case("zero_energy", np.zeros(6), *_padded([150, 160, 170, 160, 150, 140]), n_tda=5))
    # loud frames without a candidate, candidates only on quiet frames
    cp, cm = _padded([0, 0, 0, 0, 180, 190, 200, 190])
    out.append(spec_case("nv0_quiet_candidates", _on_off(8, range(4)), cp, cm))
    out.append(spec_case("nv0_no_candidates", [3, 1, 4, 1, 5], np.zeros((5, 4)), np.ones((5, 4))))
    # a frame exactly on nlfer_thresh1 (0.75, exactly representable; the mean is exactly 1): `>` leaves it unvoiced
    cp, cm = _padded([200, 210, 220, 230, 220, 210, 200, 190])
    out.append(spec_case("exact_thresh1", [0.75, 1.25, 1.0, 1.0, 0.75, 1.25, 1.5, 0.5], cp, cm, exact_mean1=True))
    out.append(spec_case("nv1_mid", *_placed(5, [2], [222])))
    out.append(spec_case("nv1_first", *_placed(5, [0], [222])))
    out.append(spec_case("f1_nv1", *_placed(1, [0], [222]), n_tda=1))
    out.append(spec_case("f1_nv0", [1.0], np.zeros((1, 4)), np.ones((1, 4)), n_tda=0))
    out.append(spec_case("f2_nv2", *_placed(2, [0, 1], [180, 260]), n_tda=2))
    out.append(spec_case("f2_nv1_last", *_placed(2, [1], [180]), n_tda=1))
    out.append(spec_case("nv2_in_7", *_placed(7, [2, 5], [180, 260])))
    out.append(spec_case("f3_nv3", *_placed(3, [0, 1, 2], [300, 310, 305]), n_tda=3))
    out.append(spec_case("f3_nv3_low", *_placed(3, [0, 1, 2], [90, 95, 92]), n_tda=2))
    out.append(spec_case("f4_nv3", *_placed(4, [0, 1, 3], [130, 140, 135]), n_tda=4))
    out.append(spec_case("f4_nv4", *_placed(4, [0, 1, 2, 3], [240, 230, 220, 210]), n_tda=3))
    out.append(spec_case("nv3_inner", *_placed(9, [2, 3, 6], [170, 180, 175])))
    out.append(spec_case("nv5_falling", *_placed(11, [1, 2, 4, 7, 8], [260, 240, 215, 190, 170])))
    # voiced ends that lie below half the track's mean: plateaus of >= 3 frames survive the 5-point median
    vals = [70] * 3 + [300] * 6 + [72] * 3
    out.append(spec_case("ends_voiced_low", *_placed(12, range(12), vals)))
    # lag clamps at f0_max / f0_min
    out.append(spec_case("clamp_f0_max", *_placed(10, range(10), [390] * 3 + [395] * 4 + [391] * 3)))
    out.append(spec_case("clamp_f0_min", *_placed(10, range(10), [64, 65, 66, 65, 64, 63, 64, 65, 66, 65]), n_tda=10))
    # pchip: knots at the even frames, median_value = 3 (k5 = 1) keeps the values as written.  Left end: secants 5, 50 ->
    # the three-point estimate is negative -> d = 0; interior: a sign change (230, 180, 200), a zero secant (205, 205);
    # right end: secants -50, +5 -> |d| = 32.5 > 3 * 5 -> d = 3 m0
    vals = [100, 110, 210, 230, 180, 200, 205, 205, 300, 200, 210]
    out.append(spec_case("pchip_arms", *_placed(21, range(0, 21, 2), vals), median=3))
    vals = [210, 200, 300, 205, 205, 200, 180, 230, 210, 110, 100]
    out.append(spec_case("pchip_arms_mirrored", *_placed(31, range(0, 31, 3), vals), median=3))
    # two knots with a slope: the Viterbi (std of slot 0 is 0, so transitions are free) takes the pitch-0 candidate of
    # the two middle frames -> track 200, 0, 0, 100 -> knots at the ends only
    cp = np.array([[150, 200, 150, 150], [150, 0, 150, 150], [150, 0, 150, 150], [150, 100, 150, 150]], dtype=np.float64)
    cm = np.tile([0.125, 1.0, 0.125, 0.125], (4, 1))
    out.append(spec_case("nk2_sloped", np.full(4, 2.0), cp, cm, n_tda=4, median=3))
    cp5 = np.vstack([cp[:1], cp[1:3], cp[1:2], cp[3:]])
    out.append(spec_case("nk2_sloped_f5", np.full(5, 2.0), cp5, np.tile([0.125, 1.0, 0.125, 0.125], (5, 1)), median=3))
    # exact tie: the last voiced frame offers 100 and 140 at equal merit after 120, 120 -> first minimum = 100
    cp, cm = np.zeros((6, 4)), np.ones((6, 4))
    cp[1:4] = [[120] * 4, [120] * 4, [100, 140, 100, 140]]
    cm[1:4] = 0.5
    out.append(spec_case("viterbi_tie", _on_off(6, [1, 2, 3]), cp, cm, median=3))
    cp, cm = np.zeros((7, 4)), np.ones((7, 4))
    cp[1:5] = [[120] * 4, [100, 140, 100, 140], [120] * 4, [120] * 4]
    cm[1:5] = 0.5
    out.append(spec_case("viterbi_tie_inner", _on_off(7, [1, 2, 3, 4]), cp, cm, median=3))
    return out


# A builder that misses a margin draws again from the next seed: SEEDS holds the draw each random case settled on
# (`python tests/yaapt_dp_cases.py` prints the table again after a builder changes); the CPU test checks that the
# margins hold for every case as committed.
SEEDS = {'rand_f255': 0, 'rand_f256': 0, 'rand_f257': 0, 'rand_f511': 2, 'rand_f513': 0, 'rand_f300': 1, 'rand_f520': 10,
         'rand_f40': 0, 'rand_f9': 0, 'rand_f6': 0, 'rand_t1': 0, 'rand_t2': 0, 'rand_t3': 0, 'rand_t4': 0, 'rand_t5': 0,
         'rand_t6': 0, 'rand_t7': 0, 'rand_t8': 0, 'rand_t40': 0, 'rand_t255': 0, 'rand_t256': 0, 'rand_t257': 0,
         'rand_t300': 0, 'rand_t520': 1, 'nccf': 0, 'big_f38401': 0, 'big_row1_f300': 0, 'big_t38401': 4,
         'big_row1_t300': 1, 'big_f19201': 0, 'big_t19201': 1}
_FIND = []


def _draw(make, what):
    if not _FIND:
        return make(SEEDS[what])
    for k in range(40):
        case = make(k)
        if margins(case)["ok"]:
            _FIND[0][what] = k
            return case
    raise AssertionError(f"{what}: no seed in 40 holds the margins: {margins(case)['why']}")


def _build_spec_cases():
    out = [c for c in _spec_literals()]
    for c in out:
        m = margins(c)
        assert m["ok"], (c["name"], m["why"])
    seed = 100
    for f, pv in ((255, 0.1), (256, 0.1), (257, 0.1), (511, 0.06), (513, 0.06), (300, 0.6), (520, 0.35), (40, 0.5),
                  (9, 0.7), (6, 0.8)):
        out.append(_draw(lambda k: random_spec(f"rand_f{f}", f, seed + 1000 * k, pv), f"rand_f{f}"))
        seed += 1
    # the rows whose branches involve the median, again under median_value 3 and 9 (k5 = 1 and 7).  Under 9 a voiced
    # run of exactly 3 frames has a 7-point median of zero everywhere (four zeros in every window): the track's mean
    # is then 0 and the lag ranges divide by zero in the reference and in the kernel alike, so nv == 3 is left out there
    for c in list(out):
        if c["median"] != 7 or c["f"] == 0:
            continue
        nv = _nv(c)
        for mv in (3, 9):
            if nv >= (4 if mv == 9 else 3) and (c["f"] <= 40 or c["f"] in (257, 300)):
                v = dict(c, name=f"{c['name']}@m{mv}", median=mv)
                if margins(v)["ok"]:
                    out.append(v)
    return out


def _nv(case):
    r = spec_reference(case)
    return int((r["vuv"] & (case["cand_pitch"][:case["f"], 0] > 0)).sum())


# ---------------------------------------------------------------------------------------------------------------
# builders: final-track
# ---------------------------------------------------------------------------------------------------------------
EMPTY = ([0.0, 0.0, 0.0], [0.001, 0.001, 0.001])   # what the NCCF emits when it finds nothing


def final_case(name, en, vuv, spec, std, c1, c2, median=7):
    """c1 / c2: per frame a (pitch [3], merit [3]) pair for each NCCF pass"""
    t = len(en)
    tp1, tm1 = _f32([c[0] for c in c1]).reshape(t, 3), _f32([c[1] for c in c1]).reshape(t, 3)
    tp2, tm2 = _f32([c[0] for c in c2]).reshape(t, 3), _f32([c[1] for c in c2]).reshape(t, 3)
    return {"kind": "final", "name": name, "t": t, "en_norm": np.asarray(en, dtype=np.float64).reshape(t),
            "vuv": np.asarray(vuv, dtype=np.uint8).reshape(t), "spec": np.asarray(spec, dtype=np.float64).reshape(t),
            "spec_std": float(std), "tp1": tp1, "tm1": tm1, "tp2": tp2, "tm2": tm2, "median": median}


def _one(p, m):
    """a single NCCF candidate: the padding rule copies it into slots 1 and 2"""
    return ([p, p, p], [m, m, m])


def random_final(name, t, seed, median=7, p_loud=0.6):
    """random NCCF tables around a smooth spectral track: each pass gives a frame nothing, one candidate (padded), two or
    three; 15 % of the frames are dead, a fraction p_loud is NLFER-voiced.  (On a voiced frame rows 5 and 6 cost the
    same; when both pitches lie between the track's pitch before and after, the two detours cost exactly the same in
    real arithmetic, |a-b| + |b-c| = |a-c|, and rounding decides: about 3 in 1000 voiced frames.  Margin (b) rejects
    such draws, so the long cases keep p_loud small.)"""
    rs = np.random.RandomState(seed)
    spec = 170.0 + 50.0 * np.sin(np.arange(t) / 31.0 + rs.uniform(0, 6)) + rs.uniform(-3, 3, t)
    std = 12.0
    kind = rs.rand(t)
    en = np.where(kind < 0.15, rs.uniform(0.0, 0.09, t), np.where(kind < 1.0 - p_loud, rs.uniform(0.12, 0.7, t),
                                                                 rs.uniform(0.8, 3.5, t)))
    vuv = en > P["nlfer_thresh1"]

    def cands():
        out = []
        for i in range(t):
            r = rs.rand()
            pit = np.clip(spec[i] * rs.choice([0.5, 1.0, 1.0, 1.0, 2.0], 3) + 2.5 * std * rs.standard_normal(3), 61, 399)
            mer = np.sort(rs.uniform(0.26, 1.0, 3))[::-1]
            if r < 0.25:
                out.append(EMPTY)
            elif r < 0.6:
                out.append(_one(pit[0], mer[0]))
            elif r < 0.8:
                out.append(([pit[0], pit[1], pit[0]], [mer[0], mer[1], mer[0]]))
            else:
                out.append((list(pit), list(mer)))
        return out
    return final_case(name, en, vuv, spec, std, cands(), cands(), median)


def _final_literals():
    out = []
    out.append(final_case("t0", [], [], [], 10.0, [], []))
    # t = 1: equal merits across the passes (140 and 160 around 150) -> the stable sort keeps pass 1 first
    out.append(final_case("t1_tie_pass1_pass2", [1.5], [1], [150.0], 10.0, [_one(140, 0.9)], [_one(160, 0.9)]))
    out.append(final_case("t1_tie_in_pass", [1.5], [1], [150.0], 10.0, [([165, 135, 165], [0.9, 0.9, 0.9])], [EMPTY]))
    out.append(final_case("t1_dead", [0.05], [0], [150.0], 10.0, [_one(150, 0.9)], [_one(150, 0.8)]))
    out.append(final_case("t1_none", [0.5], [0], [150.0], 10.0, [EMPTY], [EMPTY]))
    # en == nlfer_thresh2 exactly (float64 0.1 on both sides) is dead: `<=`.  The loud neighbours make 150 Hz cheap, so
    # a frame that is wrongly alive is tracked
    out.append(final_case("t3_dead_on_thresh2", [1.5, P["nlfer_thresh2"], 1.5], [1, 0, 1], [150.0] * 3, 10.0,
                          [_one(150, 0.9)] * 3, [_one(151, 0.8)] * 3))
    out.append(final_case("t2_voiced", [1.2, 2.4], [1, 1], [200.0, 204.0], 8.0, [_one(199, 0.8), _one(205, 0.9)],
                          [([202, 101, 202], [0.7, 0.5, 0.7]), EMPTY]))
    out.append(final_case("t3_mixed", [1.2, 0.3, 2.6], [1, 0, 1], [200.0, 202.0, 204.0], 8.0,
                          [_one(199, 0.8), EMPTY, _one(205, 0.9)], [EMPTY, _one(230, 0.4), ([203, 101, 203], [0.7, 0.6, 0.7])]))
    # weight 0 at diff == 5 std exactly (200 - 150 = 5 * 10) and beyond it; an all-zero-merit frame keeps its order
    out.append(final_case("weight0", [1.5, 1.6, 1.4, 1.5, 1.6], [1] * 5, [150.0] * 5, 10.0,
                          [_one(200, 0.9), ([149, 200, 260], [0.6, 0.9, 0.95]), _one(100, 0.9), _one(152, 0.5), _one(260, 0.9)],
                          [_one(151, 0.3), EMPTY, _one(210, 0.9), ([300, 148, 300], [0.9, 0.4, 0.9]), _one(90, 0.9)]))
    out.append(final_case("all_dead", [0.01, 0.05, 0.1, 0.0, 0.09, 0.02], [0] * 6, [150.0] * 6, 10.0,
                          [_one(150, 0.9)] * 6, [_one(149, 0.8)] * 6))
    out.append(final_case("all_none", [0.5, 0.6, 2.5, 0.3, 0.2, 1.9, 0.4, 0.5], [0, 0, 1, 0, 0, 1, 0, 0],
                          np.linspace(150, 164, 8), 10.0, [EMPTY] * 8, [EMPTY] * 8))
    # |dE| > 1 between neighbours (benefit capped at 1: the voiced <-> unvoiced step is free) and vuv == 0 frames
    en = [0.2, 0.3, 2.9, 3.1, 0.4, 0.3, 2.2, 0.9, 0.8, 0.05]
    c1 = [EMPTY, EMPTY, _one(180, 0.9), _one(182, 0.9), EMPTY, _one(181, 0.3), _one(184, 0.8), _one(186, 0.5), EMPTY, EMPTY]
    c2 = [EMPTY, _one(90, 0.3), _one(181, 0.7), ([183, 91, 183], [0.8, 0.5, 0.8]), EMPTY, EMPTY, _one(92, 0.6),
          _one(185, 0.45), _one(187, 0.3), EMPTY]
    out.append(final_case("energy_steps", en, [e > 0.75 for e in en], np.linspace(180, 189, 10), 6.0, c1, c2))
    return out


def _build_final_cases():
    out = _final_literals()
    for c in out:
        m = margins(c)
        assert m["ok"], (c["name"], m["why"])
    seed = 300
    for t in (1, 2, 3, 4, 5, 6, 7, 8, 40, 255, 256, 257, 300, 520):
        out.append(_draw(lambda k: random_final(f"rand_t{t}", t, seed + 1000 * k, p_loud=0.6 if t <= 40 else 0.12), f"rand_t{t}"))
        seed += 1
    for c in list(out):
        if c["t"] and (c["t"] <= 40 or c["t"] == 257):
            for mv in (3, 9):
                v = dict(c, name=f"{c['name']}@m{mv}", median=mv)
                if margins(v)["ok"]:
                    out.append(v)
    return out


# ---------------------------------------------------------------------------------------------------------------
# builders: the long utterances that move the back-pointers out of LDS
# ---------------------------------------------------------------------------------------------------------------
_BIG = {}


def big_launches():
    """[(F, spec cases, final cases)]: B = 2 at F_SPEC_WS (both kernels in the workspace; row 1 short, so a wrong
    per-row offset into the byte workspace shows) and B = 1 at F_FINAL_WS (spec-track in LDS, final-track not)."""
    if not _BIG:
        F = F_SPEC_WS
        a = [_draw(lambda k: random_spec(f"big_f{F}", F, 500 + 1000 * k, 0.5, p_pad=0.0), f"big_f{F}"),
             _draw(lambda k: random_spec("big_row1_f300", 300, 501 + 1000 * k, 0.5, p_pad=0.0), "big_row1_f300")]
        b = [_draw(lambda k: random_final(f"big_t{F}", F, 510 + 1000 * k, p_loud=0.01), f"big_t{F}"),
             _draw(lambda k: random_final("big_row1_t300", 300, 511 + 1000 * k), "big_row1_t300")]
        G = F_FINAL_WS
        c = [_draw(lambda k: random_spec(f"big_f{G}", G, 520 + 1000 * k, 0.5, p_pad=0.0), f"big_f{G}")]
        d = [_draw(lambda k: random_final(f"big_t{G}", G, 530 + 1000 * k, p_loud=0.01), f"big_t{G}")]
        _BIG["v"] = [(F, a, b), (G, c, d)]
    return _BIG["v"]


def launch_branches(F, kind):
    """where a launch of width F keeps its back-pointers (from kLdsBack and the bytes per frame, not from a measurement)"""
    per = 4 if kind == "spec" else 8
    return {f"{kind}:back_in_workspace" if per * F > LDS_BACK else f"{kind}:back_in_lds"}


# ---------------------------------------------------------------------------------------------------------------
# builders: NCCF
# ---------------------------------------------------------------------------------------------------------------
NCCF_F = 14                        # lag-table width of the launch
NCCF_N = FLEN + HOP * NCCF_F       # 1440 samples: 14 time-domain frames when a row is full
WIDE = (40, 268)                   # the widest range the tracker derives (f0_max .. f0_min, +- nccf_pwidth // 2)
# The number of local peaks above nccf_thresh1 that the reference lists stays at or below 64 (YA_MAXLIST in yaapt.hip)
# in every frame built here.  In the product the NCCF input is band-passed at 1 500 Hz, so peaks are at least ~10.7 lags
# apart and the widest range (229 lags) holds at most about 22 of them.  The `tone3k` rows drive a 3 kHz tone (period
# 5.33 lags) through the widest range to load the list with about 43.  No case goes beyond 64: the truncation there is
# unspecified.
DEGENERATE = [(1, 2), (5, 6), (266, 268), (583, 268), (300, TDA), (300, TDA + 50)]


def _tones(rs, n, freqs, amps, noise):
    t = np.arange(n) / FS
    x = sum(a * np.sin(2 * np.pi * f * t + rs.uniform(0, 2 * np.pi)) for f, a in zip(freqs, amps))
    return x + noise * rs.standard_normal(n)


def _nccf_row(name, sig, ns, lags):
    sig = _f32(sig)
    assert len(sig) == NCCF_N and len(lags) == NCCF_F and 0 < ns <= NCCF_N
    return {"name": name, "sig": sig, "ns": int(ns), "lags": [tuple(int(v) for v in l) for l in lags]}


def _one_frame_row(name, make, lag, seed):
    """a row with a single time-domain frame: signal from `make(rs)`, drawn again (next seed) until the frame's
    decisions hold margin (d); after 25 draws the frame stays and counts as dropped"""
    for k in range(25):
        row = _nccf_row(name, make(np.random.RandomState(seed + 1000 * k)), TDA + 37, [lag] + [WIDE] * (NCCF_F - 1))
        if nccf_frame_info(row, 0)[1]:
            break
    return row


def _glide(rs, n, f_from, f_to, amps, noise):
    ph = 2 * np.pi * np.cumsum(np.linspace(f_from, f_to, n)) / FS
    x = sum(a * np.sin(k * ph + rs.uniform(0, 2 * np.pi)) for k, a in enumerate(amps, 1))
    return x + noise * rs.standard_normal(n)


RANGES = [WIDE, (60, 140), (70, 90), (40, 100), (100, 268), (90, 130), (50, 75), (120, 200), (45, 60), (200, 268), (60, 268)]
PARTIALS = [([211.0, 333.0, 517.0, 790.0, 1130.0], 0.35), ([157.0, 412.0, 655.0, 1010.0, 1390.0], 0.5),
            ([263.0, 596.0, 873.0, 1210.0], 0.25)]


def build_nccf_case(seed):
    rs = np.random.RandomState(seed)
    rows = []
    n = NCCF_N
    voiced_amps = [1.0, 0.8, 0.9, 0.7, 0.8, 0.6, 0.7]
    # a clean periodic signal (harmonics to 1.3 kHz, a slow glide so that the peaks at two and three periods stand
    # below the first): amax > nccf_thresh2 -> the single-candidate arm.  Six overlapping frames of one row, then
    # single frames under the wider ranges
    rows.append(_nccf_row("periodic", _glide(rs, n, 186.0, 198.0, voiced_amps, 0.002), FLEN + HOP * 6,
                          [(70, 100), (60, 120), (40, 120), (75, 95), (1, 2), (80, 90)] + [WIDE] * 8))
    for j, lag in enumerate([WIDE, (60, 268), (150, 268), (60, 180), WIDE, (160, 175)]):
        rows.append(_one_frame_row(f"periodic_{j}", lambda r: _glide(r, n, 150.0 + 20 * j, 190.0 + 25 * j, voiced_amps, 0.01),
                                   lag, seed * 100 + j))
    # inharmonic partials + noise: amax < nccf_thresh2 -> the local-maximum arm with a varying number of survivors.
    # One row of overlapping frames that ends 37 samples after its 6th frame (frames 6.. would run past the end), then
    # single frames
    fr, noise = PARTIALS[0]
    rows.append(_nccf_row("inharmonic", _tones(rs, n, fr, rs.uniform(0.6, 1.0, len(fr)), noise), FLEN + HOP * 6 + 37,
                          RANGES[:6] + [WIDE] * 8))
    for j, lag in enumerate(RANGES + RANGES):
        fr, noise = PARTIALS[j % 3]
        rows.append(_one_frame_row(f"inharmonic_{j}", lambda r: _tones(r, n, fr, r.uniform(0.6, 1.0, len(fr)), noise), lag,
                                   seed * 100 + 20 + j))
    # a 3 kHz tone through the widest range: about 43 listed peaks.  Nearly clean, gliding 2.9 -> 3.5 kHz so that the
    # peak height falls with the lag (single arm); and noisy (> 3 survivors of the window test)
    for j in range(2):
        rows.append(_one_frame_row(f"tone3k_clean_{j}", lambda r: _glide(r, n, 2900.0, 3500.0, [1.0], 0.01), WIDE,
                                   seed * 100 + 60 + j))
    for j in range(4):
        rows.append(_one_frame_row(f"tone3k_noisy_{j}", lambda r: _tones(r, n, [3000.0], [1.0], 0.42), WIDE,
                                   seed * 100 + 70 + j))
    # digital silence, a step, then a constant (0.5: the kernel's float32 frame mean is exact for it); the frames that
    # straddle the step carry the degenerate lag ranges
    x = np.zeros(n)
    x[760:] = 0.5
    lags = [WIDE, (60, 140), (1, 2), WIDE] + [DEGENERATE[i] for i in (0, 1, 2, 3, 4, 5)] + [WIDE, (60, 140), (583, 268), WIDE]
    rows.append(_nccf_row("zeros_step_constant", x, n, lags))
    # the degenerate ranges on a live signal as well
    x = _tones(rs, n, [180.0, 360.0, 540.0, 900.0], [1.0, 0.7, 0.8, 0.5], 0.01)
    lags = DEGENERATE + [(1, 2), (583, 268)] + DEGENERATE
    rows.append(_nccf_row("degenerate_on_voiced", x, n, lags))
    # lag_max = TDA - 1: a one-sample window, phi = +-1 by the signs of x[0] x[lag]; one frame only (ns = TDA)
    x = rs.uniform(0.5, 1.0, n) * rs.choice([-1.0, 1.0], n)
    x[0] = 0.8
    x[385:TDA] = -np.abs(x[385:TDA])
    x[394] = 0.9
    rows.append(_nccf_row("one_sample_window", x, TDA, [(388, TDA - 1)] + [WIDE] * (NCCF_F - 1)))
    x = x.copy()
    x[394] = -0.9
    rows.append(_nccf_row("one_sample_window_empty", x, TDA + HOP - 1, [(388, TDA - 1)] + [WIDE] * (NCCF_F - 1)))
    return {"kind": "nccf", "name": f"nccf_seed{seed}", "rows": rows}


# ---------------------------------------------------------------------------------------------------------------
# branches
# ---------------------------------------------------------------------------------------------------------------
def _sgn(v):
    return int(v > 0) - int(v < 0)


def _spec_branches(case):
    f, nt, mv = case["f"], case["n_tda"], case["median"]
    if f == 0:
        return {"spec:f==0"}
    with traced() as rec:
        r = spec_reference(case)
    tags = set()
    cp0 = case["cand_pitch"][:f, 0]
    voiced = r["vuv"] & (cp0 > 0)
    nv = int(voiced.sum())
    if r["mean"] == 0:
        tags.add("spec:mean==0")
    if nv == 0:
        if r["mean"] == 0 and (cp0 > 0).any():
            tags.add("nv==0:zero_energy")
        if r["mean"] > 0 and (~r["vuv"] & (cp0 > 0)).any():
            tags.add("nv==0:below_thresh1")
        if (r["vuv"] & (cp0 == 0)).any():
            tags.add("nv==0:voiced_without_candidate")
    else:
        if nv <= 3:
            tags.add(f"nv=={nv}")
        k5 = max(1, mv - 2)
        if nv > 2:
            tags.add(f"median:k5=={k5}")
            if nv < k5:
                tags.add("median:wider_than_data")
        track = rec["medfilt"][1][2] if nv > 2 else np.full(nv, 150.0)
        t_avg = track.mean()
        for end, q in (("first", 0), ("last", -1)):
            if not voiced[q]:
                tags.add(f"end:unvoiced_{end}")
            elif track[q] < t_avg / 2:
                tags.add(f"end:voiced_low_{end}")
        x, y = rec["pchip"][0] if rec["pchip"] else (np.zeros(1), np.zeros(1))
        nk = len(x)
        if nk <= 3:
            tags.add(f"nk=={nk}")
        if nk < f:
            tags.add("pchip:interpolates")
        if nk >= 2:
            h = np.diff(x).astype(np.float64)
            m = np.diff(y) / h
            if nk == 2 and m[0] != 0:
                tags.add("nk==2:sloped")
            for k in range(1, nk - 1):
                if m[k - 1] == 0 or m[k] == 0:
                    tags.add("pchip:zero_secant")
                elif _sgn(m[k - 1]) != _sgn(m[k]):
                    tags.add("pchip:sign_change")
                else:
                    tags.add("pchip:harmonic_mean")
            if nk >= 3:
                for h0, h1, m0, m1 in ((h[0], h[1], m[0], m[1]), (h[-1], h[-2], m[-1], m[-2])):
                    d = ((2 * h0 + h1) * m0 - h0 * m1) / (h0 + h1)
                    if _sgn(d) != _sgn(m0):
                        if m0 != 0:
                            tags.add("pchip:end_d=0")
                    elif _sgn(m0) != _sgn(m1) and abs(d) > 3 * abs(m0):
                        tags.add("pchip:end_d=3m0")
        if nv > 2 and spec_differs(case, spec_reference(case, _variant("viterbi_last_min")), r):
            tags.add("viterbi:tie")
    tags.add("spec:f<=3" if f <= 3 else "spec:f==4" if f == 4 else "spec:f>4")
    if nt < f:
        tags.add("lag:rows_beyond_n_tda")
    if nt:
        if (r["spec"][:nt] - 2 * r["spec_std"] < P["f0_min"]).any():
            tags.add("lag:clamp_f0_min")
        if (r["spec"][:nt] + 2 * r["spec_std"] > P["f0_max"]).any():
            tags.add("lag:clamp_f0_max")
        if (r["lag_min"] >= r["lag_max"]).any():
            tags.add("lag:inverted")
    if f in (255, 256, 257, 511, 513) and 0 < nv < f // 4:
        tags.add(f"chunk:f=={f}")
    return tags


def _final_parts(case):
    """which of dead / has / none each frame is, with the sorted merits, from the case's inputs"""
    p = params(case["median"])
    t = case["t"]
    pit = np.hstack([case["tp1"][:t], case["tp2"][:t]]).astype(np.float64)
    raw = np.hstack([case["tm1"][:t], case["tm2"][:t]])
    diff = np.abs(pit - case["spec"][:, None])
    thresh = 5.0 * case["spec_std"]
    mer = (1.0 + p["merit_boost"]) * raw * np.where(diff < thresh, 1.0 - diff / thresh, 0.0)
    order = np.argsort(-mer, axis=1, kind="stable")
    rows = np.arange(t)[:, None]
    dead = case["en_norm"] <= p["nlfer_thresh2"]
    has = (pit[rows, order][:, 0] > 0) & ~dead
    return {"pit": pit[rows, order], "mer": mer[rows, order], "raw": raw, "diff": diff, "thresh": thresh, "dead": dead,
            "has": has, "none": ~has & ~dead, "unsorted_pit": pit, "unsorted_mer": mer}


def _final_branches(case):
    t = case["t"]
    if t == 0:
        return {"final:t==0"}
    p = params(case["median"])
    q = _final_parts(case)
    tags = set()
    if t <= 3:
        tags.add(f"final:t=={t}")
    if t < case["median"]:
        tags.add("final:median_wider_than_data")
    tags.add(f"final:median=={case['median']}")
    if q["dead"].any():
        tags.add("dead")
    if (case["en_norm"] == p["nlfer_thresh2"]).any():
        tags.add("dead:en==thresh2")
    if q["none"].any():
        tags.add("none")
    if (q["has"][:, None] & (q["pit"][:, 1:5] == 0)).any():
        tags.add("has:empty_middle")
    if q["dead"].all():
        tags.add("all_dead")
    if q["none"].all():
        tags.add("all_none")
    with traced() as rec:
        f0 = final_reference(case)
    loc = rec["viterbi"][0][0]
    rp, _ = f0m.merge_candidates(case["tp1"].T, case["tm1"].T, case["tp2"].T, case["tm2"].T, case["spec"],
                                 case["spec_std"], case["en_norm"], case["vuv"].astype(bool), p)
    if not (rp[0] > 0).any():
        tags.add("final:mean_pitch_fallback")
    live = q["raw"] > 0.0011
    if (live & (q["diff"] > q["thresh"])).any():
        tags.add("weight0:diff>5std")
    if (live & (q["diff"] == q["thresh"])).any():
        tags.add("weight0:diff==5std")
    um, up = q["unsorted_mer"], q["unsorted_pit"]
    for i in range(t):
        for a in range(6):
            for b in range(a + 1, 6):
                if um[i, a] == um[i, b] and um[i, a] > 0:
                    if up[i, a] == up[i, b]:
                        tags.add("sort:duplicated_row")
                    elif a < 3 <= b:
                        tags.add("sort:tie_pass1_pass2")
                    else:
                        tags.add("sort:tie_in_pass")
    if (case["vuv"] == 0).any():
        tags.add("vuv==0")
    if t > 1:
        cur, prv = rp.T[1:, :, None], rp.T[:-1, None, :]
        if ((cur > 0) & (prv > 0)).any():
            tags.add("trans:both")
        if ((cur == 0) & (prv == 0)).any():
            tags.add("trans:neither")
        if ((cur > 0) != (prv > 0)).any():
            tags.add("trans:mixed")
        if (np.abs(np.diff(case["en_norm"])) > 1).any():
            tags.add("trans:|dE|>1")
        assert loc.shape == rp.shape
        if (f0 > 0).any() and (f0 == 0).any():
            tags.add("final:track_switches_voicing")
    if t in (255, 256, 257):
        tags.add(f"chunk:t=={t}")
    return tags


def _cmp_rate_decisions(phi, lmin, lmax, bar):
    """the decisions oracle cmp_rate takes on phi, each with its margin: -> (robust, tags).  A decision is robust when an
    error of bar / 2 on every phi value cannot flip it: a conjunction holds with every term >= bar clear, or fails with
    one term >= bar clear."""
    c = P["nccf_pwidth"] // 2
    t1, t2 = P["nccf_thresh1"], P["nccf_thresh2"]
    tags, robust = set(), True
    pk = []
    for k in range(lmin + c, lmax - c + 1):
        terms = [phi[k] - phi[k - 1], phi[k] - phi[k + 1], phi[k] - t1]
        if min(terms) >= bar:
            pk.append(k)
        elif not min(terms) <= -bar:
            robust = False
            if min(terms) > 0:
                pk.append(k)
    if not pk:
        return robust, {"nccf:no_peak"}
    if len(pk) >= 40:
        tags.add("nccf:list>=40")
    amax = float(np.max(phi))
    robust &= abs(amax - t2) >= bar
    if amax > t2:
        tags.add("nccf:single")
        v = np.sort(phi[pk])[::-1]
        robust &= len(v) < 2 or v[0] - v[1] >= bar
        cand = [pk[int(np.argmax(phi[pk]))]]
    else:
        cand = []
        for k in pk:
            others = np.delete(phi[k - c:k + c + 1], c)
            gap = phi[k] - others.max()
            robust &= abs(gap) >= bar
            if gap > 0:
                cand.append(k)
        if not cand:
            return robust, {"nccf:no_peak"}
        tags.add(f"nccf:multi=={len(cand)}" if len(cand) <= 3 else "nccf:multi>3")
        v = np.sort(phi[cand])[::-1][:4]
        robust &= len(v) < 2 or float(np.min(-np.diff(v))) >= bar
    if len(cand) < 3:
        tags.add("nccf:fill")
    return robust, tags


def nccf_frame_info(row, fr):
    """(tags, kept) of frame `fr` of a row; kept = its candidate decisions hold margin (d)"""
    lmin, lmax = row["lags"][fr]
    nfr = nccf_frames(row)
    if fr >= nfr:
        return ({"nccf:frame_past_end"} if fr * HOP < row["ns"] else {"nccf:beyond_the_signal"}), True
    tags = set()
    x = row["sig"][fr * HOP:fr * HOP + TDA].astype(np.float64)
    if fr * HOP + TDA == row["ns"]:
        tags.add("nccf:frame_ends_on_last_sample")
    if not x.any():
        tags.add("nccf:zero_frame")
    elif np.ptp(x) == 0:
        tags.add("nccf:constant_frame")
    if (lmin, lmax) == (1, 2):
        tags.add("nccf:range(1,2)")
    elif lmax >= TDA:
        tags.add("nccf:lmax>=tda")
    elif lmax < lmin:
        tags.add("nccf:inverted")
    elif lmax == lmin + 1:
        tags.add("nccf:lmax==lmin+1")
    elif lmax - lmin < 2 * (P["nccf_pwidth"] // 2):
        tags.add("nccf:narrower_than_pwidth")
    if lmax == TDA - 1:
        tags.add("nccf:lmax==tda-1")
    if lmax >= TDA or lmax - lmin < 2 * (P["nccf_pwidth"] // 2):
        return tags | {"nccf:no_peak"}, True
    phi = nccf_frame_reference(row, fr)[0]
    robust, more = _cmp_rate_decisions(phi, lmin, lmax, 2e-3)
    return tags | more, bool(robust)


def _nccf_branches(case):
    tags = set()
    for row in case["rows"]:
        for fr in range(NCCF_F):
            t, kept = nccf_frame_info(row, fr)
            if kept:
                tags |= t
    return tags


def branches(case):
    return {"spec": _spec_branches, "final": _final_branches, "nccf": _nccf_branches}[case["kind"]](case)


# "Paths no test reaches", written out as tags
ALL_BRANCHES = [
    # spec-track kernel
    "spec:f==0", "spec:mean==0", "nv==0:below_thresh1", "nv==0:zero_energy", "nv==0:voiced_without_candidate",
    "nv==1", "nv==2", "nv==3", "median:wider_than_data", "median:k5==1", "median:k5==5", "median:k5==7",
    "end:unvoiced_first", "end:unvoiced_last", "end:voiced_low_first", "end:voiced_low_last",
    "nk==1", "nk==2", "nk==2:sloped", "nk==3", "pchip:interpolates", "pchip:sign_change", "pchip:zero_secant",
    "pchip:harmonic_mean", "pchip:end_d=0", "pchip:end_d=3m0", "viterbi:tie",
    "spec:f<=3", "spec:f==4", "spec:f>4", "lag:clamp_f0_min", "lag:clamp_f0_max", "lag:rows_beyond_n_tda", "lag:inverted",
    "chunk:f==255", "chunk:f==256", "chunk:f==257", "chunk:f==511", "chunk:f==513",
    "spec:back_in_lds", "spec:back_in_workspace",
    # final-track kernel
    "final:t==0", "final:t==1", "final:t==2", "final:t==3", "final:median_wider_than_data", "final:median==3",
    "final:median==7", "final:median==9", "dead", "dead:en==thresh2", "none", "has:empty_middle", "all_dead", "all_none",
    "final:mean_pitch_fallback", "weight0:diff>5std", "weight0:diff==5std", "sort:duplicated_row", "sort:tie_pass1_pass2",
    "sort:tie_in_pass", "vuv==0", "trans:both", "trans:neither", "trans:mixed", "trans:|dE|>1",
    "final:track_switches_voicing", "chunk:t==255", "chunk:t==256", "chunk:t==257",
    "final:back_in_lds", "final:back_in_workspace",
    # NCCF kernel
    "nccf:range(1,2)", "nccf:lmax==lmin+1", "nccf:narrower_than_pwidth", "nccf:inverted", "nccf:lmax==tda-1",
    "nccf:lmax>=tda", "nccf:zero_frame", "nccf:constant_frame", "nccf:frame_past_end", "nccf:beyond_the_signal",
    "nccf:frame_ends_on_last_sample", "nccf:no_peak", "nccf:single", "nccf:multi==1", "nccf:multi==2", "nccf:multi==3",
    "nccf:multi>3", "nccf:fill", "nccf:list>=40",
]


# ---------------------------------------------------------------------------------------------------------------
# margins
# ---------------------------------------------------------------------------------------------------------------
def _threshold_margin(en, exact, why):
    # (a) every normalised energy >= 1e-9 away from both NLFER thresholds; a frame set exactly on one is excepted when
    # its value is exact on both sides (given in float64, or float32 energies whose mean is exactly 1)
    for name in ("nlfer_thresh1", "nlfer_thresh2"):
        d = np.abs(en - P[name])
        bad = (d < 1e-9) & ~((d == 0) & exact)
        if bad.any():
            why.append(f"(a) en_norm within 1e-9 of {name} at {np.nonzero(bad)[0][:3]}")


def _unsafe_ties(local, trans, path):
    """f0._viterbi's recursion once more, looking at every decision on `path`: a rival within 1e-9 of the best (costs are
    of order 1) is safe only as its twin -- same local cost, the same transition costs into it from every state and the
    same transition cost out of it, bit for bit (an identical or a mirror-image candidate), so that the tie is exact
    whatever the common factor of the transition costs.  -> number of decisions with another kind of rival"""
    K, F = local.shape
    cum = local[:, 0].copy()
    bad = 0

    def twins(a, b, j):
        return local[a, j] == local[b, j] and (j == 0 or np.array_equal(trans[j - 1][a], trans[j - 1][b]))
    for i in range(1, F):
        tot = trans[i - 1] + cum[None, :]
        k, a = path[i], path[i - 1]
        for b in np.nonzero(tot[k] - tot[k, a] < 1e-9)[0]:
            if b != a and not (twins(a, b, i - 1) and trans[i - 1][k, a] == trans[i - 1][k, b]):
                bad += 1
        cum = tot.min(axis=1) + local[:, i]
    a = path[-1]
    for b in np.nonzero(cum - cum[a] < 1e-9)[0]:
        if b != a and not twins(a, b, F - 1):
            bad += 1
    return bad


def _viterbi_margin(rec, why, mod=f0m):
    # (b) the path is the same when every transition cost is scaled by 1 +- 1e-12.  Two samples let through a tie that
    # rounding happens to decide the same way (two candidates that both lie between the pitch before and the pitch
    # after cost exactly the same in real arithmetic: |a-b| + |b-c| = |a-c|), so in addition no decision on the path
    # has a rival within 1e-9 other than an exact twin
    for local, trans, path in rec["viterbi"]:
        for s in (1.0 + 1e-12, 1.0 - 1e-12):
            if not np.array_equal(mod._viterbi(local, trans * s), path):
                why.append(f"(b) Viterbi path changes under transition costs * {s!r}")
        bad = _unsafe_ties(local, trans, path)
        if bad:
            why.append(f"(b) {bad} decisions on the Viterbi path have a rival within 1e-9 that is no exact twin")


def _spec_margins(case):
    why = []
    f, nt = case["f"], case["n_tda"]
    if f == 0:
        return {"ok": True, "why": why}
    with traced() as rec:
        r = spec_reference(case)
    if case["exact_mean1"] and r["mean"] != 1.0:
        why.append("exact_mean1 set but the mean is not 1")
    _threshold_margin(r["en_norm"], bool(case["exact_mean1"]) or r["mean"] == 0, why)
    _viterbi_margin(rec, why)
    # the pick before the first median (closest to 0.8 avg, weighted by merit) depends on the tree-ordered avg: the best
    # and the runner-up of another pitch must be 1e-9 (relative) apart
    voiced = r["vuv"] & (case["cand_pitch"][:f, 0] > 0)
    if voiced.any():
        vp, vm = r["pit"][:, voiced], r["mer"][:, voiced]
        d = np.abs(vp - 0.8 * vp[0].mean()) * (3.0 - vm)
        best = d.min(axis=0)
        other = np.where(vp == vp[d.argmin(axis=0), np.arange(vp.shape[1])][None, :], np.inf, d).min(axis=0)
        if (other - best < 1e-9 * np.maximum(best, 1.0)).any():
            why.append("(b) the pre-median pick has a near-tie between two pitches")
    # (c) fs / hi and fs / lo >= 1e-6 away from an integer wherever a lag is derived; a bound that sits exactly on the
    # f0_min / f0_max clamp is the same float64 constant on both sides and is excepted
    if nt:
        sp, sd = r["spec"][:nt], r["spec_std"]
        if not (np.isfinite(sp).all() and np.isfinite(sd) and sd > 0):
            why.append("(c) spec / spec_std not finite and positive")
        else:
            for raw, clamp, pick in ((sp - 2 * sd, P["f0_min"], np.maximum), (sp + 2 * sd, P["f0_max"], np.minimum)):
                v = FS / pick(raw, clamp)
                d = np.abs(v - np.round(v))
                if ((d < 1e-6) & (pick(raw, clamp) != clamp)).any():
                    why.append("(c) fs / bound within 1e-6 of an integer")
    return {"ok": not why, "why": why}


def _final_margins(case):
    why = []
    if case["t"] == 0:
        return {"ok": True, "why": why}
    _threshold_margin(case["en_norm"], True, why)
    with traced() as rec:
        final_reference(case)
    _viterbi_margin(rec, why)
    return {"ok": not why, "why": why}


def _nccf_margins(case):
    # (d) every decision of cmp_rate has a margin of 2e-3 (four times the 5e-4 bar on phi) on the frames kept; at most
    # 10 % of the frames with a real lag range may be dropped
    why, kept = [], {}
    real = dropped = 0
    for row in case["rows"]:
        for fr in range(NCCF_F):
            tags, ok = nccf_frame_info(row, fr)
            kept[(row["name"], fr)] = ok
            if fr < nccf_frames(row):
                real += 1
                dropped += not ok
                if "nccf:no_peak" not in tags or ok:
                    phi = nccf_frame_reference(row, fr)[0]
                    lmin, lmax = row["lags"][fr]
                    c = P["nccf_pwidth"] // 2
                    n_list = sum(1 for k in range(max(lmin + c, 1), min(lmax - c + 1, TDA - 1))
                                 if phi[k] > phi[k - 1] and phi[k] > phi[k + 1] and phi[k] > P["nccf_thresh1"])
                    if n_list > 64:
                        why.append(f"{row['name']}[{fr}] lists {n_list} peaks (> YA_MAXLIST)")
    if dropped > 0.1 * real:
        why.append(f"(d) {dropped} of {real} frames dropped (> 10 %)")
    return {"ok": not why, "why": why, "kept": kept, "dropped": dropped, "frames": real}


def margins(case):
    """the conditions under which float64 numpy and the device may be compared exactly on a case -> {'ok', 'why', ...}"""
    return {"spec": _spec_margins, "final": _final_margins, "nccf": _nccf_margins}[case["kind"]](case)


# ---------------------------------------------------------------------------------------------------------------
# controls: dissc_amd.f0's own stages with one seeded defect each
# ---------------------------------------------------------------------------------------------------------------
def _medfilt_edge(x, k):
    x = np.asarray(x, dtype=np.float64)
    if len(x) == 0 or k <= 1:
        return x.copy()
    h = k // 2
    xp = np.concatenate([np.full(h, x[0]), x, np.full(h, x[-1])])
    return np.array([np.median(xp[i:i + k]) for i in range(len(x))])


def _pchip_no_two_point_rule(x, y):
    if len(x) == 2:
        return _sp_interp.CubicHermiteSpline(x, y, np.zeros(2))
    return _sp_interp.pchip(x, y)


# defect -> (the line of the kernels it stands for, [(old, new)] edits of f0.py's source, names injected)
DEFECTS = {
    "median_edge_replicated": ("yaapt_dp.hip median_at: `(i >= 0 && i < n) ? a[i] : 0.0`", [], {"medfilt": _medfilt_edge}),
    "viterbi_last_min": ("yaapt_dp.hip viterbi_wave: `if (fr == 0 || c < best)` and `if (k == 0 || c < bestc)`",
                         [("back[i] = np.argmin(tot, axis=1)", "back[i] = K - 1 - np.argmin(tot[:, ::-1], axis=1)"),
                          ("path[-1] = int(np.argmin(cum))", "path[-1] = K - 1 - int(np.argmin(cum[::-1]))")], {}),
    "sort_order_reversed_among_equals": ("yaapt_dp.hip final-track insertion sort: `while (j > 0 && m[j - 1] < mkk)`",
                                         [('order = np.argsort(-merit, axis=0, kind="stable")',
                                           'order = 5 - np.argsort(-merit[::-1], axis=0, kind="stable")')], {}),
    "dead_strict": ("yaapt_dp.hip final-track: `const bool dead = e <= c.nlfer_thresh2`",
                    [('dead = en <= p["nlfer_thresh2"]', 'dead = en < p["nlfer_thresh2"]')], {}),
    "pchip_two_knots_flat": ("yaapt_dp.hip spec-track: `if (nk == 2) { d = mk(0); }`",
                             [("_interp.pchip(nz, spec[nz])", "_pchip_two(nz, spec[nz])")],
                             {"_pchip_two": _pchip_no_two_point_rule}),
    "voiced_low_end_kept": ("yaapt_dp.hip spec-track: `if (raw[0] < t_avg / 2)` / `if (raw[f - 1] < t_avg / 2)`",
                            [("if spec[0] < t_avg / 2:", "if spec[0] == 0:"), ("if spec[-1] < t_avg / 2:", "if spec[-1] == 0:")],
                            {}),
    "head_replaced_at_f3": ("yaapt_dp.hip spec-track: `if (tid == 0 && f > 3)`",
                            [("    if F > 3:\n        spec[0], spec[1] = spec[2], spec[3]",
                              "    if F >= 3:\n        spec[0], spec[1] = spec[2], (spec[3] if F > 3 else 0.0)")], {}),
    "f0_max_clamp_dropped": ("yaapt_dp.hip spec-track: `hi = hi < c.f0_max ? hi : c.f0_max`",
                             [('hi = np.minimum(spec + 2.0 * std, p["f0_max"])', "hi = spec + 2.0 * std")], {}),
}
_STAGES = ("_viterbi", "spectral_track", "lag_ranges", "merge_candidates", "final_track")
_VARIANTS = {}


class _Namespace:
    pass


def _variant(defect):
    """dissc_amd.f0's host stages recompiled from their own source with the defect's edits applied (None: unedited)"""
    if defect not in _VARIANTS:
        src = "\n\n".join(inspect.getsource(getattr(f0m, n)) for n in _STAGES)
        ns = dict(vars(f0m))
        if defect is not None:
            _, edits, inject = DEFECTS[defect]
            for old, new in edits:
                assert src.count(old) == 1, (defect, old)
                src = src.replace(old, new)
            ns.update(inject)
        exec(compile(src, f"<dissc_amd.f0 with {defect}>", "exec"), ns)
        mod = _Namespace()
        for k, v in ns.items():
            setattr(mod, k, v)
        _VARIANTS[defect] = mod
    return _VARIANTS[defect]


def spec_differs(case, got, want=None):
    """does `got` (a spec_reference-like dict) miss the GPU test's bars against the reference?"""
    want = spec_reference(case) if want is None else want
    if not np.array_equal(got["vuv"], want["vuv"]) or not np.allclose(got["en_norm"], want["en_norm"], rtol=1e-12, atol=0):
        return True
    if not np.allclose(got["spec"], want["spec"], rtol=1e-9, atol=0):
        return True
    if abs(got["spec_std"] - want["spec_std"]) > 1e-9 * want["spec_std"]:
        return True
    return not (np.array_equal(got["lag_min"], want["lag_min"]) and np.array_equal(got["lag_max"], want["lag_max"]))


def final_differs(case, got, want=None):
    want = final_reference(case) if want is None else want
    return not np.array_equal(np.float32(got), np.float32(want))


# ---------------------------------------------------------------------------------------------------------------
# the committed cases (built once per process)
# ---------------------------------------------------------------------------------------------------------------
_CACHE = {}


def spec_cases():
    if "spec" not in _CACHE:
        _CACHE["spec"] = _build_spec_cases()
    return _CACHE["spec"]


def final_cases():
    if "final" not in _CACHE:
        _CACHE["final"] = _build_final_cases()
    return _CACHE["final"]


def nccf_case():
    if "nccf" not in _CACHE:
        _CACHE["nccf"] = _draw(build_nccf_case, "nccf")
    return _CACHE["nccf"]


if __name__ == "__main__":   # after a change to a builder: print the seeds table to paste above
    _FIND.append({})
    spec_cases(), final_cases(), nccf_case(), big_launches()
    print("SEEDS =", _FIND[0])
