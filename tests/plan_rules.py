"""The launch rules of the three conv families as Python statements, worked from the documented rules and the header comments of
the kernels, never from the library: the CPU plan tests (tests/test_conv_plan_cpu.py, test_wino_plan_cpu.py, test_wino8_plan_cpu.py)
hold dissc_conv_info / dissc_wino_info / dissc_wino8_info to them, and the GPU tile-edge tests take their expected instance sets and
row classes from here.  No library call, no fixture."""

# ---- the direct convs (conv_mfma32_kernel, conv_mfma_kernel) ----------------------------------------------------------------
# conv_mfma32.hip kCfgs32 / conv_mfma.hip kCfgs: id -> (BM, BN)
TILES32 = {0: (256, 64), 1: (128, 128), 2: (64, 128), 3: (32, 256), 4: (32, 512), 5: (64, 256), 6: (256, 128), 7: (128, 256),
           10: (64, 64), 11: (32, 128)}
TILES16 = {0: (256, 64), 1: (128, 128), 2: (64, 256), 3: (32, 512), 4: (16, 512), 5: (32, 256), 6: (16, 256), 7: (64, 128),
           8: (128, 64), 9: (256, 64), 10: (48, 256)}
CLASSES32, CLASSES16 = (32, 64, 128, 256), (16, 32, 64, 128, 256)
DEFAULT32 = {32: 3, 64: 2, 128: 1, 256: 0}
DEFAULT16 = {16: 6, 32: 5, 64: 7, 128: 1, 256: 0}
FALLBACK16 = {16: 4, 32: 3, 64: 2, 128: 1, 256: 0}  # what conv_cfg puts in place of an override whose BM exceeds the class
STEPS = {32: (3, 11), 64: (2, 10), 128: (1, 2, 10), 256: (0, 2, 10)}  # conv32_pick_cfg: by class, largest tile first


def cls32(M):
    return 256 if M >= 256 else 128 if M >= 128 else 64 if M >= 64 else 32


def cls16(M):
    return 256 if M >= 256 else 128 if M >= 128 else 64 if M >= 64 else 32 if M >= 32 else 16


def rule_pick(M, B, L, small_grid=1):
    """the documented rule: the class's table entry, then the first tile of the class's step list that gives at least
    256 * small_grid workgroups, otherwise the last one"""
    steps = STEPS[cls32(M)]
    if not small_grid:
        return steps[0]
    for cfg in steps:
        bm, bn = TILES32[cfg]
        if -(-L // bn) * -(-M // bm) * B >= 256 * small_grid:
            return cfg
    return steps[-1]


def rule_override32(cls, cfg):
    """conv32_set_cfg / conv32_cfg: ids 0..7 are taken, a tile taller than the class or id 4 outside class 32 is replaced by the
    class default; anything else leaves the table as it was"""
    if not 0 <= cfg < 8:
        return DEFAULT32[cls]
    if TILES32[cfg][0] > cls or (cfg == 4 and cls != 32):
        return DEFAULT32[cls]
    return cfg


def rule_override16(cls, cfg):
    if not 0 <= cfg < 10:  # (10, 48 x 256, belongs to the 48-row layers alone)
        return DEFAULT16[cls]
    return FALLBACK16[cls] if TILES16[cfg][0] > cls else cfg


# ---- the six-point F(4,3) convs (conv_wino_kernel) --------------------------------------------------------------------------
WINO_CS, KS, DS = (64, 128, 256, 512), (3, 7, 11), (1, 3, 5)
SMALL_GRID = 96        # workgroups of the large tile below which a launch steps down
LDS_LIMIT = 160 * 1024


def wino_geometry(k, d, rh, tw):
    """(unit, OT): a tile unit is 4 outputs in each of D = d NS phases, NS = ceil(k / 3) sub-filters; a wave's 32 TW columns (one
    per (unit, phase)) hold floor(32 TW / D) units; a workgroup has RH row halves and 3 - RH column halves"""
    D = d * -(-k // 3)
    return 4 * D, 4 * D * (32 * tw // D) * (3 - rh)


def wino_rule(C, k, d, B, Lmax, small_grid=1, wino_sv=1):
    """the documented choice (CPR, RH, TW, SHV)"""
    if C == 32:  # the diagnostic instance: no layer takes it
        return (16, 1, 1, 0)
    rh = 1 if C == 64 else 2
    n = -(-Lmax // wino_geometry(k, d, rh, 2)[1]) * (1 if C == 64 else C // 128) * B
    if small_grid and n < SMALL_GRID:
        return (16, rh, 1, 0)
    if C == 64:
        return (16, 1, 2, 0)
    if wino_sv:
        return (32 if k == 3 else 16, 2, 2, 1)  # (with 32 channels per round the k = 7 / 11 instances spill)
    return (16 if (k, d) == (11, 5) else 32, 2, 2, 0)  # (k = 11, d = 5 with 32 needs more registers than three waves per SIMD leave)


def wino_instances(C, k, d):
    """the instances (NS, d, CPR, RH, TW, SHV) a supported layer of C channels can reach, by the rule"""
    ns = -(-k // 3)
    return {(ns, d) + wino_rule(C, k, d, B, L, sg, sv) for B, L in ((1, 1), (4096, 4096)) for sg in (0, 1) for sv in (0, 1)}


def wino_all_instances():
    return set().union(*(wino_instances(C, k, d) for C in WINO_CS + (32,) for k in KS for d in DS))


# ---- the eight-point F(6,3) / F(5,4) convs (conv_wino8_kernel) --------------------------------------------------------------
WINO8_TILES = [(1, 1, 4), (2, 1, 4), (2, 2, 4), (4, 2, 2), (2, 4, 2), (2, 2, 2)]  # (MI, NI, WPS) built per transform shape
WINO8_CS, RS = (64, 128, 256, 512), (3, 4)


def wino8_geometry(R, k, d, NI, WPS):
    """(unit width, OT, CPR) of a tile.  A unit is MO = 9 - R outputs in each of D = d NS phases, NS = ceil(k / R) sub-filters; a
    tile of 32 NI columns (one per (unit, phase)) holds NTU = floor(32 NI / D) units -- as F(6,3) an odd D takes an even unit
    count, so that the tile is a whole number of output quads; F(5,4) takes them all.  A round stages 16 channels, 8 in the
    tiles built for two workgroups per CU (WPS = 4) or with 128 columns -- except the NI = 1 (latency) tiles, which stage 16."""
    MO, NS = 9 - R, -(-k // R)
    D = d * NS
    ntu = 32 * NI // D
    if R == 3 and D % 2 == 1 and ntu % 2 == 1:
        ntu -= 1
    cpr = 16 if NI == 1 else 8 if (NI == 4 or WPS == 4) else 16
    return MO * D, MO * D * ntu, cpr


def wino8_has_instance(C, k, d, R, experimental):
    if C not in WINO8_CS or k not in KS or d not in DS or R not in RS or (R == 4 and k == 3):
        return False
    return k != 3 or experimental or (C == 64 and d == 1)  # the default build carries one k = 3 instance


def wino8_rule(C, k, d, R, B, Lmax, small_grid=1, wide=3, experimental=False):
    """the documented tile choice.  C >= 128: 128 x 64 tiles; under "small_grid", with n = the workgroups those tiles would
    make, n < 128 -> 64 x 64 on two workgroups per CU, n < 64 -> 64 x 32, n < 32 -> 32 x 32 -- but never below the tile whose row
    tiles number 8 (they are pinned to the 8 XCDs and must divide them): C = 512 stops at MI = 2, on the same NI and so the
    same bits.  C = 64: under "small_grid", fewer than 192 of the 64 x 64 tiles -> 64 x 32; otherwise "wino8_c64_wide": 1 = 64 x 128,
    2 = 64 x 64 two per CU, 3 = 1 for k = 7 as F(6,3) and 2 otherwise, 4 = 1 for k = 7 and 2 otherwise, anything else 64 x 64 one
    per CU.  k = 3 (default build): the one instance whatever the options say."""
    if k == 3 and not experimental:
        return (2, 2, 4)
    if C >= 128:
        n = -(-Lmax // wino8_geometry(R, k, d, 2, 2)[1]) * (C // 128) * B
        if small_grid and n < 32:
            return (2 if C // 32 > 8 else 1, 1, 4)
        if small_grid and n < 64:
            return (2, 1, 4)
        if small_grid and n < 128:
            return (2, 2, 4)
        return (4, 2, 2)
    n = -(-Lmax // wino8_geometry(R, k, d, 2, 4)[1]) * (C // 64) * B
    if small_grid and n < 192:
        return (2, 1, 4)
    mode = ((1 if (k == 7 and R == 3) else 2) if wide == 3 else (1 if k == 7 else 2) if wide == 4 else wide)
    return {1: (2, 4, 2), 2: (2, 2, 4)}.get(mode, (2, 2, 2))
