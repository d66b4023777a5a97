"""dissc_conv_info without a GPU: the tile shape every direct-conv launch runs on (conv_mfma32_kernel's twelve-entry table,
conv_mfma_kernel's eleven), held to a Python statement of the documented rules -- the small-grid step-down, the clamps of the
conv32_cfg_bm* / conv_cfg_bm* overrides, the phase grouping of ConvTranspose1d -- and the read-back of those options.  The GPU
tests (tests/test_gpu_direct_conv_tiles.py) take their tile ids and tile-edge lengths from this entry."""
import itertools

import pytest

import conv_grad_ref as R
from plan_rules import (CLASSES16, CLASSES32, DEFAULT16, DEFAULT32, STEPS, TILES16, TILES32, cls16, cls32, rule_override16,
                        rule_override32, rule_pick)
from tile_harness import lib, options  # noqa: F401  (lib: the module fixture)


def one(lib, cin, cout, k, d, B, L):
    info = lib.conv_info(cin, cout, k, d, 1, B, L)
    assert len(info) == 1
    i = info[0]
    assert (i["p0"], i["np"], i["ntap"], i["pad_left"], i["rows"]) == (0, 1, k, (k - 1) * d // 2, cout)
    assert (i["bm"], i["bn"]) == (TILES32 if i["family"] == 32 else TILES16)[i["cfg"]]
    return i


def test_shipped_tables_and_families(lib):
    for cls, cfg in DEFAULT32.items():
        assert lib.get_option(f"conv32_cfg_bm{cls}") == cfg
    for cls, cfg in DEFAULT16.items():
        assert lib.get_option(f"conv_cfg_bm{cls}") == cfg
    assert lib.lib.dissc_abi_version() == 9
    assert one(lib, 16, 16, 11, 5, 32, 4000)["family"] == 16 and one(lib, 16, 1, 7, 1, 32, 4000)["cfg"] == 6
    assert one(lib, 32, 32, 3, 1, 32, 4000)["family"] == 32
    with options(lib, mfma32=0):
        for M in (32, 40, 64, 128, 320, 512):
            i = one(lib, 64, M, 3, 1, 32, 4000)
            assert (i["family"], i["cfg"]) == (16, DEFAULT16[cls16(M)])
    # the special instances keep their own tile and are not described
    import ctypes
    n = ctypes.c_int(0)
    assert lib.lib.dissc_conv_info(768, 768, 1, 1, 1, 4, 100, None, 0, ctypes.byref(n)) == -1  # a big 1x1 layer
    assert lib.lib.dissc_conv_info(64, 64, 11, 7, 1, 4, 100, None, 0, ctypes.byref(n)) == -1   # span 70 > 60
    assert lib.lib.dissc_conv_info(64, 64, 4, 1, 1, 4, 100, None, 0, ctypes.byref(n)) == -1    # even k
    assert lib.lib.dissc_conv_info(64, 32, 5, 1, 2, 4, 100, None, 0, ctypes.byref(n)) == -1    # (k - s) odd
    assert lib.lib.dissc_conv_info(64, 64, 3, 1, 1, 4, 100, None, 0, ctypes.byref(n)) == 0 and n.value == 1  # count only


def test_step_down_follows_the_documented_rule(lib):
    """a grid of (M, B, L) on both sides of 256 workgroups for every tier of every class, under small_grid 1, 2 and 0"""
    seen = set()
    for M in (32, 40, 64, 96, 128, 200, 256, 320, 512):
        lens = set()
        for cfg in STEPS[cls32(M)]:
            bm, bn = TILES32[cfg]
            mt = -(-M // bm)
            for B in (1, 3, 32):
                nt = -(-256 // (mt * B))  # time tiles that reach 256 workgroups
                lens |= {(B, max(1, (nt - 1) * bn)), (B, (nt - 1) * bn + 1), (B, nt * bn), (B, 2 * nt * bn + 1)}
        for (B, L), sg in itertools.product(sorted(lens), (1, 2, 0)):
            with options(lib, small_grid=sg):
                got = one(lib, 48, M, 3, 1, B, L)
            want = rule_pick(M, B, L, sg)
            assert (got["family"], got["cfg"]) == (32, want), (M, B, L, sg, got)
            seen.add((cls32(M), want))
    assert seen == {(c, s) for c in CLASSES32 for s in STEPS[c]}  # every tier of every class was reached


def test_generator_layers_take_base_shapes_at_benchmark_size_and_the_last_tier_for_one_short_utterance(lib):
    for cin, cout, k, d, L in R.generator_layer_shapes(frames=500):
        i = one(lib, cin, cout, k, d, 32, L)
        if cout >= 32:
            assert (i["family"], i["cfg"]) == (32, DEFAULT32[cls32(cout)]), (cin, cout, k, d, L, i)  # 3 / 2 / 1 / 0
        else:
            assert (i["family"], i["cfg"]) == (16, 6)
    for cin, cout, k, d, L in R.generator_layer_shapes(frames=100):
        i = one(lib, cin, cout, k, d, 1, L)
        if cout >= 32:
            assert i["cfg"] == STEPS[cls32(cout)][-1] == rule_pick(cout, 1, L), (cin, cout, k, d, L, i)


def test_overrides_are_taken_or_clamped_and_switch_the_step_down_off(lib):
    for cls, cfg in itertools.product(CLASSES32, range(-1, 13)):
        key = f"conv32_cfg_bm{cls}"
        with options(lib, **{key: cfg}):
            want = rule_override32(cls, cfg)
            # set then get: an id the table takes reads back as set, a refused one leaves the shipped value
            assert lib.get_option(key) == (cfg if 0 <= cfg < 8 else DEFAULT32[cls])
            for M in (cls, cls + cls // 4):
                big, small = one(lib, 48, M, 3, 1, 32, 100000), one(lib, 48, M, 3, 1, 1, 64)
                assert big["cfg"] == want, (cls, cfg, big)
                # an override in force is left alone on a small grid; the shipped id steps down
                assert small["cfg"] == (want if want != DEFAULT32[cls] else STEPS[cls][-1]), (cls, cfg, small)
            for other in CLASSES32:
                if other != cls:
                    assert one(lib, 48, other, 3, 1, 32, 100000)["cfg"] == DEFAULT32[other]
        assert lib.get_option(key) == DEFAULT32[cls]
    with options(lib, mfma32=0):
        for cls, cfg in itertools.product(CLASSES16, range(-1, 13)):
            key = f"conv_cfg_bm{cls}"
            with options(lib, **{key: cfg}):
                assert lib.get_option(key) == (cfg if 0 <= cfg < 10 else DEFAULT16[cls])
                for B, L in ((32, 100000), (1, 64)):  # the 16-row family never steps down
                    got = one(lib, 48, cls, 3, 1, B, L)
                    assert (got["family"], got["cfg"]) == (16, rule_override16(cls, cfg)), (cls, cfg, got)
            assert lib.get_option(key) == DEFAULT16[cls]
    assert one(lib, 48, 16, 3, 1, 1, 64)["family"] == 16  # (below 32 rows whatever mfma32 says)


def phase_taps(p, k, s):
    """input offsets delta with a tap of phase p: out[s q + p] = sum x[q + delta] w[p + pad - s delta]"""
    pad = (k - s) // 2
    return [(p + pad - kk) // s for kk in range(k) if (kk - p - pad) % s == 0]


GENERATOR_UPS = [(512, 256, 11, 5), (256, 128, 8, 4), (128, 64, 8, 4), (64, 32, 4, 2), (32, 16, 4, 2)]
SYNTHETIC_UPS = [(96, 80, 9, 3), (64, 64, 4, 4), (64, 64, 12, 4), (32, 32, 9, 3), (48, 24, 3, 3), (128, 128, 6, 2), (64, 16, 7, 5),
                 (64, 64, 2, 2), (64, 64, 5, 3)]


@pytest.mark.parametrize("cin,cout,k,s", GENERATOR_UPS + SYNTHETIC_UPS)
def test_conv_transpose_grouping(lib, cin, cout, k, s):
    groups = lib.conv_info(cin, cout, k, 1, s, 4, 300)
    covered = []
    for g in groups:
        phases = list(range(g["p0"], g["p0"] + g["np"]))
        covered += phases
        ranges = [(min(t), max(t)) for t in map(lambda p: phase_taps(p, k, s), phases)]
        lo, hi = min(r[0] for r in ranges), max(r[1] for r in ranges)
        # the group's taps dlo .. dlo + ntap - 1 cover every tap of its phases, and no more than their union
        assert g["pad_left"] == -lo and g["ntap"] == hi - lo + 1, (g, ranges)
        for p in phases:
            assert all(lo <= dl <= hi for dl in phase_taps(p, k, s)) and phase_taps(p, k, s)
        if cout >= 64:
            assert len(set(ranges)) == 1, (g, ranges)  # wide layers: identical ranges only (no zero taps)
        assert g["rows"] == cout * g["np"]
        fam_tiles = TILES32 if g["family"] == 32 else TILES16
        assert (g["bm"], g["bn"]) == fam_tiles[g["cfg"]]
        assert g["family"] == (32 if g["rows"] >= 32 else 16)
    assert covered == list(range(s)), covered  # every phase in exactly one group, in order
    if cout < 64:
        assert len(groups) == 1  # narrow layers: one launch over the union
    else:
        for a, b in zip(groups, groups[1:]):  # maximal: neighbours differ in their range
            assert (a["pad_left"], a["ntap"]) != (b["pad_left"], b["ntap"])


def test_generator_conv_transpose_plans(lib):
    """the five ConvTranspose layers as the generator runs them: (p0, np, ntap, pad_left) per launch"""
    plan = lambda *a: [(g["p0"], g["np"], g["ntap"], g["pad_left"]) for g in lib.conv_info(*a[:3], 1, a[3], 32, 500)]
    assert plan(512, 256, 11, 5) == [(0, 2, 2, 1), (2, 1, 3, 1), (3, 2, 2, 0)]
    assert plan(256, 128, 8, 4) == [(0, 2, 2, 1), (2, 2, 2, 0)]
    assert plan(128, 64, 8, 4) == [(0, 2, 2, 1), (2, 2, 2, 0)]
    assert plan(64, 32, 4, 2) == [(0, 2, 3, 1)]
    assert plan(32, 16, 4, 2) == [(0, 2, 3, 1)]
