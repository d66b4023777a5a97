"""dissc_wino8_info without a GPU: the conv_wino8_kernel instance (tile (MI, NI, WPS) of a transform shape (R, NS, d)) and grid
that run_wino8 launches, held to a Python statement of the documented rules -- the small-grid ladder of C >= 128 (thresholds
32 / 64 / 128 on the count of 128-row tiles), the one step of C = 64 (192 of the 64 x 64 tiles), "wino8_c64_wide", the fixed k = 3
instance -- and to the tile geometry as conv_wino8.hip's header comment and Wino8Geo define it.  Every plan must be launchable
(the row tiles divide the 8 XCDs): C = 512 therefore stops at MI = 2.  The GPU tests (tests/test_gpu_wino8_tiles.py) take their
tiles and tile-edge lengths from this entry."""
import ctypes
import itertools

import pytest

from plan_rules import (DS, KS, RS, WINO8_CS as CS, WINO8_TILES as TILES, wino8_geometry as geometry, wino8_has_instance as has_instance,
                        wino8_rule as rule)
from tile_harness import lib, options  # noqa: F401  (lib: the module fixture)


@pytest.fixture(scope="module")
def exp_build(lib):
    return lib.get_option("experimental") == 1


def plan(lib, C, k, d, R, B, Lmax):
    """the entry's answer as a dict, or None where it refuses"""
    out = lib.DisscWino8Plan()
    if lib.lib.dissc_wino8_info(C, k, d, R, B, Lmax, ctypes.byref(out)) != 0:
        return None
    return {f: getattr(out, f) for f, _ in lib.DisscWino8Plan._fields_}


def check_plan(p, C, k, d, R, B, Lmax, want):
    """the plan names the tile the rule gives, its widths are the restated geometry, its grid covers Lmax, and it is launchable"""
    what = (C, k, d, R, B, Lmax, p)
    assert p is not None, what
    assert (p["mi"], p["ni"], p["wps"]) == want, (what, want)
    assert (p["r"], p["ns"]) == (R, -(-k // R)), what
    assert (p["unit"], p["ot"], p["cpr"]) == geometry(R, k, d, p["ni"], p["wps"]), what
    assert p["gx"] == -(-Lmax // p["ot"]) and p["gy"] * 32 * p["mi"] == C, what
    assert p["gy"] >= 1 and 8 % p["gy"] == 0 and C % p["cpr"] == 0, ("not launchable", what)


def threshold_lengths(C, k, d, R, B):
    """Lmax either side of every threshold of the class at this batch, and one far above them all"""
    if C >= 128:
        ot, rows, ts = geometry(R, k, d, 2, 2)[1], C // 128, (32, 64, 128)
    else:
        ot, rows, ts = geometry(R, k, d, 2, 4)[1], C // 64, (192,)
    lens = {1, ot, 300 * ot + 1}
    for t in ts:
        nt = -(-t // (rows * B))  # time tiles of the longest utterance that reach the threshold
        lens |= {(nt - 1) * ot, (nt - 1) * ot + 1, nt * ot, nt * ot + 1}
    return sorted(n for n in lens if n >= 1)


def test_abi_and_unit_grid_of_every_tile(lib):
    """Every OT is a whole number of units (every tile starts on the global unit grid, which is what makes the tiles of a shape
    agree bit for bit) and every F(6,3) OT a whole number of output quads (its epilogue stores aligned quads only); F(5,4) has
    tiles that are not (the shared-quad path)."""
    assert lib.lib.dissc_abi_version() == 9
    odd = 0
    for R, k, d, (MI, NI, WPS) in itertools.product(RS, (7, 11), DS, TILES):
        unit, ot, cpr = geometry(R, k, d, NI, WPS)
        assert ot > 0 and ot % unit == 0 and unit == (9 - R) * d * -(-k // R)
        assert 32 * NI - d * -(-k // R) * (1 + (R == 3)) < ot // (9 - R) <= 32 * NI  # at most two units' columns are left empty
        if R == 3:
            assert ot % 4 == 0, (k, d, NI, ot)
        odd += ot % 4 != 0
    assert odd > 0
    assert geometry(3, 3, 1, 2, 4) == (6, 384, 8)
    # worked by hand: F(5,4) of k = 11 at d = 1 has D = 3, 21 units of 15 = 315 outputs, not whole quads; F(6,3) of k = 7 at d = 1
    # has D = 3 and drops the 21st unit: 20 units of 18 = 360
    assert geometry(4, 11, 1, 2, 4)[1] == 315 and geometry(3, 7, 1, 2, 2)[1] == 360


@pytest.mark.parametrize("C", CS)
def test_ladder_and_launchability(lib, exp_build, C):
    experimental = exp_build
    """C x k x d x R x B in 1..64 x Lmax either side of every threshold, under small_grid 1 / 0 / 2 (any non-zero value switches
    the ladder on) and, for C = 64, every "wino8_c64_wide": the tile is the rule's, the widths are the geometry's, the plan can
    be launched.  (Before the ladder stopped at gy = 8, C = 512 was refused on every grid below 32 workgroups.)"""
    seen = set()
    for k, d, R in itertools.product(KS, DS, RS):
        if not has_instance(C, k, d, R, experimental):
            assert plan(lib, C, k, d, R, 4, 1000) is None, (C, k, d, R)
            assert b"no instance" in lib.lib.dissc_last_error()
            continue
        for sg, wide in [(1, 3), (0, 3), (2, 3)] + ([(s, w) for s in (1, 0) for w in (0, 1, 2, 4, 7)] if C == 64 else []):
            with options(lib, small_grid=sg, wino8_c64_wide=wide):
                for B in range(1, 65):
                    for Lmax in threshold_lengths(C, k, d, R, B):
                        want = rule(C, k, d, R, B, Lmax, sg, wide, experimental)
                        p = plan(lib, C, k, d, R, B, Lmax)
                        check_plan(p, C, k, d, R, B, Lmax, want)
                        seen.add((R, p["ns"], want))
    # every tier of the class was reached, in both forms
    if C >= 128:
        tiers = {(2 if C == 512 else 1, 1, 4), (2, 1, 4), (2, 2, 4), (4, 2, 2)}
    else:
        tiers = {(2, 1, 4), (2, 4, 2), (2, 2, 4), (2, 2, 2)}
    assert {t for R, ns, t in seen if ns > 1} == tiers, seen
    assert {(R, ns) for R, ns, _ in seen if ns > 1} == {(3, 3), (3, 4), (4, 2), (4, 3)}
    if C == 64 and not experimental:
        assert {t for R, ns, t in seen if ns == 1} == {(2, 2, 4)}  # k = 3: one instance under every option


def test_small_grid_off_and_the_k3_instance(lib, exp_build):
    experimental = exp_build
    with options(lib, small_grid=0):
        for C, k, d, R in itertools.product((128, 256, 512), (7, 11), DS, RS):
            p = plan(lib, C, k, d, R, 1, 1)
            assert (p["mi"], p["ni"], p["wps"]) == (4, 2, 2), (C, k, d, R, p)
    if not experimental:
        for sg, wide, B, L in itertools.product((0, 1), range(5), (1, 64), (1, 100000)):
            with options(lib, small_grid=sg, wino8_c64_wide=wide):
                p = plan(lib, 64, 3, 1, 3, B, L)
                assert (p["mi"], p["ni"], p["wps"], p["ns"], p["unit"], p["ot"]) == (2, 2, 4, 1, 6, 384), (sg, wide, p)
                assert plan(lib, 128, 3, 1, 3, B, L) is None and plan(lib, 64, 3, 3, 3, B, L) is None


def test_refusals(lib):
    for args in [(32, 7, 1, 3, 4, 100), (96, 7, 1, 3, 4, 100), (1024, 7, 1, 3, 4, 100), (64, 5, 1, 3, 4, 100), (64, 7, 2, 3, 4, 100),
                 (64, 7, 1, 2, 4, 100), (64, 7, 1, 5, 4, 100), (64, 3, 1, 4, 4, 100), (64, 7, 1, 3, 0, 100), (64, 7, 1, 3, 4, 0)]:
        assert lib.lib.dissc_wino8_info(*args, None) == -1, args
        assert b"wino8_plan: no instance" in lib.lib.dissc_last_error()
    assert lib.lib.dissc_wino8_info(64, 7, 1, 3, 4, 100, None) == 0  # (the output is optional)


def test_c512_small_grids_stop_at_eight_row_tiles(lib):
    """the defect this entry showed: C = 512 on fewer than 32 workgroups took the 32-row tile, whose 16 row tiles no launch
    accepts -- a 512-channel layer worked in a big batch and failed every forward at B = 1"""
    for k, d, R in itertools.product((7, 11), DS, RS):
        p = plan(lib, 512, k, d, R, 1, 300)
        assert p is not None and (p["mi"], p["ni"], p["wps"], p["gy"]) == (2, 1, 4, 8), (k, d, R, p)
        q = plan(lib, 256, k, d, R, 1, 300)
        assert (q["mi"], q["ni"], q["wps"], q["gy"]) == (1, 1, 4, 8) and (q["unit"], q["ot"]) == (p["unit"], p["ot"])
