"""dissc_wino_info without a GPU: the conv_wino_kernel instance (NS, d, CPR, RH, TW, SHV) and grid that run_wino launches for a
six-point F(4,3) conv, held to a Python statement of the documented rules -- C = 64 on 64-row x 128-column tiles, C >= 128 on
128 x 64 tiles, either on 32 x 32 wave tiles below 96 workgroups of the large tile under "small_grid", the shared transform under
"wino_sv", 32 channels per barrier round where the registers allow it -- and to the tile geometry as conv_wino.hip's header
comment defines it.  Every plan must be launchable (the row tiles divide the 8 XCDs, the LDS fits the 160 KB the launch asks
for), and the library must carry exactly the instances the rules can reach.  The GPU tests (tests/test_gpu_wino_tiles.py) take
their instances and tile-edge lengths from this entry and their expected instance sets from the same statement of the rules,
`wino_instances` of tests/plan_rules.py."""
import ctypes
import itertools
import re

import pytest
import torch
import torch.nn.functional as F

from plan_rules import (DS, KS, LDS_LIMIT, SMALL_GRID, WINO_CS as CS, wino_all_instances as all_instances, wino_geometry as geometry,
                        wino_instances as instances, wino_rule as rule)
from tile_harness import beyond_mask, edge_mask, lib, options  # noqa: F401  (lib: the module fixture)

# outputs per workgroup tile for (k, d) = (3,1) (3,3) (3,5) (7,1) (7,3) (7,5) (11,1) (11,3) (11,5), worked by hand from
# OT = 4 D floor(32 TW / D) (3 - RH), D = d ceil(k / 3): C >= 128 (RH = 2); C = 64 (RH = 1) has twice that
OT_LARGE = (256, 252, 240, 252, 252, 240, 256, 240, 240)
OT_SMALL = (128, 120, 120, 120, 108, 120, 128, 96, 80)


def plan(lib, C, k, d, B, Lmax):
    """the entry's answer as a dict, or None where it refuses"""
    out = lib.DisscWinoPlan()
    if lib.lib.dissc_wino_info(C, k, d, B, Lmax, ctypes.byref(out)) != 0:
        return None
    return {f: getattr(out, f) for f, _ in lib.DisscWinoPlan._fields_}


def check_plan(p, C, k, d, B, Lmax, want):
    """the plan names the instance the rule gives, its widths are the restated geometry, its grid covers Lmax, it is launchable"""
    what = (C, k, d, B, Lmax, p)
    assert p is not None, what
    assert (p["cpr"], p["rh"], p["tw"], p["shv"]) == want, (what, want)
    assert (p["ns"], p["dilation"]) == (-(-k // 3), d), what
    assert (p["unit"], p["ot"]) == geometry(k, d, p["rh"], p["tw"]), what
    assert p["ot"] > 0 and p["ot"] % p["unit"] == 0 and p["ot"] % 4 == 0, what
    assert p["gx"] == -(-Lmax // p["ot"]) and p["gy"] * 32 * p["tw"] * p["rh"] == C, what
    assert p["gy"] >= 1 and 8 % p["gy"] == 0 and C % p["cpr"] == 0, ("not launchable", what)
    assert p["wgs"] == 8 * -(-p["gx"] * B // (8 // p["gy"])), what
    # two windows of cpr channels x at least (OT + the taps' reach) samples and 12 x 8 V rows of 112, within what the launch asks for
    floor = 4 * (2 * p["cpr"] * (p["ot"] + d * (3 * p["ns"] - 1)) + 12 * 8 * 112)
    assert floor <= p["lds_bytes"] <= LDS_LIMIT, (what, floor)


def threshold_lengths(C, k, d, B):
    """Lmax either side of the threshold of 96 workgroups at this batch, and one far above it"""
    ot = geometry(k, d, 1 if C == 64 else 2, 2)[1]
    rows = 1 if C == 64 else C // 128
    nt = -(-SMALL_GRID // (rows * B))  # time tiles of the longest utterance that reach the threshold
    lens = {1, ot, ot + 1, 300 * ot + 1, (nt - 1) * ot, (nt - 1) * ot + 1, nt * ot, nt * ot + 1}
    return sorted(n for n in lens if n >= 1)


def test_abi_and_the_tile_widths(lib):
    """the widths worked by hand, from the restated geometry and from the entry; every OT is a whole number of units (every tile
    starts on the global unit grid, which is what makes the instances of a shape agree bit for bit) and of output quads"""
    assert lib.lib.dissc_abi_version() == 9
    for i, (k, d) in enumerate(itertools.product(KS, DS)):
        assert geometry(k, d, 2, 2)[1] == OT_LARGE[i] and geometry(k, d, 2, 1)[1] == OT_SMALL[i], (k, d)
        assert geometry(k, d, 1, 2)[1] == 2 * OT_LARGE[i] and geometry(k, d, 1, 1)[1] == 2 * OT_SMALL[i], (k, d)
        with options(lib, small_grid=0):
            assert plan(lib, 128, k, d, 1, 1)["ot"] == OT_LARGE[i] and plan(lib, 64, k, d, 1, 1)["ot"] == 2 * OT_LARGE[i]
        with options(lib, small_grid=1):
            assert plan(lib, 512, k, d, 1, 1)["ot"] == OT_SMALL[i] and plan(lib, 64, k, d, 1, 1)["ot"] == 2 * OT_SMALL[i]
        for rh, tw in ((1, 1), (1, 2), (2, 1), (2, 2)):
            unit, ot = geometry(k, d, rh, tw)
            assert ot % unit == 0 and ot % 4 == 0 and 32 * tw - unit // 4 < ot // (4 * (3 - rh)) <= 32 * tw  # less than a unit's columns idle


@pytest.mark.parametrize("C", CS)
def test_ladder_and_launchability(lib, C):
    """C x k x d x B in 1..64 (and two large batches) x Lmax either side of the threshold, under small_grid 0 / 1 / 2 (any non-zero
    value switches the step-down on) x wino_sv 0 / 1 / 2: the instance is the rule's, the widths are the geometry's, the plan can
    be launched (gy divides 8: C = 512 has 8 row tiles on the small tile, 4 on the large one), the LDS fits"""
    seen = set()
    for k, d in itertools.product(KS, DS):
        for sg, sv in itertools.product((1, 0, 2), (1, 0, 2)):
            with options(lib, small_grid=sg, wino_sv=sv):
                for B in list(range(1, 65)) + [97, 1000]:
                    for Lmax in threshold_lengths(C, k, d, B):
                        want = rule(C, k, d, B, Lmax, sg, sv)
                        p = plan(lib, C, k, d, B, Lmax)
                        check_plan(p, C, k, d, B, Lmax, want)
                        seen.add((p["ns"], d) + want)
    assert seen == set().union(*(instances(C, k, d) for k in KS for d in DS)), seen
    assert len(seen) == (18 if C == 64 else 27)
    rh = 1 if C == 64 else 2
    assert [plan(lib, C, 7, 1, B, 1)["gy"] for B in (1, 4096)] == [C // (32 * rh), C // (64 * rh)]  # the small tile, the large one


def test_small_grid_off_and_the_transform_option(lib):
    with options(lib, small_grid=0):
        for C, k, d in itertools.product((128, 256, 512), KS, DS):
            for sv in (0, 1):
                with options(lib, wino_sv=sv):
                    p = plan(lib, C, k, d, 1, 1)
                assert (p["rh"], p["tw"], p["shv"]) == (2, 2, sv), (C, k, d, sv, p)
                assert p["cpr"] == ((32 if k == 3 else 16) if sv else (16 if (k, d) == (11, 5) else 32)), (C, k, d, sv, p)
        for k, d, sv in itertools.product(KS, DS, (0, 1)):  # "wino_sv" does not reach C = 64
            with options(lib, wino_sv=sv):
                p = plan(lib, 64, k, d, 1, 1)
            assert (p["cpr"], p["rh"], p["tw"], p["shv"]) == (16, 1, 2, 0), (k, d, sv, p)


def test_the_diagnostic_instance_of_c32(lib):
    """C = 32 (mode 2 of dissc_respair1d; no layer takes it): one instance whatever the options and the batch say"""
    for k, d, sg, sv, (B, L) in itertools.product(KS, DS, (0, 1), (0, 1), ((1, 1), (4096, 4096))):
        with options(lib, small_grid=sg, wino_sv=sv):
            p = plan(lib, 32, k, d, B, L)
        check_plan(p, 32, k, d, B, L, (16, 1, 1, 0))
        assert p["gy"] == 1


def test_refusals(lib):
    for args in [(16, 7, 1, 4, 100), (48, 7, 1, 4, 100), (96, 7, 1, 4, 100), (192, 7, 1, 4, 100), (1024, 7, 1, 4, 100),
                 (64, 5, 1, 4, 100), (64, 9, 1, 4, 100), (64, 7, 2, 4, 100), (64, 7, 0, 4, 100), (64, 7, 1, 0, 100), (64, 7, 1, 4, 0),
                 (32, 5, 1, 4, 100), (32, 7, 2, 4, 100)]:
        assert lib.lib.dissc_wino_info(*args, None) == -1, args
        assert b"wino_plan: no instance" in lib.lib.dissc_last_error()
    assert lib.lib.dissc_wino_info(64, 7, 1, 4, 100, None) == 0  # (the output is optional)


def test_the_library_carries_the_reachable_instances_and_no_other(lib):
    """the kernel instantiations named in the library are the 45 the rules reach -- five per (NS, d): before the ladder became a
    table, 18 more were built that no supported width could launch (the 16-channel fallbacks of the 32-channel rounds and the
    32-channel forms of their exceptions: every supported C has an even number of 16-channel chunks)"""
    with open(lib.library_path(), "rb") as f:
        blob = f.read()
    built = {tuple(int(v) for v in m.groups()) for m in
             re.finditer(rb"_ZN5dissc16conv_wino_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EEEvNS_8WinoArgsE", blob)}
    want = all_instances()
    assert len(want) == 45 and built == want, built ^ want


def test_the_edge_column_bar_has_teeth():
    """tests/test_gpu_wino_tiles.py holds the rms error over the columns within a unit of a tile boundary or of an utterance's end to
    2 x the direct kernel's.  A model of it on the CPU (C = 64, k = 7, d = 3: D = 9, unit 36, tiles of 216 and 504): the "kernel" is
    torch's fp32 conv over the channels in another order (a correct kernel with its own rounding), the "direct kernel" torch's
    fp32 conv, the reference float64, the lengths and the edge columns those of the GPU test.  Two defects, each in ONE utterance at
    ONE tile boundary (the second tile of the width under test): (a) the first tap dropped where it reads the previous tile's
    columns (d columns), (b) one unit's columns shifted by D.  Either must miss the edge bar by more than 1 000 x; the clean model must sit inside it."""
    C, k, d, unit, widths = 64, 7, 3, 36, (216, 504)
    D, pad = unit // 4, (k - 1) * d // 2
    lengths = [1009, 215, 216, 217, 431, 432, 433, 35, 37, 503, 504, 505]
    g = torch.Generator().manual_seed(7)
    B, ld = len(lengths), 1012
    x = torch.rand(B, C, ld, generator=g) * 2 - 1
    for i, n in enumerate(lengths):
        x[i, :, n:] = 0.0
    w = (torch.rand(C, C, k, generator=g) * 2 - 1) * 0.025 * (256 / C) ** 0.5
    b = torch.rand(C, generator=g) * 0.2 - 0.1
    xa = F.leaky_relu(x, 0.1)
    r64 = F.conv1d(xa.double(), w.double(), b.double(), padding=pad, dilation=d)
    direct = F.conv1d(xa, w, b, padding=pad, dilation=d)
    perm = torch.randperm(C, generator=g)
    clean = F.conv1d(xa[:, perm], w[:, perm], b, padding=pad, dilation=d)
    valid = ~beyond_mask(lengths, ld).expand(B, C, ld)
    def rms(y, mask):
        return float((torch.where(mask, y.double() - r64, torch.zeros_like(r64)).pow(2).sum() / mask.sum()).sqrt())

    for wd in widths:
        t0 = wd  # the second tile of row 0 on tiles of this width
        dropped = clean.clone()  # (a) outputs t0 .. t0 + d - 1 lose tap 0, which reads columns t0 - pad .. of the tile before
        dropped[0, :, t0:t0 + d] -= torch.einsum("oc,ct->ot", w[:, :, 0], xa[0, :, t0 - pad:t0 - pad + d])
        shifted = clean.clone()  # (b) the first unit of that tile comes from D columns further on
        shifted[0, :, t0:t0 + unit] = clean[0, :, t0 + D:t0 + unit + D]
        edge = edge_mask(lengths, ld, unit, [wd]).expand(B, C, ld) & valid
        base = rms(direct, edge)
        ratios = {name: rms(y, edge) / base for name, y in (("clean", clean), ("tap dropped", dropped), ("unit shifted", shifted))}
        whole = {name: rms(y, valid) / rms(direct, valid) for name, y in (("tap dropped", dropped), ("unit shifted", shifted))}
        print(f"\nteeth, edge columns of w {wd} ({100 * float(edge.sum()) / float(valid.sum()):.0f} % of all): rms / direct's "
              + ", ".join(f"{n} {v:.3g}" for n, v in ratios.items()) + "; over all columns " + ", ".join(f"{n} {v:.3g}" for n, v in whole.items()))
        assert ratios["clean"] <= 2.0
        assert ratios["tap dropped"] > 2.0 * 1000 and ratios["unit shifted"] > 2.0 * 1000, ratios
