"""conv_wino8_kernel (the eight Toom-Cook points as F(6,3) and F(5,4)) in EVERY instance the library carries -- 12 transform shapes
(k = 7 / 11, d = 1 / 3 / 5, both forms) x 6 tiles (MI, NI, WPS), and the one k = 3 instance -- at lengths that end beside every
tile's edge: all tiles of a shape must give the same bits (the claim above wino8_plan), the same bits as an utterance alone and
as a uniform (lengths = NULL) call, write nothing beyond an utterance, and sit inside the float64 bars of
test_f63_f54_conv_matches_torch_and_the_f43_form -- over all columns and over the columns beside a tile edge or an utterance's
end alone; the residual / MRF epilogues of two transform-domain launches on the smallest and the largest tile of a class; the
ragged walk beyond 64 utterances; C = 512 on small grids.
Which tile runs is never assumed: dissc_wino8_info (tests/test_wino8_plan_cpu.py) is asked under the options and batch of every
launch, and the set of instances that ran is asserted.  Every tile is reached through the launch path's own ladder: leading
sub-batches of one batch (row 0 is the longest, so Lmax is fixed), the list of rows repeated until the full batch reaches the
top tier, "small_grid" = 0 and "wino8_c64_wide" = 0 / 1 / 2; no tile needed an override.
Helpers: tests/tile_harness.py (options, poison, edge checks, launches, the sweep that FAMILY below describes this kernel to, the
bar and epilogue checks), tests/pair_harness.py (pair data, reference, launch).  Measured ratios, instances and wall time:
profiles/wino8_tiles.md."""
import pytest
import torch

import pair_harness as ph
import tile_harness as th
from tile_harness import SLOPE, lib  # noqa: F401  (lib: the module fixture)

pytestmark = pytest.mark.gpu
TILES = {64: {(2, 1, 4), (2, 4, 2), (2, 2, 4), (2, 2, 2)}, 128: {(1, 1, 4), (2, 1, 4), (2, 2, 4), (4, 2, 2)}}
TILES[256] = TILES[128]
CONV = {3: dict(wino8=2, wino8_r4=0), 4: dict(wino8=2, wino8_r4=2)}  # dissc_conv1d as F(6,3) / F(5,4)
DIRECT = dict(wino8=0)                                                 # ... on the direct kernel
ALL_SHAPES = 0o777777777
PAIR = {3: dict(wino8=1, wino8_mask=ALL_SHAPES, wino8_r4=0),           # mode 4 of dissc_respair1d: both convs as F(6,3) / F(5,4)
        4: dict(wino8=1, wino8_mask=ALL_SHAPES, wino8_r4=1, wino8_r4_mask=ALL_SHAPES)}
SHAPES = [(C, k, d) for C in (64, 128, 256) for k in (7, 11) for d in (1, 3, 5)] + [(64, 3, 1)]
MAX_ERR, K_RMS, RMS_FLOOR = 2e-5, 3.0, 1e-8  # the bars of test_f63_f54_conv_matches_torch_and_the_f43_form


def forms_of(k):
    return (3, 4) if k != 3 else (3,)


def plan(lib, C, k, d, R, B, Lmax):
    """the instance (R, NS, d, MI, NI, WPS) in force for this launch under the current options, and its widths"""
    p = lib.wino8_info(C, k, d, R, B, Lmax)
    assert p["gy"] >= 1 and 8 % p["gy"] == 0 and C % p["cpr"] == 0 and p["ot"] % p["unit"] == 0, p
    return (p["r"], p["ns"], d, p["mi"], p["ni"], p["wps"]), p


def shape_widths(lib, k, d, R):
    """(unit width, {tile widths}) of the transform shape, from the entry: the 32-, 64- and 128-column tiles of C = 64"""
    ws, units = set(), set()
    for opts in (dict(small_grid=1), dict(small_grid=0, wino8_c64_wide=1), dict(small_grid=0, wino8_c64_wide=2)):
        with th.options(lib, **opts):
            _, p = plan(lib, 64, k, d, R, 1, 1)
        ws.add(p["ot"])
        units.add(p["unit"])
    assert len(units) == 1 and (k == 3 or len(ws) == 3), (k, d, R, ws, units)
    return units.pop(), ws


def tile_settings(lib, C, k, d, R, B, nb, Lmax):
    """every way to a tile of the class at this batch: under the shipped options the largest leading sub-batch that each tier
    of the ladder takes, the full batch under "small_grid" = 0, and for C = 64 the full batch under "wino8_c64_wide" = 0 / 1 / 2.
    [(options, rows, instance)], a full batch first"""
    by_tile = {}
    for b in range(1, B + 1):
        by_tile[plan(lib, C, k, d, R, b, Lmax)[0]] = b
    out = []
    for opts in [dict(small_grid=0)] + ([dict(wino8_c64_wide=v) for v in (0, 1, 2)] if C == 64 else []):
        with th.options(lib, **opts):
            out.append((opts, B, plan(lib, C, k, d, R, B, Lmax)[0]))
    out += [({}, b, inst) for inst, b in sorted(by_tile.items(), key=lambda t: -t[1])]
    return [s for i, s in enumerate(out) if s[1:] not in [t[1:] for t in out[:i]]]  # (one launch per (rows, instance))


FAMILY = th.Family(name="eight-point", forms=forms_of, conv=CONV.get, direct=DIRECT, plan=plan, tile_settings=tile_settings,
                   shape_widths=lambda lib, C, k, d, R: shape_widths(lib, k, d, R),  # (the 32-, 64- and 128-column tiles of C = 64)
                   alone_at_256=lambda unit, w1, Lmax: (1, w1 - 1, w1, w1 + 1, 2 * w1 + 1, Lmax), lmax_cap=1600)


def sweep(lib, C, k, d):
    return th.sweep(lib, FAMILY, C, k, d)


def expected_instances(C, k, d):
    return {(R, -(-k // R), d) + t for R in forms_of(k) for t in (TILES[C] if k != 3 else {(2, 2, 4)})}


@pytest.mark.parametrize("C,k,d", SHAPES, ids=lambda v: str(v))
def test_every_tile_gives_the_same_bits(lib, C, k, d):
    res = sweep(lib, C, k, d)
    print(f"\nW8 C {C} k {k} d {d}: {res['B']} rows, lengths {res['lengths']}, instances {sorted(res['ran'])}")
    assert res["ran"] == expected_instances(C, k, d), res["ran"] ^ expected_instances(C, k, d)


@pytest.mark.parametrize("C,k,d", SHAPES, ids=lambda v: str(v))
def test_float64_bars_whole_and_at_the_edges(lib, C, k, d):
    """once per shape and form (the tiles share their bits): max error 2e-5, rms at most 3x the direct kernel's on the same
    data -- and the same over only the columns within a unit width of a tile boundary (per tile width of the shape) or of an
    utterance's end, where a wrong column is not averaged away by the interior"""
    res = sweep(lib, C, k, d)
    for R, f in res["fig"].items():
        print(f"\nW8 C {C} k {k} d {d} F({9 - R},{R}): " + th.figures_line(f))
    th.assert_float64_bars(res["fig"], MAX_ERR, K_RMS, K_RMS, RMS_FLOOR, what=("eight-point, forms by R", C, k, d))


def test_all_73_instances_ran(lib):
    """the union over the shapes (each swept once per process, here if not before): 12 transform shapes x 6 tiles + the k = 3 one"""
    ran = set().union(*(sweep(lib, *s)["ran"] for s in SHAPES))
    want = {(R, -(-k // R), d, *t) for R in (3, 4) for k in (7, 11) for d in (1, 3, 5) for t in TILES[64] | TILES[128]} | {(3, 1, 1, 2, 2, 4)}
    assert len(want) == 73 and ran == want, ran ^ want


# ---- residual / MRF epilogues of two transform-domain launches ----------------------------------------------------------
# C = 256 runs the instances of C = 128 (a call packs both convs' weights on the host): the d = 1 shapes only
EPI_SHAPES = [(C, k, d) for C in (64, 128) for k in (7, 11) for d in (1, 3, 5)] + [(256, 7, 1), (256, 11, 1)]


@pytest.mark.parametrize("C,k,d", EPI_SHAPES, ids=lambda v: str(v))
def test_residual_and_mrf_epilogues_smallest_and_largest_tile(lib, C, k, d):
    """dissc_respair1d mode 4 ("wino8_mask" / "wino8_r4_mask" put both convs on F(6,3) or on F(5,4)): conv_d (plain store) then
    conv_1 with epilogue 1..4, at the F(5,4) edge lengths of the tiles in force -- where the quads a tile shares with its
    neighbour are stored element by element and the MRF modes read, add and write `acc` -- on the smallest tile of the class (a
    small grid) and the largest ("small_grid" = 0; C = 64: the 128-column tile).  Reference and bars: tests/pair_harness.py
    (float64 per utterance, max error 1e-5, rms at most max(3x the two direct launches', 1e-6), the MRF modes bit for bit)."""
    small, large = min(TILES[C]), (4, 2, 2) if C >= 128 else (2, 4, 2)
    ran = set()
    for want, opts in ((small, dict(small_grid=1)), (large, dict(small_grid=0, wino8_c64_wide=1))):
        with th.options(lib, **opts):
            ws = {plan(lib, C, k, dd, 4, 1, 1)[1]["ot"] for dd in (d, 1)} if want == small else \
                 {plan(lib, C, k, dd, 4, 64, 100000)[1]["ot"] for dd in (d, 1)}
        lengths = [2 * max(ws) + 1] + sorted({w + e for w in ws for e in (-1, 0, 1)})
        B, ld, Lmax = len(lengths), (max(lengths) + 3) // 4 * 4, max(lengths)
        pair = ph.data(C, k, lengths, ld, seed=C + k + d)
        acc0 = torch.rand(B, C, ld, device=th.DEV)
        beyond = th.beyond_mask(lengths, ld).to(th.DEV).expand(B, C, ld)
        y0 = ph.run_pair(lib, 0, *pair, lengths, k, d)
        outs = {}

        def tile_in_force(R):
            insts = {plan(lib, C, k, dd, R, B, Lmax)[0] for dd in (d, 1)}
            assert {i[3:] for i in insts} == {want}, (insts, want, B, Lmax)
            ran.update(insts)
            return insts

        for R in (3, 4):
            outs[R] = th.pair_epilogues_every_setting(lib, 4, pair, lengths, k, d, acc0, beyond, [dict(PAIR[R], **opts)],
                                                      inspect=lambda o: tile_in_force(R))
            th.check_pair_epilogues(outs[R], pair, lengths, k, d, acc0, beyond, f"W8 pair C {C} k {k} d {d} F({9 - R},{R}) tile {want}: ", y0=y0)
        assert not torch.equal(outs[3][1], outs[4][1]), "the two forms gave the same bits: one of them did not run"
    assert {i[3:] for i in ran} == {small, large} and {i[0] for i in ran} == {3, 4}, ran


# ---- the ragged walk ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [3, 4])
def test_ragged_walk_beyond_64_utterances(lib, R):
    """ragged_tile<OT>'s prefix sum runs over 64 utterances at a time: 70 rows of C = 64 with empty utterances at the round
    boundary and elsewhere, in all four tiles of the class bit for bit, rows of the batch = the rows alone"""
    opts_list = [dict(CONV[R], small_grid=1)] + [dict(CONV[R], small_grid=0, wino8_c64_wide=v) for v in (0, 1, 2)]
    tiles = set()
    for o in opts_list:
        with th.options(lib, **o):
            tiles.add(plan(lib, 64, 7, 1, R, 70, 300)[0][3:])
    assert tiles == TILES[64], tiles
    with th.options(lib, **CONV[R]):  # (the rows alone run under these: one row of C = 64 takes the 64 x 32 tile)
        th.walk_case(lib, (64, 64, 7, 1, SLOPE), 70, opts_list, alone=[0, 63, 65, 68, 1])


# ---- C = 512 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,d", [(7, 1), (11, 5)])
def test_c512_on_small_grids(lib, k, d):
    """a 512-channel layer at B = 1 and B = 2 (the ladder stops at the 64-row tile, whose 8 row tiles divide the 8 XCDs; the
    32-row tile it used to take was refused by the launch): both forms against float64 at the bars above, the same bits at
    both batch sizes and on the 128-row tile ("small_grid" = 0)"""
    C, lengths = 512, [389, 300]
    x, w, b, ld = th.make_case(C, k, lengths, seed=512 + k)
    beyond = th.beyond_mask(lengths, ld).to(th.DEV)
    valid = ~beyond.expand(2, C, ld)
    r64 = th.reference64(x, w, b, lengths, k, d)
    err = lambda y: torch.where(valid, y.double() - r64, torch.zeros_like(r64))
    with th.options(lib, **DIRECT):
        ed = err(th.run_conv(lib, x, w, b, lengths, k, d, SLOPE))
    drms = float((ed.pow(2).sum() / valid.sum()).sqrt())
    for R in (3, 4):
        ys, tiles = [], []
        for rows, opts in ((2, {}), (1, {}), (2, dict(small_grid=0))):
            with th.options(lib, **CONV[R], **opts):
                tiles.append(plan(lib, C, k, d, R, rows, 389)[0][3:])
                y = th.run_conv(lib, x[:rows], w, b, lengths[:rows], k, d, SLOPE)
            th.check_edges(y, beyond[:rows], (R, rows, opts))
            ys.append(y)
        assert tiles == [(2, 1, 4), (2, 1, 4), (4, 2, 2)], tiles
        assert torch.equal(ys[1], ys[0][:1]) and torch.equal(ys[2], ys[0]), (R, "the tiles differ")
        e = err(ys[0])
        mx, rms = float(e.abs().max()), float((e.pow(2).sum() / valid.sum()).sqrt())
        print(f"\nW8 C 512 k {k} d {d} F({9 - R},{R}): max {mx:.2e} rms {rms:.2e} (direct {drms:.2e}, ratio {rms / drms:.2f})")
        assert mx <= MAX_ERR and float(ed.abs().max()) <= MAX_ERR and rms <= K_RMS * drms + RMS_FLOOR
