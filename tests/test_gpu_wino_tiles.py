"""conv_wino_kernel (the six Toom-Cook points as F(4,3): every k = 3 conv of the 128- and 256-channel stages, the shapes "wino8_mask"
leaves to it, the arithmetic of mode 2 of dissc_respair1d) in EVERY instance the library carries -- nine (k, d) shapes x five
(CPR, RH, TW, SHV) -- at lengths that end beside every tile's edge: all instances of a shape must give the same bits (the claim
above wino_plan), the same bits as an utterance alone and as a uniform (lengths = NULL) call, write nothing beyond an utterance,
and sit inside the float64 bars of test_toom_cook_conv_matches_torch_and_the_direct_kernel -- over all columns and over the
columns beside a tile edge or an utterance's end alone, where a wrong column is not averaged away by the interior; the residual
/ MRF epilogues of two launches in all three code forms of the epilogue, ragged last quads included, on both tiles and on the
C = 32 diagnostic instance; the ragged walk beyond 64 utterances with empty rows; C = 256 (row tile > 0 on large tiles) and C = 512.
Which instance runs is never assumed: dissc_wino_info (tests/test_wino_plan_cpu.py) is asked under the options and batch of every
launch, and the set of instances that ran is asserted against the set the rule of tests/plan_rules.py enumerates.  Every
instance is reached through the launch path's own ladder: leading sub-batches of one batch (row 0 is the longest, so Lmax is fixed)
for the small tile, the list of rows repeated until the batch reaches 96 workgroups -- and "small_grid" = 0 -- for the large one,
"wino_sv" = 0 / 1.
Helpers: tests/tile_harness.py (options, poison, data, float64 reference, edge checks and columns, launches, the sweep that FAMILY
below describes this kernel to, the bar and epilogue checks), tests/plan_rules.py (the instances the rules reach), tests/
pair_harness.py (pair data, reference, launch).  Measured ratios, instances, the teeth of the edge bar and the wall time:
profiles/wino_tiles.md."""
import pytest
import torch

import pair_harness as ph
import tile_harness as th
from plan_rules import LDS_LIMIT, wino_all_instances, wino_instances
from tile_harness import SLOPE, lib  # noqa: F401  (lib: the module fixture)

pytestmark = pytest.mark.gpu
CONV = dict(wino=2, wino8=1)    # dissc_conv1d on conv_wino_kernel ("wino8" below 2: not the eight-point kernel)
DIRECT = dict(wino=0, wino8=0)  # ... on the direct kernel
KD = [(k, d) for k in (3, 7, 11) for d in (1, 3, 5)]
# all nine shapes at C = 64 and 128; C = 256 (two row tiles of 128: mt > 0 on large tiles, 4 / 2 workgroups of a row tile per round of
# the 8 XCDs), one shape per NS; C = 512 (8 row tiles on the small tile, 4 on the large one)
SHAPES = [(C, k, d) for C in (64, 128) for k, d in KD] + [(256, 3, 3), (256, 7, 1), (256, 11, 5), (512, 3, 1), (512, 7, 5)]
# the bars of test_toom_cook_conv_matches_torch_and_the_direct_kernel: per element, and rms against the direct kernel's on the
# same columns -- over all columns, and over the edge columns alone
MAX_ERR, K_RMS, K_EDGE, RMS_FLOOR = 2e-5, 2.0, 2.0, 1e-8


def plan(lib, C, k, d, B, Lmax):
    """the instance (NS, d, CPR, RH, TW, SHV) in force for this launch under the current options, and its plan"""
    p = lib.wino_info(C, k, d, B, Lmax)
    assert p["gy"] >= 1 and 8 % p["gy"] == 0 and C % p["cpr"] == 0 and p["ot"] % p["unit"] == 0 and p["lds_bytes"] <= LDS_LIMIT, p
    return (p["ns"], p["dilation"], p["cpr"], p["rh"], p["tw"], p["shv"]), p


def shape_widths(lib, C, k, d):
    """(unit width, {tile widths}) of the shape at this C, from the entry: the small-grid tile and the large one"""
    ps = []
    for sg in (1, 0):
        with th.options(lib, small_grid=sg):
            ps.append(plan(lib, C, k, d, 1, 1)[1])
    assert ps[0]["unit"] == ps[1]["unit"] and (C == 32 or ps[1]["ot"] > ps[0]["ot"]), ps
    return ps[0]["unit"], {p["ot"] for p in ps}


def tile_settings(lib, C, k, d, B, nb, Lmax):
    """every way to an instance of the shape at this batch, per "wino_sv": the full batch and the largest leading sub-batch that
    each tier of the ladder takes under the shipped "small_grid", and the first nb rows under "small_grid" = 0.
    [(options, rows, instance)], a full batch first, one launch per (rows, instance)"""
    out = []
    for sv in (1, 0):
        with th.options(lib, wino_sv=sv):
            out.append((dict(wino_sv=sv), B, plan(lib, C, k, d, B, Lmax)[0]))
            by_inst = {}
            for b in range(1, B + 1):
                by_inst[plan(lib, C, k, d, b, Lmax)[0]] = b
            out += [(dict(wino_sv=sv), b, inst) for inst, b in sorted(by_inst.items(), key=lambda t: -t[1])]
        with th.options(lib, wino_sv=sv, small_grid=0):
            out.append((dict(wino_sv=sv, small_grid=0), nb, plan(lib, C, k, d, nb, Lmax)[0]))
    return [s for i, s in enumerate(out) if s[1:] not in [t[1:] for t in out[:i]]]


FAMILY = th.Family(name="F(4,3)", forms=lambda k: (None,), conv=lambda form: CONV, direct=DIRECT, lmax_cap=2 * 512 + 1,
                   plan=lambda lib, C, k, d, form, B, Lmax: plan(lib, C, k, d, B, Lmax),
                   shape_widths=lambda lib, C, k, d, form: shape_widths(lib, C, k, d),
                   tile_settings=lambda lib, C, k, d, form, B, nb, Lmax: tile_settings(lib, C, k, d, B, nb, Lmax),
                   alone_at_256=lambda unit, w1, Lmax: (1, unit + 1, w1 - 1, w1, w1 + 1, 2 * w1 + 1, Lmax))


def sweep(lib, C, k, d):
    return th.sweep(lib, FAMILY, C, k, d)


@pytest.mark.parametrize("C,k,d", SHAPES, ids=lambda v: str(v))
def test_every_instance_gives_the_same_bits(lib, C, k, d):
    res = sweep(lib, C, k, d)
    unit, widths = res["geo"][None]
    print(f"\nW6 C {C} k {k} d {d}: unit {unit}, widths {widths}, {res['B']} rows, lengths {res['lengths']}, instances {sorted(res['ran'])}")
    assert res["ran"] == wino_instances(C, k, d), res["ran"] ^ wino_instances(C, k, d)


@pytest.mark.parametrize("C,k,d", SHAPES, ids=lambda v: str(v))
def test_float64_bars_whole_and_at_the_edges(lib, C, k, d):
    """once per shape (the instances share their bits): max error 2e-5, rms at most 2x the direct kernel's on the same data --
    and the same over only the columns within a unit width of a tile boundary (per tile width of the shape) or of an
    utterance's end"""
    figs = sweep(lib, C, k, d)["fig"]
    print(f"\nW6 C {C} k {k} d {d}: " + th.figures_line(figs[None]))
    th.assert_float64_bars(figs, MAX_ERR, K_RMS, K_EDGE, RMS_FLOOR, edge_max=MAX_ERR, what=("F(4,3)", C, k, d))


def test_all_45_instances_ran(lib):
    """the union over the shapes (each swept once per process, here if not before) is all the library carries: tests/
    test_wino_plan_cpu.py holds the instantiations named in the library to the same set (tests/plan_rules.py)"""
    ran = set().union(*(sweep(lib, *s)["ran"] for s in SHAPES))
    assert len(wino_all_instances()) == 45 and ran == wino_all_instances(), ran ^ wino_all_instances()


# ---- residual / MRF epilogues of two conv_wino launches -----------------------------------------------------------------
# the second launch (dilation 1) carries the epilogue: k = 3 is its D = 1 form, k = 7 (D = 3) the output-tile form, k = 11 (D = 4)
# the D % 4 == 0 form
EPI_SHAPES = [(C, k, d) for C in (32, 64, 128) for k, d in ((3, 5), (7, 3), (11, 1))]


@pytest.mark.parametrize("C,k,d", EPI_SHAPES, ids=lambda v: str(v))
def test_residual_and_mrf_epilogues_both_tiles(lib, C, k, d):
    """dissc_respair1d mode 2: conv_d (plain store) then conv_1 with epilogue 1..4, at the edge lengths of both tiles of both
    convs + 2 (so that len % 4 takes all four values: the ragged last quad goes through epi_store1 next to the prefetched
    residual quads) -- on the small tile, the large one ("small_grid" = 0) under "wino_sv" = 1 / 0, the same bits in all; C = 32 is
    the one diagnostic instance.  Reference and bars: tests/pair_harness.py (float64 per utterance, max error 1e-5, rms at most
    max(3x the two direct launches', 1e-6), the MRF modes bit for bit), accumulator and output untouched beyond each length."""
    ws = set().union(*(shape_widths(lib, C, k, dd)[1] for dd in (d, 1)))
    lengths = [2 * max(ws) + 1] + sorted({w + e for w in ws for e in (-1, 0, 1, 2)} | {3, 6})
    assert {n % 4 for n in lengths} == {0, 1, 2, 3} and max(lengths) <= 2 * 512 + 1
    B, ld, Lmax = len(lengths), (max(lengths) + 3) // 4 * 4, max(lengths)
    pair = ph.data(C, k, lengths, ld, seed=C + k + d)
    acc0 = torch.rand(B, C, ld, device=th.DEV)
    beyond = th.beyond_mask(lengths, ld).to(th.DEV).expand(B, C, ld)
    y0 = ph.run_pair(lib, 0, *pair, lengths, k, d)
    ran = set()

    def instances_in_force(opts):
        insts = {plan(lib, C, k, dd, B, Lmax)[0] for dd in (d, 1)}
        assert {i[4] for i in insts} == {2 if (opts["small_grid"] == 0 and C != 32) else 1}, (insts, opts)
        ran.update(insts)
        return insts

    first = th.pair_epilogues_every_setting(lib, 2, pair, lengths, k, d, acc0, beyond, inspect=instances_in_force,
                                            settings=(dict(small_grid=1), dict(small_grid=0, wino_sv=1), dict(small_grid=0, wino_sv=0)))
    assert ran == set().union(*(wino_instances(C, k, dd) for dd in (d, 1))) if C != 32 else ran == {(-(-k // 3), dd, 16, 1, 1, 0) for dd in (d, 1)}, ran
    th.check_pair_epilogues(first, pair, lengths, k, d, acc0, beyond, f"W6 pair C {C} k {k} d {d}: instances {sorted(ran)}, ", y0=y0)


# ---- the ragged walk ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", ["small", "large"])
def test_ragged_walk_beyond_64_utterances(lib, tile):
    """ragged_tile<OT>'s prefix sum runs over 64 utterances at a time: 70 rows of C = 64, k = 3 at mixed edge lengths of the tile in
    force, with empty utterances in the middle, at the round boundary (index 64) and at the end -- every row of the batch = the
    row alone, nothing beyond a length.  The tile follows from the ladder: 70 rows of at most one large tile's width stay below 96
    workgroups, 70 rows of up to three do not."""
    C, k, d, B = 64, 3, 1, 70
    unit, ws = shape_widths(lib, C, k, d)
    w1, w2 = min(ws), max(ws)
    top = w2 if tile == "small" else 2 * w2 + 1
    pool = sorted({1, 2, 3, unit - 1, unit + 1} | {m * wd + e for wd in ws for m in (1, 2) for e in (-1, 0, 1) if m * wd + e <= top})
    lengths = [top] + [pool[(7 * i) % len(pool)] for i in range(1, B)]
    for i in (3, 31, 32, 64, B - 1):
        lengths[i] = 0
    with th.options(lib, **CONV):
        inst, p = plan(lib, C, k, d, B, top)
    assert inst == (1, 1, 16, 1, 1 if tile == "small" else 2, 0) and p["gx"] == (2 if tile == "small" else 3), (inst, p)
    x, w, b, ld = th.make_case(C, k, lengths, seed=70 + len(tile))
    beyond = th.beyond_mask(lengths, ld).to(th.DEV)
    with th.options(lib, **CONV):
        y = th.run_conv(lib, x, w, b, lengths, k, d, SLOPE)
        th.check_edges(y, beyond, tile)
        for i, n in enumerate(lengths):
            if n == 0:
                continue
            one = th.run_conv(lib, x[i:i + 1].clone(), w, b, [n], k, d, SLOPE)
            assert torch.equal(one[0, :, :n], y[i, :, :n]), (i, n)
    with th.options(lib, **DIRECT):
        yd = th.run_conv(lib, x, w, b, lengths, k, d, SLOPE)
    assert not torch.equal(y, yd), "the direct kernel ran"
    r64 = th.reference64(x, w, b, lengths, k, d)
    assert float(torch.where(beyond.expand_as(y), torch.zeros_like(r64), y.double() - r64).abs().max()) <= MAX_ERR
