"""conv_wino_kernel (the six Toom-Cook points as F(4,3): every k = 3 conv of the 128- and 256-channel stages, the shapes "wino8_mask"
leaves to it, the arithmetic of mode 2 of dissc_respair1d) in EVERY instance the library carries -- nine (k, d) shapes x five
(CPR, RH, TW, SHV) -- at lengths that end beside every tile's edge: all instances of a shape must give the same bits (the claim
above wino_plan), the same bits as an utterance alone and as a uniform (lengths = NULL) call, write nothing beyond an utterance,
and sit inside the float64 bars of test_toom_cook_conv_matches_torch_and_the_direct_kernel -- over all columns and over the
columns beside a tile edge or an utterance's end alone, where a wrong column is not averaged away by the interior; the residual
/ MRF epilogues of two launches in all three code forms of the epilogue, ragged last quads included, on both tiles and on the
C = 32 diagnostic instance; the ragged walk beyond 64 utterances with empty rows; C = 256 (row tile > 0 on large tiles) and C = 512.
Which instance runs is never assumed: dissc_wino_info (tests/test_wino_plan_cpu.py) is asked under the options and batch of every
launch, and the set of instances that ran is asserted against the set that file's rule enumerates.  Every instance is reached
through the launch path's own ladder: leading sub-batches of one batch (row 0 is the longest, so Lmax is fixed) for the small
tile, the list of rows repeated until the batch reaches 96 workgroups -- and "small_grid" = 0 -- for the large one, "wino_sv" = 0 / 1.
Helpers: tests/test_gpu_direct_conv_tiles.py (options, poison, edge checks, launch), tests/test_gpu_wino8_tiles.py (data, float64
reference, uniform launch, edge columns), tests/pair_harness.py (pair data, reference, launch).  Measured ratios, instances, the
teeth of the edge bar and the wall time: profiles/wino_tiles.md."""
import functools

import pytest
import torch

import pair_harness as ph
import test_gpu_direct_conv_tiles as dt
import test_gpu_wino8_tiles as w8
import test_wino_plan_cpu as wp

pytestmark = pytest.mark.gpu
DEV, SLOPE = dt.DEV, dt.SLOPE
CONV = dict(wino=2, wino8=1)    # dissc_conv1d on conv_wino_kernel ("wino8" below 2: not the eight-point kernel)
DIRECT = dict(wino=0, wino8=0)  # ... on the direct kernel
KD = [(k, d) for k in (3, 7, 11) for d in (1, 3, 5)]
# all nine shapes at C = 64 and 128; C = 256 (two row tiles of 128: mt > 0 on large tiles, 4 / 2 workgroups of a row tile per round of
# the 8 XCDs), one shape per NS; C = 512 (8 row tiles on the small tile, 4 on the large one)
SHAPES = [(C, k, d) for C in (64, 128) for k, d in KD] + [(256, 3, 3), (256, 7, 1), (256, 11, 5), (512, 3, 1), (512, 7, 5)]
# the bars of test_toom_cook_conv_matches_torch_and_the_direct_kernel: per element, and rms against the direct kernel's on the
# same columns -- over all columns, and over the edge columns alone
MAX_ERR, K_RMS, K_EDGE, RMS_FLOOR = 2e-5, 2.0, 2.0, 1e-8


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import _lib
    return _lib


def plan(lib, C, k, d, B, Lmax):
    """the instance (NS, d, CPR, RH, TW, SHV) in force for this launch under the current options, and its plan"""
    p = lib.wino_info(C, k, d, B, Lmax)
    assert p["gy"] >= 1 and 8 % p["gy"] == 0 and C % p["cpr"] == 0 and p["ot"] % p["unit"] == 0 and p["lds_bytes"] <= wp.LDS_LIMIT, p
    return (p["ns"], p["dilation"], p["cpr"], p["rh"], p["tw"], p["shv"]), p


def shape_widths(lib, C, k, d):
    """(unit width, {tile widths}) of the shape at this C, from the entry: the small-grid tile and the large one"""
    ps = []
    for sg in (1, 0):
        with dt.options(lib, small_grid=sg):
            ps.append(plan(lib, C, k, d, 1, 1)[1])
    assert ps[0]["unit"] == ps[1]["unit"] and (C == 32 or ps[1]["ot"] > ps[0]["ot"]), ps
    return ps[0]["unit"], {p["ot"] for p in ps}


def tile_settings(lib, C, k, d, B, nb, Lmax):
    """every way to an instance of the shape at this batch, per "wino_sv": the full batch and the largest leading sub-batch that
    each tier of the ladder takes under the shipped "small_grid", and the first nb rows under "small_grid" = 0.
    [(options, rows, instance)], a full batch first, one launch per (rows, instance)"""
    out = []
    for sv in (1, 0):
        with dt.options(lib, wino_sv=sv):
            out.append((dict(wino_sv=sv), B, plan(lib, C, k, d, B, Lmax)[0]))
            by_inst = {}
            for b in range(1, B + 1):
                by_inst[plan(lib, C, k, d, b, Lmax)[0]] = b
            out += [(dict(wino_sv=sv), b, inst) for inst, b in sorted(by_inst.items(), key=lambda t: -t[1])]
        with dt.options(lib, wino_sv=sv, small_grid=0):
            out.append((dict(wino_sv=sv, small_grid=0), nb, plan(lib, C, k, d, nb, Lmax)[0]))
    return [s for i, s in enumerate(out) if s[1:] not in [t[1:] for t in out[:i]]]


def rows_for(lib, C, k, d, rows):
    """the list of rows repeated until the full batch takes the large tile by the ladder itself (96 workgroups), and no further"""
    for reps in (1, 2, 3, 4):
        with dt.options(lib, small_grid=0):
            top = plan(lib, C, k, d, reps * len(rows), max(rows))[0]
        if plan(lib, C, k, d, reps * len(rows), max(rows))[0] == top:
            return rows * reps
    raise AssertionError(("the large tile is out of the ladder's reach", C, k, d))


@functools.lru_cache(maxsize=None)
def sweep(lib, C, k, d):
    """One batch per (C, k, d), shared by every instance: the edge lengths of both tile widths, longest first.  The batch through
    every tile setting, every utterance alone (C >= 256: a subset at the edge lengths -- its instances are those of C = 128, where
    every row runs alone, and a call packs the weights on the host), two uniform calls; all bit-identical on an utterance's
    columns, the sentinel untouched beyond.  Returns the instances that ran and the error figures against float64 (not asserted
    here)."""
    pad = (k - 1) * d // 2
    unit, ws = shape_widths(lib, C, k, d)
    base = ({0, 1, 2, pad, pad + 1, unit - 1, unit + 1} | {m * wd + e for wd in ws for m in (1, 2) for e in (-1, 0, 1)})
    # the longest first (Lmax is that of every leading sub-batch), then the edges of the small tile: the rows the small-grid tier,
    # which takes the fewest rows, sees in a batch
    narrow = {m * min(ws) + e for m in (1, 2) for e in (-1, 0, 1)}
    base = [max(base)] + sorted(base - {max(base)}, key=lambda n: (n not in narrow, n))
    lengths = rows_for(lib, C, k, d, base)
    nb, B, Lmax = len(base), len(lengths), max(lengths)
    assert lengths[0] == Lmax == 2 * max(ws) + 1 and Lmax <= 2 * 512 + 1
    x, w, b, ld = w8.make_case(C, k, base, seed=1000 * C + 10 * k + d)
    x = x.repeat(B // nb, 1, 1)  # (repeated rows carry the same data)
    beyond = dt.beyond_mask(lengths, ld).to(DEV)
    valid = ~beyond.expand(B, C, ld)
    r64 = w8.reference64(x, w, b, lengths, k, d)

    def errors(y, mask):
        e = torch.where(mask, y.double() - r64, torch.zeros_like(r64))
        return float(e.abs().max()), float((e.pow(2).sum() / mask.sum()).sqrt())

    with dt.options(lib, **DIRECT):
        yd = dt.run_conv(lib, x, w, b, lengths, k, d, SLOPE)
    dt.check_edges(yd, beyond, "direct")
    res = dict(lengths=base, B=B, unit=unit, widths=sorted(ws), ran=set())
    first = first_inst = None
    for opts, rows, inst in tile_settings(lib, C, k, d, B, nb, Lmax):
        with dt.options(lib, **CONV, **opts):
            assert plan(lib, C, k, d, rows, Lmax)[0] == inst
            y = dt.run_conv(lib, x[:rows], w, b, lengths[:rows], k, d, SLOPE)
        dt.check_edges(y, beyond[:rows], (opts, rows, inst))
        if first is None:
            assert rows == B
            first, first_inst = y, inst
        assert torch.equal(y, first[:rows]), f"instance {inst[2:]} ({opts}, {rows} rows) differs from instance {first_inst[2:]}"
        res["ran"].add(inst)
    for i in range(nb, B):  # a repeated row = its original
        assert torch.equal(first[i], first[i % nb]), i
    assert not torch.equal(first, yd), "the direct kernel ran"
    w1 = min(ws)
    alone = range(nb) if C < 256 else [i for i, n in enumerate(base) if n in (1, unit + 1, w1 - 1, w1, w1 + 1, 2 * w1 + 1, Lmax)]
    with dt.options(lib, **CONV):
        for i in alone:
            n = lengths[i]
            if n == 0:
                continue
            res["ran"].add(plan(lib, C, k, d, 1, n)[0])
            one = dt.run_conv(lib, x[i:i + 1].clone(), w, b, [n], k, d, SLOPE)
            dt.check_edges(one, beyond[i:i + 1], ("alone", n))
            assert torch.equal(one[0, :, :n], first[i, :, :n]), ("alone", n)
        for n in (min(ws) + 1, 2 * max(ws) - 1):  # uniform: two rows of that length, lengths = NULL
            i = lengths.index(n)
            res["ran"].add(plan(lib, C, k, d, 2, n)[0])
            two = w8.run_uniform(lib, x[i:i + 1].expand(2, C, ld).contiguous(), w, b, n, k, d)
            dt.check_edges(two, beyond[i:i + 1].expand(2, 1, ld), ("uniform", n))
            assert torch.equal(two[0, :, :n], first[i, :, :n]) and torch.equal(two[1], two[0]), ("uniform", n)
    fig = dict(all=errors(first, valid), direct=errors(yd, valid), edge=[])
    for wd in sorted(ws):  # per tile width
        edge = w8.edge_mask(lengths, ld, unit, [wd]).to(DEV).expand(B, C, ld) & valid
        assert 0 < int(edge.sum()) <= int(valid.sum())
        fig["edge"].append((wd, float(edge.sum()) / float(valid.sum()), errors(first, edge), errors(yd, edge)))
    res["fig"] = fig
    return res


@pytest.mark.parametrize("C,k,d", SHAPES, ids=lambda v: str(v))
def test_every_instance_gives_the_same_bits(lib, C, k, d):
    res = sweep(lib, C, k, d)
    print(f"\nW6 C {C} k {k} d {d}: unit {res['unit']}, widths {res['widths']}, {res['B']} rows, lengths {res['lengths']}, "
          f"instances {sorted(res['ran'])}")
    assert res["ran"] == wp.instances(C, k, d), res["ran"] ^ wp.instances(C, k, d)


@pytest.mark.parametrize("C,k,d", SHAPES, ids=lambda v: str(v))
def test_float64_bars_whole_and_at_the_edges(lib, C, k, d):
    """once per shape (the instances share their bits): max error 2e-5, rms at most 2x the direct kernel's on the same data --
    and the same over only the columns within a unit width of a tile boundary (per tile width of the shape) or of an
    utterance's end"""
    f = sweep(lib, C, k, d)["fig"]
    (mx, rms), (dmx, drms) = f["all"], f["direct"]
    print(f"\nW6 C {C} k {k} d {d}: max {mx:.2e} rms {rms:.2e} (direct {dmx:.2e} / {drms:.2e}, ratio {rms / drms:.2f}); edge columns of "
          + ", ".join(f"w {wd} ({100 * sh:.0f} %): max {e[0]:.2e} rms {e[1]:.2e} ratio {e[1] / de[1]:.2f}" for wd, sh, e, de in f["edge"]))
    bad = []
    if not (mx <= MAX_ERR and dmx <= MAX_ERR):
        bad.append(("max", mx, dmx))
    if not rms <= K_RMS * drms + RMS_FLOOR:
        bad.append(("rms", rms, drms))
    for wd, _, (emx, erms), (_, derms) in f["edge"]:
        if not (emx <= MAX_ERR and erms <= K_EDGE * derms + RMS_FLOOR):
            bad.append(("edge", wd, emx, erms, derms))
    assert not bad, bad


def test_all_45_instances_ran(lib):
    """the union over the shapes (each swept once per process, here if not before) is all the library carries: tests/
    test_wino_plan_cpu.py holds the instantiations named in the library to the same set"""
    ran = set().union(*(sweep(lib, *s)["ran"] for s in SHAPES))
    assert len(wp.all_instances()) == 45 and ran == wp.all_instances(), ran ^ wp.all_instances()


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
    x, w1, b1, w2, b2 = ph.data(C, k, lengths, ld, seed=C + k + d)
    ref = ph.reference(x, w1, b1, w2, b2, lengths, k, d)
    acc0 = torch.rand(B, C, ld, device=DEV)
    beyond = dt.beyond_mask(lengths, ld).to(DEV).expand(B, C, ld)
    y0 = ph.run_pair(lib, 0, x, w1, b1, w2, b2, lengths, k, d)
    first, ran = None, set()
    for opts in (dict(small_grid=1), dict(small_grid=0, wino_sv=1), dict(small_grid=0, wino_sv=0)):
        with dt.options(lib, **opts):
            insts = {plan(lib, C, k, dd, B, Lmax)[0] for dd in (d, 1)}
            assert {i[4] for i in insts} == {2 if (opts["small_grid"] == 0 and C != 32) else 1}, (insts, opts)
            ran |= insts
            outs = {epi: ph.run_pair(lib, 2, x, w1, b1, w2, b2, lengths, k, d, epi=epi, acc=None if epi == 1 else acc0)
                    for epi in (1, 2, 3, 4)}
        for epi, o in outs.items():
            untouched = torch.full_like(o, -7.0) if epi == 1 else acc0
            assert torch.equal(torch.where(beyond, o, untouched), untouched), (opts, epi, "wrote beyond an utterance")
            assert torch.isfinite(torch.where(beyond, torch.zeros_like(o), o)).all(), (opts, epi, "read beyond an utterance")
        if first is None:
            first = outs
        for epi in outs:
            assert torch.equal(outs[epi], first[epi]), (opts, epi, "the tiles differ")
    assert ran == set().union(*(wp.instances(C, k, dd) for dd in (d, 1))) if C != 32 else ran == {(-(-k // 3), dd, 16, 1, 1, 0) for dd in (d, 1)}, ran
    y = first[1]
    e = torch.where(beyond, torch.zeros_like(ref), y.double() - ref)
    e0 = torch.where(beyond, torch.zeros_like(ref), y0.double() - ref)
    worst, rms, rms0 = float(e.abs().max()), float(e.pow(2).mean().sqrt()), float(e0.pow(2).mean().sqrt())
    print(f"\nW6 pair C {C} k {k} d {d}: instances {sorted(ran)}, max err {worst:.2e}, rms {rms:.2e} (direct launches {rms0:.2e}), lengths {lengths}")
    assert not torch.equal(y, y0), "the direct launches ran"
    assert worst <= 1e-5 and rms <= max(3.0 * rms0, 1e-6)
    for i, n in enumerate(lengths):
        for epi in (2, 3, 4):
            want = y[i, :, :n] if epi == 2 else acc0[i, :, :n] + y[i, :, :n]
            if epi == 4:
                want = (want.cpu() / 3.0).to(DEV)  # a true division, like the reference's xs / num_kernels
            assert torch.equal(first[epi][i, :, :n], want), (epi, i, n)


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
    with dt.options(lib, **CONV):
        inst, p = plan(lib, C, k, d, B, top)
    assert inst == (1, 1, 16, 1, 1 if tile == "small" else 2, 0) and p["gx"] == (2 if tile == "small" else 3), (inst, p)
    x, w, b, ld = w8.make_case(C, k, lengths, seed=70 + len(tile))
    beyond = dt.beyond_mask(lengths, ld).to(DEV)
    with dt.options(lib, **CONV):
        y = dt.run_conv(lib, x, w, b, lengths, k, d, SLOPE)
        dt.check_edges(y, beyond, tile)
        for i, n in enumerate(lengths):
            if n == 0:
                continue
            one = dt.run_conv(lib, x[i:i + 1].clone(), w, b, [n], k, d, SLOPE)
            assert torch.equal(one[0, :, :n], y[i, :, :n]), (i, n)
    with dt.options(lib, **DIRECT):
        yd = dt.run_conv(lib, x, w, b, lengths, k, d, SLOPE)
    assert not torch.equal(y, yd), "the direct kernel ran"
    r64 = w8.reference64(x, w, b, lengths, k, d)
    assert float(torch.where(beyond.expand_as(y), torch.zeros_like(r64), y.double() - r64).abs().max()) <= MAX_ERR
