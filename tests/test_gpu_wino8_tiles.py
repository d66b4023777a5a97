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
Helpers: tests/test_gpu_direct_conv_tiles.py (options, poison, edge checks, launch), tests/pair_harness.py (pair data, reference,
launch).  Measured ratios, instances and wall time: profiles/wino8_tiles.md."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import pair_harness as ph
import test_gpu_direct_conv_tiles as dt

pytestmark = pytest.mark.gpu
DEV, SENTINEL, SLOPE = dt.DEV, dt.SENTINEL, dt.SLOPE
TILES = {64: {(2, 1, 4), (2, 4, 2), (2, 2, 4), (2, 2, 2)}, 128: {(1, 1, 4), (2, 1, 4), (2, 2, 4), (4, 2, 2)}}
TILES[256] = TILES[128]
CONV = {3: dict(wino8=2, wino8_r4=0), 4: dict(wino8=2, wino8_r4=2)}  # dissc_conv1d as F(6,3) / F(5,4)
DIRECT = dict(wino8=0)                                                 # ... on the direct kernel
ALL_SHAPES = 0o777777777
PAIR = {3: dict(wino8=1, wino8_mask=ALL_SHAPES, wino8_r4=0),           # mode 4 of dissc_respair1d: both convs as F(6,3) / F(5,4)
        4: dict(wino8=1, wino8_mask=ALL_SHAPES, wino8_r4=1, wino8_r4_mask=ALL_SHAPES)}
SHAPES = [(C, k, d) for C in (64, 128, 256) for k in (7, 11) for d in (1, 3, 5)] + [(64, 3, 1)]
MAX_ERR, K_RMS, RMS_FLOOR = 2e-5, 3.0, 1e-8  # the bars of test_f63_f54_conv_matches_torch_and_the_f43_form


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import _lib
    return _lib


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
        with dt.options(lib, **opts):
            _, p = plan(lib, 64, k, d, R, 1, 1)
        ws.add(p["ot"])
        units.add(p["unit"])
    assert len(units) == 1 and (k == 3 or len(ws) == 3), (k, d, R, ws, units)
    return units.pop(), ws


def make_case(C, k, lengths, seed):
    """x uniform in [-1, 1) with NaN beyond each length, weights and bias at the magnitudes of the bars' own test"""
    g = torch.Generator().manual_seed(seed)
    B, ld = len(lengths), (max(lengths) + 3) // 4 * 4
    x = torch.rand(B, C, ld, generator=g) * 2 - 1
    for i, n in enumerate(lengths):
        x[i, :, n:] = float("nan")  # never read
    w = (torch.rand(C, C, k, generator=g) * 2 - 1) * 0.025 * (256 / C) ** 0.5
    b = torch.rand(C, generator=g) * 0.2 - 0.1
    return x.to(DEV), w, b, ld


def reference64(x, w, b, lengths, k, d):
    """float64 F.conv1d on leaky_relu(x), every utterance on its own samples: zeros beyond a length are the "same" padding"""
    xz = torch.nan_to_num(x.double(), nan=0.0)
    return F.conv1d(F.leaky_relu(xz, SLOPE), w.double().to(x.device), b.double().to(x.device), padding=(k - 1) * d // 2, dilation=d)


def run_uniform(lib, x, w, b, n, k, d):
    """dissc_conv1d with lengths = NULL: every row has n columns"""
    B, C, ld = x.shape
    y = torch.full((B, C, ld), SENTINEL, device=DEV)
    lib.check(lib.lib.dissc_conv1d(x.data_ptr(), w.contiguous().data_ptr(), b.contiguous().data_ptr(), y.data_ptr(), None,
                                   B, C, C, k, d, ld, ld, n, ctypes.c_float(SLOPE), None), "dissc_conv1d")
    return y


def tile_settings(lib, C, k, d, R, B, Lmax):
    """every way to a tile of the class at this batch: under the shipped options the largest leading sub-batch that each tier
    of the ladder takes, the full batch under "small_grid" = 0, and for C = 64 the full batch under "wino8_c64_wide" = 0 / 1 / 2.
    [(options, rows, instance)], a full batch first"""
    by_tile = {}
    for b in range(1, B + 1):
        by_tile[plan(lib, C, k, d, R, b, Lmax)[0]] = b
    out = []
    for opts in [dict(small_grid=0)] + ([dict(wino8_c64_wide=v) for v in (0, 1, 2)] if C == 64 else []):
        with dt.options(lib, **opts):
            out.append((opts, B, plan(lib, C, k, d, R, B, Lmax)[0]))
    out += [({}, b, inst) for inst, b in sorted(by_tile.items(), key=lambda t: -t[1])]
    return [s for i, s in enumerate(out) if s[1:] not in [t[1:] for t in out[:i]]]  # (one launch per (rows, instance))


def rows_for(lib, C, k, d, rows):
    """the list of rows repeated until the full batch reaches the top tier by the ladder itself (C = 64 needs 192 tiles)"""
    Lmax = max(rows)
    for reps in (1, 2, 3, 4):
        ok = True
        for R in forms_of(k):
            with dt.options(lib, small_grid=0):
                top = plan(lib, C, k, d, R, reps * len(rows), Lmax)[0]
            ok = ok and plan(lib, C, k, d, R, reps * len(rows), Lmax)[0] == top
        if ok:
            return rows * reps
    raise AssertionError(("the ladder's top tier is out of reach", C, k, d))


def edge_mask(lengths, ld, unit, widths):
    """columns within one unit width of a boundary of the tiles of these widths or of the utterance's end"""
    c = torch.arange(ld)
    near = torch.zeros(ld, dtype=torch.bool)
    for w in widths:
        near |= (c % w < unit) | (c % w >= w - unit)
    m = torch.zeros(len(lengths), 1, ld, dtype=torch.bool)
    for i, n in enumerate(lengths):
        m[i, 0, :n] = near[:n] | (c[:n] >= n - unit)
    return m


@functools.lru_cache(maxsize=None)
def sweep(lib, C, k, d):
    """One batch per (C, k, d), shared by both forms and every tile: the edge lengths of every tile width either form has,
    longest first.  Per form: the batch through every tile setting, every utterance alone (C = 256: a subset -- its instances
    are those of C = 128, where every row runs alone, and a call packs 16 MB of weights on the host), two uniform calls; all
    bit-identical on an utterance's columns, the sentinel untouched beyond.  Returns the instances that ran and the error figures
    against float64 (not asserted here)."""
    pad = (k - 1) * d // 2
    geo = {R: shape_widths(lib, k, d, R) for R in forms_of(k)}
    widths = set().union(*(ws for _, ws in geo.values()))
    base = ({0, 1, 2, pad, pad + 1} | {u + e for u, _ in geo.values() for e in (-1, 1)} |
            {m * wd + e for wd in widths for m in (1, 2) for e in (-1, 0, 1)})
    # the longest first (Lmax is that of every leading sub-batch), then the edges of each form's narrowest tile: the rows the
    # small-grid tiers, which take the fewest rows, see in a batch
    narrow = {m * min(ws) + e for _, ws in geo.values() for m in (1, 2) for e in (-1, 0, 1)}
    base = [max(base)] + sorted(base - {max(base)}, key=lambda n: (n not in narrow, n))
    lengths = rows_for(lib, C, k, d, base)
    nb, B, Lmax = len(base), len(lengths), max(lengths)
    assert lengths[0] == Lmax == 2 * max(widths) + 1 and Lmax <= 1600
    x, w, b, ld = make_case(C, k, base, seed=1000 * C + 10 * k + d)
    x = x.repeat(B // nb, 1, 1)  # (repeated rows carry the same data)
    beyond = dt.beyond_mask(lengths, ld).to(DEV)
    valid = ~beyond.expand(B, C, ld)
    r64 = reference64(x, w, b, lengths, k, d)

    def errors(y, mask):
        e = torch.where(mask, y.double() - r64, torch.zeros_like(r64))
        return float(e.abs().max()), float((e.pow(2).sum() / mask.sum()).sqrt())

    with dt.options(lib, **DIRECT):
        yd = dt.run_conv(lib, x, w, b, lengths, k, d, SLOPE)
    dt.check_edges(yd, beyond, "direct")
    res = dict(lengths=base, B=B, ran=set(), fig={})
    for R in forms_of(k):
        unit, ws = geo[R]
        first = first_inst = None
        for opts, rows, inst in tile_settings(lib, C, k, d, R, B, Lmax):
            with dt.options(lib, **CONV[R], **opts):
                assert plan(lib, C, k, d, R, rows, Lmax)[0] == inst
                y = dt.run_conv(lib, x[:rows], w, b, lengths[:rows], k, d, SLOPE)
            dt.check_edges(y, beyond[:rows], (R, opts, rows, inst))
            if first is None:
                assert rows == B
                first, first_inst = y, inst
            assert torch.equal(y, first[:rows]), f"F({9 - R},{R}) tile {inst[3:]} ({opts}, {rows} rows) differs from tile {first_inst[3:]}"
            res["ran"].add(inst)
        for i in range(nb, B):  # a repeated row = its original
            assert torch.equal(first[i], first[i % nb]), (R, i)
        assert not torch.equal(first, yd), "the direct kernel ran"
        w1 = min(ws)
        alone = range(nb) if C < 256 else [i for i, n in enumerate(base) if n in (1, w1 - 1, w1, w1 + 1, 2 * w1 + 1, Lmax)]
        with dt.options(lib, **CONV[R]):
            for i in alone:
                n = lengths[i]
                if n == 0:
                    continue
                res["ran"].add(plan(lib, C, k, d, R, 1, n)[0])
                one = dt.run_conv(lib, x[i:i + 1].clone(), w, b, [n], k, d, SLOPE)
                dt.check_edges(one, beyond[i:i + 1], (R, "alone", n))
                assert torch.equal(one[0, :, :n], first[i, :, :n]), (R, "alone", n)
            for n in (min(ws) + 1, 2 * max(ws) - 1):  # uniform: two rows of that length, lengths = NULL
                i = lengths.index(n)
                res["ran"].add(plan(lib, C, k, d, R, 2, n)[0])
                two = run_uniform(lib, x[i:i + 1].expand(2, C, ld).contiguous(), w, b, n, k, d)
                dt.check_edges(two, beyond[i:i + 1].expand(2, 1, ld), (R, "uniform", n))
                assert torch.equal(two[0, :, :n], first[i, :, :n]) and torch.equal(two[1], two[0]), (R, "uniform", n)
        fig = dict(all=errors(first, valid), direct=errors(yd, valid), edge=[])
        for wd in sorted(ws):  # per tile width: the 32-column tiles of d = 3 / 5 are one or two units wide, all of them edge
            edge = edge_mask(lengths, ld, unit, [wd]).to(DEV).expand(B, C, ld) & valid
            assert 0 < int(edge.sum()) <= int(valid.sum())
            fig["edge"].append((wd, float(edge.sum()) / float(valid.sum()), errors(first, edge), errors(yd, edge)))
        res["fig"][R] = fig
    return res


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
    bad = []
    for R, f in res["fig"].items():
        (mx, rms), (dmx, drms) = f["all"], f["direct"]
        print(f"\nW8 C {C} k {k} d {d} F({9 - R},{R}): max {mx:.2e} rms {rms:.2e} (direct {dmx:.2e} / {drms:.2e}, ratio {rms / drms:.2f}); edge columns of "
              + ", ".join(f"w {wd} ({100 * sh:.0f} %): max {e[0]:.2e} rms {e[1]:.2e} ratio {e[1] / de[1]:.2f}" for wd, sh, e, de in f["edge"]))
        if not (mx <= MAX_ERR and dmx <= MAX_ERR):
            bad.append((R, "max", mx, dmx))
        if not rms <= K_RMS * drms + RMS_FLOOR:
            bad.append((R, "rms", rms, drms))
        for wd, _, (_, erms), (_, derms) in f["edge"]:
            if not erms <= K_RMS * derms + RMS_FLOOR:
                bad.append((R, "edge rms", wd, erms, derms))
    assert not bad, bad


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
        with dt.options(lib, **opts):
            ws = {plan(lib, C, k, dd, 4, 1, 1)[1]["ot"] for dd in (d, 1)} if want == small else \
                 {plan(lib, C, k, dd, 4, 64, 100000)[1]["ot"] for dd in (d, 1)}
        lengths = [2 * max(ws) + 1] + sorted({w + e for w in ws for e in (-1, 0, 1)})
        B, ld, Lmax = len(lengths), (max(lengths) + 3) // 4 * 4, max(lengths)
        x, w1, b1, w2, b2 = ph.data(C, k, lengths, ld, seed=C + k + d)
        ref = ph.reference(x, w1, b1, w2, b2, lengths, k, d)
        acc0 = torch.rand(B, C, ld, device=DEV)
        beyond = dt.beyond_mask(lengths, ld).to(DEV).expand(B, C, ld)
        y0 = ph.run_pair(lib, 0, x, w1, b1, w2, b2, lengths, k, d)
        outs = {}
        for R in (3, 4):
            with dt.options(lib, **PAIR[R], **opts):
                insts = {plan(lib, C, k, dd, R, B, Lmax)[0] for dd in (d, 1)}
                assert {i[3:] for i in insts} == {want}, (insts, want, B, Lmax)
                ran |= insts
                outs[R] = {epi: ph.run_pair(lib, 4, x, w1, b1, w2, b2, lengths, k, d, epi=epi, acc=None if epi == 1 else acc0)
                           for epi in (1, 2, 3, 4)}
            for epi, o in outs[R].items():
                untouched = torch.full_like(o, -7.0) if epi == 1 else acc0
                assert torch.equal(torch.where(beyond, o, untouched), untouched), (R, want, epi, "wrote beyond an utterance")
                assert torch.isfinite(torch.where(beyond, torch.zeros_like(o), o)).all(), (R, want, epi, "read beyond an utterance")
            y = outs[R][1]
            e = torch.where(beyond, torch.zeros_like(ref), y.double() - ref)
            e0 = torch.where(beyond, torch.zeros_like(ref), y0.double() - ref)
            worst, rms, rms0 = float(e.abs().max()), float(e.pow(2).mean().sqrt()), float(e0.pow(2).mean().sqrt())
            print(f"\nW8 pair C {C} k {k} d {d} F({9 - R},{R}) tile {want}: max err {worst:.2e}, rms {rms:.2e} (direct launches {rms0:.2e}), "
                  f"lengths {lengths}")
            assert not torch.equal(y, y0), "the direct launches ran"
            assert worst <= 1e-5 and rms <= max(3.0 * rms0, 1e-6)
            for i, n in enumerate(lengths):
                for epi in (2, 3, 4):
                    want_o = y[i, :, :n] if epi == 2 else acc0[i, :, :n] + y[i, :, :n]
                    if epi == 4:
                        want_o = (want_o.cpu() / 3.0).to(DEV)  # a true division, like the reference's xs / num_kernels
                    assert torch.equal(outs[R][epi][i, :, :n], want_o), (R, want, epi, i, n)
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
        with dt.options(lib, **o):
            tiles.add(plan(lib, 64, 7, 1, R, 70, 300)[0][3:])
    assert tiles == TILES[64], tiles
    with dt.options(lib, **CONV[R]):  # (the rows alone run under these: one row of C = 64 takes the 64 x 32 tile)
        dt.walk_case(lib, (64, 64, 7, 1, SLOPE), 70, opts_list, alone=[0, 63, 65, 68, 1])


# ---- C = 512 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,d", [(7, 1), (11, 5)])
def test_c512_on_small_grids(lib, k, d):
    """a 512-channel layer at B = 1 and B = 2 (the ladder stops at the 64-row tile, whose 8 row tiles divide the 8 XCDs; the
    32-row tile it used to take was refused by the launch): both forms against float64 at the bars above, the same bits at
    both batch sizes and on the 128-row tile ("small_grid" = 0)"""
    C, lengths = 512, [389, 300]
    x, w, b, ld = make_case(C, k, lengths, seed=512 + k)
    beyond = dt.beyond_mask(lengths, ld).to(DEV)
    valid = ~beyond.expand(2, C, ld)
    r64 = reference64(x, w, b, lengths, k, d)
    err = lambda y: torch.where(valid, y.double() - r64, torch.zeros_like(r64))
    with dt.options(lib, **DIRECT):
        ed = err(dt.run_conv(lib, x, w, b, lengths, k, d, SLOPE))
    drms = float((ed.pow(2).sum() / valid.sum()).sqrt())
    for R in (3, 4):
        ys, tiles = [], []
        for rows, opts in ((2, {}), (1, {}), (2, dict(small_grid=0))):
            with dt.options(lib, **CONV[R], **opts):
                tiles.append(plan(lib, C, k, d, R, rows, 389)[0][3:])
                y = dt.run_conv(lib, x[:rows], w, b, lengths[:rows], k, d, SLOPE)
            dt.check_edges(y, beyond[:rows], (R, rows, opts))
            ys.append(y)
        assert tiles == [(2, 1, 4), (2, 1, 4), (4, 2, 2)], tiles
        assert torch.equal(ys[1], ys[0][:1]) and torch.equal(ys[2], ys[0]), (R, "the tiles differ")
        e = err(ys[0])
        mx, rms = float(e.abs().max()), float((e.pow(2).sum() / valid.sum()).sqrt())
        print(f"\nW8 C 512 k {k} d {d} F({9 - R},{R}): max {mx:.2e} rms {rms:.2e} (direct {drms:.2e}, ratio {rms / drms:.2f})")
        assert mx <= MAX_ERR and float(ed.abs().max()) <= MAX_ERR and rms <= K_RMS * drms + RMS_FLOOR
