"""The generator's split-bf16 kernels (CodeGenerator(..., precision="split_bf16"): conv_bf3_kernel, csrc/conv_bf3.hip, and
resblock_bf3_kernel, csrc/resblock_bf3.hip) on their own, in every tile and instance, at lengths that end beside every tile
edge.  Entries: dissc_conv1d_prec / dissc_conv_transpose1d_prec (prec = 1), dissc_respair1d mode 5, dissc_resblock1d_bf3; which
tile or window runs is never assumed: dissc_bf3_info answers from the launches' own planning functions and the set that ran is
asserted.  x is NaN beyond every length, outputs start as a sentinel (accumulators as known values) and must be untouched there.

Yardsticks, all computed on the CPU (tests/split_bf16_model.py, rehearsed in tests/test_gen_split_bf16_model_cpu.py); errors are
the worst column's l2 over the channels, relative, over all valid columns and again over the columns within one tap reach (one
halo for a block) of a tile boundary or an utterance end:
  one launch (conv, ConvTranspose)  against float64 on the same split operands  <= KERNEL_RATIO = 4 x torch fp32's error;
  a pair or a block                 against float64 on the unsplit operands     <= MODEL_FACTOR = 2 x the model's + 4 x torch fp32's.
The distance of a pair or block to the model itself is printed, not asserted.  Run with -s for one "GSB" line per case;
profiles/gen_split_bf16_tiles.md is a copy of them."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pair_harness as ph
import split_bf16_model as sm
import tile_harness as th
from tile_harness import (DEV, PAIRED, SENTINEL, SLOPE, UPS, beyond_mask, check_edges, edge_columns, held, lib, make_x, options,  # noqa: F401
                          paired_store)

pytestmark = pytest.mark.gpu

# (Cin, Cout, k, dilation, input slope): one per row class of conv_bf3_kernel's table, and the awkward ones
CONVS = [(257, 512, 7, 1, 1.0),      # conv_pre: Cin no multiple of 16, two M tiles
         (256, 256, 11, 5, SLOPE),   # span 50, the widest in use
         (256, 256, 3, 1, SLOPE),
         (128, 128, 7, 3, SLOPE),
         (128, 128, 11, 5, SLOPE),
         (20, 40, 7, 3, SLOPE),      # rows pad to the tile, Cin pads to the chunk
         (32, 32, 3, 1, SLOPE),      # class 0 on its own tile
         (48, 64, 7, 2, SLOPE)]      # class 1 on its own tile
# (tile index, small grid) a layer of each row class runs on under small_grid = 0 and 1 at these batch sizes
TILES_OF_CLASS = {0: {(0, 0)}, 1: {(1, 0)}, 2: {(2, 0), (1, 1)}, 3: {(3, 0), (1, 1)}}
BLOCKS = [(C, k, (1, 3, 5)) for C in (16, 32, 64) for k in (3, 7, 11)] + [(64, 11, (5, 5, 5))]


@pytest.fixture(scope="module", autouse=True)
def abi(lib):
    assert lib.lib.dissc_abi_version() >= 8


def bf3_class(M):
    return 3 if M >= 256 else 2 if M >= 128 else 1 if M >= 64 else 0


def edge_lengths(widths, pad):
    """0, 1, 2, 3, pad, pad + 1, m W + e for every width in play (m = 1, 2; e = -1, 0, 1), two columns past the first edge of the
    narrowest (so that every residue modulo 4 ends beside an edge) and the row stride itself -> (lengths, ld)"""
    ls = th.edge_lengths(widths, pad, extra=(3, min(widths) + 2))
    ld = (max(ls) + 3) // 4 * 4
    ls = sorted(set(ls) | {ld})
    assert {n % 4 for n in ls if any(0 < abs(n - m * w) <= 2 for w in widths for m in (1, 2))} == {1, 2, 3}
    return ls, ld


class Worst:
    """worst column error of the kernel and of the yardsticks, over all valid columns and over the edge columns"""

    def __init__(self, names):
        self.v = {(k, w): 0.0 for k in names for w in ("all", "edge")}

    def add(self, edge, **errs):
        for k, e in errs.items():
            if e.numel():
                self.v[(k, "all")] = max(self.v[(k, "all")], float(e.max()))
            if edge.any():
                self.v[(k, "edge")] = max(self.v[(k, "edge")], float(e[..., edge].max()))


def assert_launch_bar(tag, w):
    """one launch against float64 on the split operands"""
    for where in ("all", "edge"):
        ek, et = w.v[("kernel", where)], w.v[("fp32", where)]
        ratio = ek / max(et, sm.FLOOR)
        print(f"GSB {tag} [{where} columns]: kernel {ek:.2e} vs float64 on the split operands, torch fp32 {et:.2e} vs float64, "
              f"ratio {ratio:.2f} (bar {sm.KERNEL_RATIO})")
        assert ek <= sm.launch_bar(et), (tag, where, ek, et, ratio)


def assert_block_bar(tag, w):
    """a pair or a block against float64 on the unsplit operands"""
    for where in ("all", "edge"):
        ek, em, et, dist = (w.v[(k, where)] for k in ("kernel", "model", "fp32", "to_model"))
        bar = sm.block_bar(em, et)
        print(f"GSB {tag} [{where} columns]: kernel {ek:.2e} vs float64, model {em:.2e}, torch fp32 {et:.2e}, {ek / bar:.2f} of the bar "
              f"{bar:.2e}; kernel to model {dist:.2e}")
        assert ek <= bar, (tag, where, ek, em, et)


def in_one_row(x, lengths, gap):
    """the utterances' valid columns one after the other in ONE row, `gap` zeros between them (>= the reach of the taps: the
    "same" padding of each) -> (row [1, C, T], first column of each): one reference call per case instead of one per utterance"""
    offs, t = [], 0
    for n in lengths:
        offs.append(t)
        t += n + gap
    row = torch.zeros(1, x.shape[1], t, dtype=x.dtype)
    for i, n in enumerate(lengths):
        row[0, :, offs[i]:offs[i] + n] = x[i, :, :n]
    return row, offs


run_conv = functools.partial(th.run_conv, prec=1)  # dissc_conv1d_prec, split-bf16


# ---- conv_bf3_kernel, every tile -----------------------------------------------------------------------------------------
def test_conv_shapes_cover_every_tile(lib):
    """host only: the shapes below reach the four class tiles and the small-grid one"""
    classes = {bf3_class(s[1]) for s in CONVS}
    assert classes == {0, 1, 2, 3}
    assert set().union(*(TILES_OF_CLASS[c] for c in classes)) == {(0, 0), (1, 0), (2, 0), (3, 0), (1, 1)}
    with options(lib, small_grid=0):
        assert [lib.bf3_conv_info(64, m, 3, 1, 16, 600)["tile"] for m in (32, 64, 128, 256)] == [0, 1, 2, 3]


@pytest.mark.parametrize("shape", CONVS, ids=lambda s: f"{s[0]}-{s[1]}-k{s[2]}-d{s[3]}")
def test_conv_bf3_every_tile(lib, shape):
    """under small_grid = 0 and 1 (for >= 128 rows: the class tile and the 64 x 128 one, bit-identical as launch_conv_bf3 claims);
    every utterance alone and as a uniform lengths = NULL call gives the bits it has in the ragged batch"""
    cin, cout, k, d, slope = shape
    pad = (k - 1) * d // 2
    cls = bf3_class(cout)
    widths = set()
    for sg in (0, 1):
        with options(lib, small_grid=sg):
            widths.add(lib.bf3_conv_info(cin, cout, k, d, 16, 600)["bn"])
    lengths, ld = edge_lengths(widths, pad)
    B, Lmax = len(lengths), max(lengths)
    rs = np.random.RandomState(1000 * cin + 10 * k + d)
    x = make_x(rs, B, cin, ld, lengths)
    w = torch.from_numpy((rs.standard_normal((cout, cin, k)) / np.sqrt(cin * k)).astype(np.float32))
    b = torch.from_numpy(rs.uniform(-1, 1, cout).astype(np.float32))
    xd, beyond = x.to(DEV), beyond_mask(lengths, ld).to(DEV)
    first, ran = None, set()
    for sg in (0, 1):
        with options(lib, small_grid=sg):
            info = lib.bf3_conv_info(cin, cout, k, d, B, Lmax)
            y = run_conv(lib, xd, w, b, lengths, k, d, slope)
        assert info["bn"] in widths and (info["bm"], info["bn"]) == {0: (32, 256), 1: (64, 128), 2: (128, 256), 3: (256, 128)}[info["tile"]]
        check_edges(y, beyond, (shape, sg, info))
        first = y if first is None else first
        assert torch.equal(y, first), f"tile {info} differs from the class tile"
        ran.add((info["tile"], info["small_grid"]))
    print(f"\nGSB conv {cin} -> {cout} k {k} d {d}: tiles (index, small grid) {sorted(ran)}, widths {sorted(widths)}, lengths {lengths}")
    assert ran == TILES_OF_CLASS[cls], ran
    for i, n in enumerate(lengths):
        if n:
            one = run_conv(lib, xd[i:i + 1].clone(), w, b, [n], k, d, slope)
            assert torch.equal(one[0, :, :n], first[i, :, :n]) and (one[0, :, n:] == SENTINEL).all(), (i, n, "alone")
            uni = run_conv(lib, xd[i:i + 1].clone(), w, b, None, k, d, slope, Lmax=n)
            assert torch.equal(uni[0, :, :n], first[i, :, :n]) and (uni[0, :, n:] == SENTINEL).all(), (i, n, "uniform")
    x0, offs = in_one_row(x, lengths, 2 * pad)
    ref = sm.conv1d_ref(x0, w, b, k, d, slope)
    r64 = F.conv1d(F.leaky_relu(x0.double(), slope), w.double(), b.double(), padding=pad, dilation=d)
    r32 = F.conv1d(F.leaky_relu(x0, slope), w, b, padding=pad, dilation=d)
    yh, worst = held(first, beyond), Worst(("kernel", "fp32"))
    for i, n in enumerate(lengths):
        if n:
            sl = slice(offs[i], offs[i] + n)
            worst.add(edge_columns(n, widths, pad), kernel=sm.col_errs(yh[i, :, :n], ref[0, :, sl]), fp32=sm.col_errs(r32[0, :, sl], r64[0, :, sl]))
    assert_launch_bar(f"conv {cin} -> {cout} k {k} d {d}", worst)


# ---- the residual / MRF epilogues through two launches of conv_bf3_kernel -------------------------------------------------
@pytest.mark.parametrize("C,k,d", [(128, 7, 3), (256, 3, 1)])
def test_pair_epilogues_on_the_large_and_the_small_grid_tile(lib, C, k, d):
    """dissc_respair1d mode 5: conv_d (plain store) then conv_1 with epilogue 1 .. 4, both packed for split-bf16; lengths of every
    residue modulo 4 end in the epilogue's scalar tail"""
    widths = set()
    for sg in (0, 1):
        with options(lib, small_grid=sg):
            widths |= {lib.bf3_conv_info(C, C, k, dd, 16, 600)["bn"] for dd in (d, 1)}
    pad = (k - 1) * d // 2
    lengths, ld = edge_lengths(widths, pad)
    B = len(lengths)
    x, w1, b1, w2, b2 = pair = ph.data(C, k, lengths, ld, seed=C + k)
    acc0 = torch.rand(B, C, ld, device=DEV)
    beyond = beyond_mask(lengths, ld).to(DEV).expand(B, C, ld)
    ran = set()

    def tile_in_force(opts):
        infos = [lib.bf3_conv_info(C, C, k, dd, B, max(lengths)) for dd in (d, 1)]
        assert infos[0] == infos[1] and infos[0]["small_grid"] == opts["small_grid"], (opts, infos)
        ran.add((infos[0]["tile"], opts["small_grid"]))
        return infos[0]

    # (the small-grid tile gives the bits of the class tile)
    first = th.pair_epilogues_every_setting(lib, 5, pair, lengths, k, d, acc0, beyond, [dict(small_grid=0), dict(small_grid=1)], tile_in_force)
    assert ran == TILES_OF_CLASS[bf3_class(C)], ran
    xc, a0 = x.cpu(), acc0.cpu()
    got = {epi: o.cpu() for epi, o in first.items()}
    worst = {epi: Worst(("kernel", "model", "fp32", "to_model")) for epi in (1, 2, 3, 4)}
    for i, n in enumerate(lengths):
        if not n:
            continue
        xi, ai = xc[i:i + 1, :, :n], a0[i:i + 1, :, :n]
        y64 = sm.resblock_plain(xi[0], [w1, w2], [b1, b2], k, (d,), 0, 1)[None]
        y32 = sm.resblock_plain(xi[0], [w1, w2], [b1, b2], k, (d,), 0, 1, dtype=torch.float32)[None]
        edge = edge_columns(n, widths, pad + (k - 1) // 2)
        for epi in (1, 2, 3, 4):
            r64 = y64 if epi < 3 else ai.double() + y64 if epi == 3 else (ai.double() + y64) / 3.0
            r32 = y32 if epi < 3 else ai + y32 if epi == 3 else (ai + y32) / 3.0
            model = sm.pair_ref(xi, w1, b1, w2, b2, k, d, SLOPE, epi=epi, acc=ai)
            yk = got[epi][i:i + 1, :, :n]
            worst[epi].add(edge, kernel=sm.col_errs(yk, r64)[0], model=sm.col_errs(model, r64)[0], fp32=sm.col_errs(r32, r64)[0],
                           to_model=sm.col_errs(yk, model)[0])
        # exactly the pair's output stored / accumulated (a true division, like the reference's xs / num_kernels)
        y = got[1][i, :, :n]
        assert torch.equal(got[2][i, :, :n], y) and torch.equal(got[3][i, :, :n], ai[0] + y) and torch.equal(got[4][i, :, :n], (ai[0] + y) / 3.0), (i, n)
    print(f"\nGSB pair C {C} k {k} d {d}: tiles (index, small grid) {sorted(ran)}, lengths {lengths}")
    for epi in (1, 2, 3, 4):
        assert_block_bar(f"pair C {C} k {k} d {d} epilogue {epi}", worst[epi])


# ---- ConvTranspose ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,k,s", UPS[:5])
def test_conv_transpose_every_tile(lib, cin, cout, k, s):
    """the generator's five upsamplers, one launch of conv_bf3_kernel per phase group, with the paired float2 stores and the scalar
    path of the shared epilogue; lengths in INPUT columns"""
    groups = lib.conv_info(cin, cout, k, 1, s, 16, 600)  # the phase groups: rows, taps and left padding of each conv
    assert [paired_store(g, s) for g in groups] == [PAIRED[(cin, cout, k, s)]] * len(groups), groups
    widths = set()
    for sg in (0, 1):
        with options(lib, small_grid=sg):
            widths |= {lib.bf3_conv_info(cin, g["rows"], g["ntap"], 1, 16, 600)["bn"] for g in groups}
    reach = max(max(g["pad_left"], g["ntap"] - 1 - g["pad_left"]) for g in groups)
    lengths, ld = edge_lengths(widths, reach)
    B, Lmax = len(lengths), max(lengths)
    ldo = (s * Lmax + 3) // 4 * 4
    rs = np.random.RandomState(cin + k)
    x = make_x(rs, B, cin, ld, lengths)
    w = torch.from_numpy((rs.standard_normal((cin, cout, k)) / np.sqrt(cin * k / s)).astype(np.float32))
    b = torch.from_numpy(rs.uniform(-1, 1, cout).astype(np.float32))
    xd, ln = x.to(DEV), torch.as_tensor(lengths, dtype=torch.int32, device=DEV)
    beyond = beyond_mask(lengths, ldo, s).to(DEV)

    def run(xs, lens, lmax):
        y = torch.full((xs.shape[0], cout, ldo), SENTINEL, device=DEV)
        lib.check(lib.lib.dissc_conv_transpose1d_prec(xs.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), None if lens is None else lens.data_ptr(),
                                                      xs.shape[0], cin, cout, k, s, ld, ldo, lmax, ctypes.c_float(SLOPE), 1, None),
                  "dissc_conv_transpose1d_prec")
        return y

    first, ran = None, set()
    for sg in (0, 1):
        with options(lib, small_grid=sg):
            infos = [lib.bf3_conv_info(cin, g["rows"], g["ntap"], 1, B, Lmax) for g in groups]
            y = run(xd, ln, Lmax)
        check_edges(y, beyond, (sg, infos))
        first = y if first is None else first
        assert torch.equal(y, first), (sg, infos)
        ran |= {(bf3_class(g["rows"]), i["tile"], i["small_grid"]) for g, i in zip(groups, infos)}
    assert ran == {(c, t, sml) for c in {bf3_class(g["rows"]) for g in groups} for t, sml in TILES_OF_CLASS[c]}, ran
    for i, n in enumerate(lengths):
        if n:
            one = run(xd[i:i + 1].clone(), ln[i:i + 1].clone(), n)
            assert torch.equal(one[0, :, :n * s], first[i, :, :n * s]) and (one[0, :, n * s:] == SENTINEL).all(), (i, n, "alone")
            uni = run(xd[i:i + 1].clone(), None, n)
            assert torch.equal(uni[0, :, :n * s], first[i, :, :n * s]) and (uni[0, :, n * s:] == SENTINEL).all(), (i, n, "uniform")
    x0, offs = in_one_row(x, lengths, 2 * reach)
    ref = sm.conv_transpose1d_ref(x0, w, b, s, SLOPE)
    r64 = F.conv_transpose1d(F.leaky_relu(x0.double(), SLOPE), w.double(), b.double(), stride=s, padding=(k - s) // 2)
    r32 = F.conv_transpose1d(F.leaky_relu(x0, SLOPE), w, b, stride=s, padding=(k - s) // 2)
    yh, worst = held(first, beyond), Worst(("kernel", "fp32"))
    for i, n in enumerate(lengths):
        if n:
            sl = slice(offs[i] * s, (offs[i] + n) * s)
            worst.add(edge_columns(n, widths, reach, s), kernel=sm.col_errs(yh[i, :, :n * s], ref[0, :, sl]), fp32=sm.col_errs(r32[0, :, sl], r64[0, :, sl]))
    print(f"\nGSB convT {cin} -> {cout} k {k} s {s}: groups (p0, np, taps, rows) {[(g['p0'], g['np'], g['ntap'], g['rows']) for g in groups]}, "
          f"paired stores {PAIRED[(cin, cout, k, s)]}, tiles (class, index, small grid) {sorted(ran)}, lengths {lengths}")
    assert_launch_bar(f"convT {cin} -> {cout} k {k} s {s}", worst)


# ---- resblock_bf3_kernel, all nine instances ----------------------------------------------------------------------------------
def run_block(lib, x, w6, b6, acc, lengths, k, dil, epi, m0, m1, slope=SLOPE, div=3.0):
    """dissc_resblock1d_bf3 on device x / acc [B, C, ld] (acc is updated in place)"""
    B, C, ld = x.shape
    ln = torch.as_tensor(lengths, dtype=torch.int32, device=DEV)
    wp = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in w6])
    bp = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in b6])
    lib.check(lib.lib.dissc_resblock1d_bf3(x.data_ptr(), wp, bp, acc.data_ptr(), ln.data_ptr(), B, C, k, (ctypes.c_int32 * 3)(*dil), ld,
                                           int(max(lengths)), ctypes.c_float(slope), epi, ctypes.c_float(div), m0, m1, None),
              "dissc_resblock1d_bf3")
    return acc


def block_forms(lib, x, w6, b6, acc0, lengths, k, dil, epi, beyond):
    """the block in its two forms -> (one launch, three pair launches chained through EPI_STORE into NaN-filled buffers as
    generator.hip chains them, the final epilogue on the last)"""
    one = run_block(lib, x, w6, b6, acc0.clone(), lengths, k, dil, epi, 0, 3)
    src = x
    for m in (0, 1):
        nxt = run_block(lib, src, w6, b6, torch.full_like(x, float("nan")), lengths, k, dil, 0, m, m + 1)
        assert torch.isnan(torch.where(beyond, nxt, torch.full_like(nxt, float("nan")))).all(), (m, "wrote beyond an utterance")
        assert torch.isfinite(torch.where(beyond, torch.zeros_like(nxt), nxt)).all(), (m, "read beyond an utterance")
        src = nxt
    return one, run_block(lib, src, w6, b6, acc0.clone(), lengths, k, dil, epi, 2, 3)


@pytest.mark.parametrize("C,k,dil", BLOCKS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_resblock_bf3_both_forms(lib, C, k, dil):
    """Every instance as ONE launch (m0 = 0, m1 = 3) and as THREE pair launches: other halos, other centre widths (C = 32, k = 11:
    392 against 488 / 472 / 448), so every length sits differently in the two tile grids.  A column's MFMA k-step sequence does
    not depend on where its tile starts, a recomputed halo column is the same sum as the centre column of the neighbour, and
    x_k passes between pair launches as the fp32 it is in registers: the two forms agree bit for bit on every valid column, in
    all four epilogues.  The scalar tail (len % 4 = 1, 2, 3, len < 4) is in the lengths."""
    whole = lib.bf3_block_info(C, k, dil, 0, 3)
    pairs = [lib.bf3_block_info(C, k, dil, m, m + 1) for m in range(3)]
    halo = whole["h4"]
    assert whole["cols"] == (256 if C == 64 else 512) and whole["bn"] == whole["cols"] - 2 * halo
    assert all(p["cols"] == whole["cols"] and p["bn"] > whole["bn"] and sum(q["h4"] for q in pairs) >= halo for p in pairs)
    widths = {whole["bn"]} | {p["bn"] for p in pairs}
    lengths, ld = edge_lengths(widths, whole["pad"])
    assert {n % 4 for n in lengths if n > 4} == {0, 1, 2, 3} and {1, 2, 3} <= set(lengths)
    B = len(lengths)
    rs = np.random.RandomState(100 * C + k + sum(dil))
    x = torch.from_numpy(rs.uniform(-1, 1, (B, C, ld)).astype(np.float32))
    for i, n in enumerate(lengths):
        x[i, :, n:] = float("nan")  # never read
    w6 = [torch.from_numpy((rs.standard_normal((C, C, k)) / np.sqrt(C * k)).astype(np.float32)) for _ in range(6)]
    b6 = [torch.from_numpy(rs.uniform(-0.1, 0.1, C).astype(np.float32)) for _ in range(6)]
    xd = x.to(DEV)
    acc0 = torch.rand(B, C, ld, device=DEV) + 1.0  # the random accumulator EPI_MRF_ADD / _DIV start from; untouched beyond a length
    beyond = beyond_mask(lengths, ld).to(DEV).expand(B, C, ld)
    out = {}
    for epi in (0, 2, 3, 4):
        one, three = block_forms(lib, xd, w6, b6, acc0, lengths, k, dil, epi, beyond)
        for name, o in (("one launch", one), ("three launches", three)):
            assert torch.equal(torch.where(beyond, o, acc0), acc0), (epi, name, "wrote beyond an utterance")
            assert torch.isfinite(torch.where(beyond, torch.zeros_like(o), o)).all(), (epi, name, "read beyond an utterance")
        diff = (one != three) & ~beyond
        assert not diff.any(), (epi, "the two forms differ at (utterance, channel, column)", diff.nonzero()[:8].tolist(),
                                [lengths[i] for i in diff.nonzero()[:8, 0].tolist()])
        out[epi] = one.cpu()
    a0 = acc0.cpu()
    # every utterance alone, in both forms
    for i, n in enumerate(lengths):
        if n:
            bi = beyond[i:i + 1]
            for o in block_forms(lib, xd[i:i + 1].clone(), w6, b6, acc0[i:i + 1], lengths[i:i + 1], k, dil, 2, bi):
                assert torch.equal(o[0, :, :n].cpu(), out[2][i, :, :n]) and torch.equal(o[0, :, n:], acc0[i, :, n:]), (i, n, "alone")
    worst = Worst(("kernel", "model", "fp32", "to_model"))
    for i, n in enumerate(lengths):
        if not n:
            continue
        xi, y = x[i, :, :n], out[2][i, :, :n]
        r64 = sm.resblock_plain(xi, w6, b6, k, dil)
        model = sm.resblock_ref(xi, w6, b6, k, dil)
        worst.add(edge_columns(n, widths, halo), kernel=sm.col_errs(y, r64), model=sm.col_errs(model, r64),
                  fp32=sm.col_errs(sm.resblock_plain(xi, w6, b6, k, dil, dtype=torch.float32), r64), to_model=sm.col_errs(y, model))
        # EPI_STORE and EPI_MRF_SET store x_k; _ADD / _DIV accumulate exactly it (a true division)
        ai = a0[i, :, :n]
        assert torch.equal(out[0][i, :, :n], y) and torch.equal(out[3][i, :, :n], ai + y) and torch.equal(out[4][i, :, :n], (ai + y) / 3.0), (i, n)
    print(f"\nGSB block C {C} k {k} dil {dil}: one launch cols {whole['cols']} h4 {halo} bn {whole['bn']}; pair launches h4 / bn "
          f"{[(p['h4'], p['bn']) for p in pairs]}; lengths {lengths}")
    assert_block_bar(f"block C {C} k {k} dil {dil}", worst)


def test_blocks_cover_every_instance_and_the_largest_halo(lib):
    """host only: the nine (C, k) instances, and dilations (5, 5, 5) at C = 64, k = 11 leave the narrowest centre there is"""
    assert {(C, k) for C, k, _ in BLOCKS} == {(C, k) for C in (16, 32, 64) for k in (3, 7, 11)}
    assert lib.bf3_block_info(64, 11, (5, 5, 5))["bn"] == 72
    assert [lib.bf3_block_info(32, 11, (1, 3, 5), m, m + 1)["bn"] for m in range(3)] == [488, 472, 448]
    assert lib.bf3_block_info(32, 11, (1, 3, 5))["bn"] == 392


# ---- what the entries refuse ------------------------------------------------------------------------------------------------------
def test_entries_refuse_what_the_kernels_do_not_take(lib):
    """non-zero with a message and nothing written: no launch happens"""
    L = lib.lib

    def refused(rc, *outs):
        msg = L.dissc_last_error()
        assert rc != 0 and msg, (rc, msg)
        torch.cuda.synchronize()
        for o in outs:
            assert (o == SENTINEL).all()
        return msg.decode()

    C, k, ld = 32, 3, 16
    buf = torch.zeros(2 * C * ld + 8, device=DEV)
    acc = torch.full((C * ld + 8,), SENTINEL, device=DEV)
    w6 = [torch.zeros(64, 64, 11) for _ in range(6)]
    b6 = [torch.zeros(64) for _ in range(6)]
    wp = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in w6])
    bp = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in b6])
    f = ctypes.c_float

    def block(x=buf.data_ptr(), a=acc.data_ptr(), B=1, C=C, k=k, dil=(1, 3, 5), ld=ld, Lmax=ld, epi=2, m0=0, m1=3):
        return L.dissc_resblock1d_bf3(x, wp, bp, a, None, B, C, k, (ctypes.c_int32 * 3)(*dil), ld, Lmax, f(SLOPE), epi, f(3.0), m0, m1, None)

    assert block() == 0 and (acc[:C * ld] != SENTINEL).all() and (acc[C * ld:] == SENTINEL).all()  # (the arguments the refusals vary)
    acc.fill_(SENTINEL)
    assert "multiple of 4" in refused(block(ld=18, Lmax=16), acc)
    assert "multiple of 4" in refused(block(ld=2, Lmax=2), acc)
    assert "aligned" in refused(block(x=buf.data_ptr() + 4), acc)
    assert "aligned" in refused(block(a=acc.data_ptr() + 8), acc)
    assert "C = 48" in refused(block(C=48), acc)
    assert "k = 5" in refused(block(k=5), acc)
    refused(block(dil=(1, 3, 6)), acc)
    for m0, m1 in ((2, 2), (2, 1), (0, 4), (-1, 2)):
        assert "pairs" in refused(block(m0=m0, m1=m1), acc)
    refused(block(B=0), acc)
    refused(block(Lmax=0), acc)
    refused(block(epi=1), acc)
    refused(block(a=buf.data_ptr()))  # acc aliasing x
    with pytest.raises(lib.DisscError):
        lib.bf3_block_info(48, 3, (1, 3, 5))
    with pytest.raises(lib.DisscError):
        lib.bf3_block_info(32, 3, (1, 3, 5), 2, 2)

    # the single convs: prec = 1 never runs fp32 instead
    x = torch.zeros(1, 64, 16, device=DEV)
    y = torch.full((1, 64, 16), SENTINEL, device=DEV)
    w = torch.zeros(64, 64, 11)

    def conv(cin=64, cout=64, k=3, d=1, ldx=16, xp=x.data_ptr(), prec=1):
        return L.dissc_conv1d_prec(xp, w.data_ptr(), None, y.data_ptr(), None, 1, cin, cout, k, d, ldx, 16, 16, f(SLOPE), prec, None)

    assert conv() == 0 and (y == 0).all()
    y.fill_(SENTINEL)
    assert "split-bf16" in refused(conv(cout=16), y)           # a 16-row layer
    assert "split-bf16" in refused(conv(k=11, d=7), y)         # taps span 70 > MAX_TAP_SPAN columns
    assert "aligned" in refused(conv(ldx=18), y)               # launch_conv's own check, before the dispatch to conv_bf3.hip
    assert "aligned" in refused(conv(xp=x.data_ptr() + 4), y)
    refused(conv(prec=2), y)
    # ConvTranspose 32 -> 8, k = 4, stride 2: one phase group of 16 GEMM rows
    assert "split-bf16" in refused(L.dissc_conv_transpose1d_prec(x.data_ptr(), w.data_ptr(), None, y.data_ptr(), None, 1, 32, 8, 4, 2, 16, 32, 16,
                                                                 f(SLOPE), 1, None), y)
    assert "split-bf16" in refused(L.dissc_respair1d(x.data_ptr(), w.data_ptr(), None, w.data_ptr(), None, y.data_ptr(), None, None, 1, 16, 3, 1, 16,
                                                     16, f(SLOPE), 1, f(3.0), 5, None), y)
    for bad in ((64, 16, 3, 1), (64, 64, 11, 7), (512, 512, 1, 1)):  # (Cin, Cout, k, d): the last is a big 1x1 layer
        with pytest.raises(lib.DisscError):
            lib.bf3_conv_info(*bad, 4, 100)
