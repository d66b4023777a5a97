"""The direct implicit-GEMM convs (conv_mfma32_kernel, conv_mfma_kernel) in EVERY tile shape their tables offer, at lengths that
end beside every shape's tile edge: all shapes of a class must give the same bits (the claim above conv32_pick_cfg), write nothing
beyond an utterance, and sit inside the float64 bars of tests/train_stage_cases.py; the ragged walk beyond 64 utterances, the
ConvTranspose epilogues (paired float2 stores and the scalar path), and the residual / MRF epilogues of two direct launches.
Which shape runs is never assumed: dissc_conv_info (tests/test_conv_plan_cpu.py) is asked after every option change, and the set
of ids that ran is asserted.  Measured ratios, ids and wall time: profiles/direct_conv_tiles.md."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_grad_ref as R
import pair_harness as ph
from plan_rules import cls16, cls32
from tile_harness import (DEV, PAIRED, SENTINEL, SLOPE, UPS, beyond_mask, check_edges, check_pair_epilogues, edge_lengths, held, lib,  # noqa: F401
                          make_x, options, pair_epilogues_every_setting, paired_store, run_conv, walk_case)

pytestmark = pytest.mark.gpu

# (Cin, Cout, k, dilation, input slope) by row class of the 32-row kernel
SHAPES = [(20, 40, 7, 3, SLOPE),      # class 32: Cin no multiple of 16, M pads to 64
          (64, 64, 11, 5, SLOPE),     # class 64: span 50 (MAX_TAP_SPAN = 60)
          (128, 128, 3, 1, SLOPE),    # class 128
          (129, 320, 5, 2, SLOPE),    # class 256: two M tiles, the second partly empty
          (257, 512, 7, 1, 1.0)]      # class 256: conv_pre
NARROW = [(16, 16, 11, 5, SLOPE), (16, 1, 7, 1, SLOPE)]  # below 32 rows: the 16-row kernel whatever "mfma32" says
# the ids each class accepts (conv32_cfg / conv_cfg clamp the rest; 10 / 11 are the last small-grid tier)
IDS32 = {256: {0, 1, 2, 3, 5, 6, 7, 10}, 128: {1, 2, 3, 5, 7, 10}, 64: {2, 3, 5, 10}, 32: {3, 4, 11}}
IDS16 = {256: set(range(10)), 128: set(range(1, 9)), 64: {2, 3, 4, 5, 6, 7}, 32: {3, 4, 5, 6}, 16: {4, 6}}

# The bars: conv_grad_ref.check(..., "act", ...), e <= 4 x max(torch's fp32 CPU error, 2^-24 rms(ref)) against float64, whole tensor
# and worst channel.  No shape of this file needs the exception tests/train_stage_cases.py allows for long fp32 chains: the worst
# measured ratios are 3.19 / 3.70 (257 -> 512, k = 7, n = 1 799); every figure is in profiles/direct_conv_tiles.md.
K_WHOLE, K_CH = R.K_WHOLE, R.K_CH


def cls_of(M, family=32):
    return cls32(M) if family == 32 else cls16(M)


def tile_settings(lib, key_fmt, classes, info, extra=None):
    """every way to a tile shape of the classes: each id 0..10 as an override (all classes at once) under small_grid 0 and 1,
    and the shipped table under small_grid 0, 1 and 64 (64 x 256 workgroups are never there: the last step-down tier).
    Yields (options, ids in force per launch), asked of dissc_conv_info under those options."""
    out = []
    for cfg in [None] + list(range(11)):
        for sg in (0, 1) + ((64,) if cfg is None else ()):
            opts = dict(extra or {}, small_grid=sg)
            if cfg is not None:
                opts.update({key_fmt.format(c): cfg for c in classes})
            with options(lib, **opts):
                out.append((opts, tuple((g["family"], g["cfg"], g["bn"]) for g in info())))
    return out


def tile_edge_lengths(widths, pad):
    """beside the first edge of every width, and one length past the second edge of the widest"""
    return edge_lengths(widths, pad, multiples=(1,), extra=[2 * max(widths) + 1])


@functools.lru_cache(maxsize=None)
def conv_case(lib, shape):
    """one batch per shape, shared by every tile shape of both kernel families: lengths at the edges of every width either
    family has for the class, NaN beyond each length, and the float64 / float32 CPU references (computed once, read-only)"""
    cin, cout, k, d, slope = shape
    pad = (k - 1) * d // 2
    widths = set()
    families = [(16, "conv_cfg_bm{}", {"mfma32": 0} if cout >= 32 else {})] + ([(32, "conv32_cfg_bm{}", {})] if cout >= 32 else [])
    for fam, key, extra in families:
        for _, forms in tile_settings(lib, key, [cls_of(cout, fam)], lambda: lib.conv_info(cin, cout, k, d, 1, 20, 1025), extra):
            widths |= {bn for _, _, bn in forms}
    lengths = tile_edge_lengths(widths, pad)
    B, ld = len(lengths), (max(lengths) + 3) // 4 * 4
    rs = np.random.RandomState(1000 * cin + 10 * k + d)
    x = make_x(rs, B, cin, ld, lengths)
    w = torch.from_numpy((rs.uniform(-1, 1, (cout, cin, k)) / np.sqrt(cin * k)).astype(np.float32))
    b = torch.from_numpy(rs.uniform(-1, 1, cout).astype(np.float32))
    refs = {}
    for dt in (torch.float64, torch.float32):
        r = torch.zeros(B, cout, ld, dtype=dt)
        for i, n in enumerate(lengths):
            if n:
                r[i, :, :n] = F.conv1d(F.leaky_relu(x[i:i + 1, :, :n].to(dt), slope), w.to(dt), b.to(dt), padding=pad, dilation=d)[0]
        refs[dt] = r
    return dict(x=x.to(DEV), w=w, b=b, lengths=lengths, ld=ld, r64=refs[torch.float64], r32=refs[torch.float32],
                beyond=beyond_mask(lengths, ld).to(DEV))


def all_tiles(lib, case, shape, family):
    """the shape through every tile id of its class x small_grid x ragged_enum: one output (all bit-identical, nothing written
    beyond a length), and the set of ids that were in force"""
    cin, cout, k, d, slope = shape
    extra = {} if family == 32 or cout < 32 else {"mfma32": 0}
    key = "conv32_cfg_bm{}" if family == 32 else "conv_cfg_bm{}"
    B, Lmax = len(case["lengths"]), max(case["lengths"])
    first, ran = None, set()
    for opts, forms in tile_settings(lib, key, [cls_of(cout, family)], lambda: lib.conv_info(cin, cout, k, d, 1, B, Lmax), extra):
        (fam, cfg, _), = forms
        assert fam == family, (opts, forms)
        for enum in (0, 1):
            with options(lib, ragged_enum=enum, **opts):
                y = run_conv(lib, case["x"], case["w"], case["b"], case["lengths"], k, d, slope)
            check_edges(y, case["beyond"], (opts, cfg, enum))
            if first is None:
                first, first_cfg = y, cfg
            assert torch.equal(y, first), f"tile id {cfg} ({opts}, ragged_enum {enum}) differs from id {first_cfg}"
        ran.add(cfg)
    return first, ran


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}-{s[1]}-k{s[2]}-d{s[3]}")
def test_32_row_kernel_every_tile_shape(lib, shape):
    cin, cout, k, d, _ = shape
    case = conv_case(lib, shape)
    y, ran = all_tiles(lib, case, shape, 32)
    print(f"\nDT 32-row {cin} -> {cout} k {k} d {d}: ids {sorted(ran)}, lengths {case['lengths']}")
    assert ran == IDS32[cls_of(cout)], ran
    bad = R.check(f"32-row {cin}->{cout} k{k} d{d}", "act", held(y, case["beyond"]), case["r64"], case["r32"], K_WHOLE, K_CH)
    assert not bad, bad


@pytest.mark.parametrize("shape", NARROW + SHAPES, ids=lambda s: f"{s[0]}-{s[1]}-k{s[2]}-d{s[3]}")
def test_16_row_kernel_every_tile_shape(lib, shape):
    """the narrow layers as shipped, and the >= 32-row shapes under "mfma32" = 0.  Every tile shape of conv_mfma_kernel walks
    (chunk, tap, 4-channel k-step) in the same order for an output element, so the family is bit-identical within itself.
    Across the families: both kernels feed an output's products to the matrix core in the same order (chunk, tap, channel
    ascending), four channels per 16x16x4 step here and two per 32x32x2 step there, and the fp32 MFMA adds the products of a step
    to the accumulator one after the other -- so the two independent kernels (their own weight packing, fragment layout and
    epilogue) agree BIT FOR BIT, measured on every shape of this file (profiles/direct_conv_tiles.md).  That is asserted, as the
    stronger statement; that the 16-row kernel is the one that ran is shown by dissc_conv_info (family 16 under "mfma32" = 0,
    from the very functions the launch dispatches on) and by the ids in force, which are those of its own table (4, 8 and 9
    exist in no class of the 32-row kernel)."""
    cin, cout, k, d, slope = shape
    case = conv_case(lib, shape)
    y, ran = all_tiles(lib, case, shape, 16)
    print(f"\nDT 16-row {cin} -> {cout} k {k} d {d}: ids {sorted(ran)}, lengths {case['lengths']}")
    assert ran == IDS16[cls_of(cout, 16)], ran
    bad = R.check(f"16-row {cin}->{cout} k{k} d{d}", "act", held(y, case["beyond"]), case["r64"], case["r32"], K_WHOLE, K_CH)
    assert not bad, bad
    if cout >= 32:
        y32 = run_conv(lib, case["x"], case["w"], case["b"], case["lengths"], k, d, slope)
        (g,) = lib.conv_info(cin, cout, k, d, 1, len(case["lengths"]), max(case["lengths"]))
        assert g["family"] == 32
        assert torch.equal(y32, y), "the 16-row and the 32-row kernel differ"


@pytest.mark.parametrize("B", [70, 130])
def test_ragged_walk_beyond_64_utterances(lib, B):
    """ragged_tile's prefix sum runs over 64 utterances at a time: a batch of two and three rounds, empty utterances at the
    round boundary (index 64) and elsewhere, enumerated and plain grids bit for bit, rows of the batch = the rows alone"""
    walk_case(lib, (32, 32, 3, 1, SLOPE), B, [{"ragged_enum": e, "small_grid": s} for e in (1, 0) for s in (1, 0)],
              alone=[0, 63, 65, B - 2, 1])


def test_ragged_walk_in_xcd_order(lib):
    """"xcd_order" bit 2 puts the general instances on the 1-D XCD-ordered grid where a launch has >= 2 M tiles (129 -> 320 on
    256-row tiles has two): same tiles, same bits, with and without the ragged enumeration"""
    shape = (129, 320, 5, 2, SLOPE)
    with options(lib, small_grid=0):
        (g,) = lib.conv_info(129, 320, 5, 2, 1, 70, 300)
    assert (g["family"], g["cfg"], g["bm"]) == (32, 0, 256)
    walk_case(lib, shape, 70, [{"small_grid": 0, "xcd_order": x, "ragged_enum": e} for x in (11, 15) for e in (1, 0)] +
              [{"small_grid": 1, "xcd_order": 15}, {"small_grid": 0, "xcd_order": 15, "xcd_mg": 1}], alone=[0, 63, 65, 68, 1])


# ---- ConvTranspose ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,k,s", UPS)
def test_conv_transpose_every_tile_shape(lib, cin, cout, k, s):
    groups = lib.conv_info(cin, cout, k, 1, s, 16, 600)
    assert [paired_store(g, s) for g in groups] == [PAIRED[(cin, cout, k, s)]] * len(groups), groups
    assert all(g["family"] == 32 for g in groups)
    classes = sorted({cls_of(g["rows"]) for g in groups})
    settings = tile_settings(lib, "conv32_cfg_bm{}", classes, lambda: lib.conv_info(cin, cout, k, 1, s, 16, 600))
    widths = {bn for _, forms in settings for _, _, bn in forms}
    lengths = tile_edge_lengths(widths, max(g["pad_left"] for g in groups))
    B, ld, Lmax = len(lengths), (max(lengths) + 3) // 4 * 4, max(lengths)
    ldo = (s * Lmax + 3) // 4 * 4
    rs = np.random.RandomState(cin + k)
    x = make_x(rs, B, cin, ld, lengths)
    w = torch.from_numpy((rs.uniform(-1, 1, (cin, cout, k)) / np.sqrt(cin * k / s)).astype(np.float32))
    b = torch.from_numpy(rs.uniform(-1, 1, cout).astype(np.float32))
    refs = {}
    for dt in (torch.float64, torch.float32):
        r = torch.zeros(B, cout, ldo, dtype=dt)
        for i, n in enumerate(lengths):
            if n:
                r[i, :, :n * s] = F.conv_transpose1d(F.leaky_relu(x[i:i + 1, :, :n].to(dt), SLOPE), w.to(dt), b.to(dt), stride=s,
                                                     padding=(k - s) // 2)[0]
        refs[dt] = r
    xd, ln = x.to(DEV), torch.as_tensor(lengths, dtype=torch.int32, device=DEV)
    beyond = beyond_mask(lengths, ldo, s).to(DEV)
    first, ran = None, set()
    for opts, _ in settings:
        with options(lib, **opts):
            forms = lib.conv_info(cin, cout, k, 1, s, B, Lmax)  # (at this batch)
            y = torch.full((B, cout, ldo), SENTINEL, device=DEV)
            lib.check(lib.lib.dissc_conv_transpose1d(xd.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), ln.data_ptr(), B, cin, cout,
                                                     k, s, ld, ldo, Lmax, ctypes.c_float(SLOPE), None), "dissc_conv_transpose1d")
        ids = tuple(g["cfg"] for g in forms)
        check_edges(y, beyond, (opts, ids))
        first = y if first is None else first
        assert torch.equal(y, first), (opts, ids)
        ran |= {(cls_of(g["rows"]), g["cfg"]) for g in forms}
    print(f"\nDT convT {cin} -> {cout} k {k} s {s}: groups {[(g['p0'], g['np'], g['ntap'], g['rows']) for g in groups]}, "
          f"ids {sorted(ran)}, lengths {lengths}")
    assert ran == {(c, i) for c in classes for i in IDS32[c]}, ran
    yh = held(first, beyond)
    kw, kc = K_WHOLE, K_CH
    bad = R.check(f"convT {cin}->{cout} k{k} s{s}", "act", yh, refs[torch.float64], refs[torch.float32], kw, kc)
    worst = [0.0, 0.0]
    for i, n in enumerate(lengths):  # each utterance on its own columns
        if n:
            sl = (slice(i, i + 1), slice(None), slice(0, n * s))
            m = R.compare("act", yh[sl], refs[torch.float64][sl], refs[torch.float32][sl])
            worst = [max(worst[0], m["ratio"]), max(worst[1], m["ch_ratio"])]
            bad += R.check(f"  utterance {i} len {n}", "act", yh[sl], refs[torch.float64][sl], refs[torch.float32][sl], kw, kc, verbose=False)
    print(f"DT convT {cin} -> {cout}: worst utterance alone, ratio {worst[0]:.3f} worst channel {worst[1]:.3f}")
    assert not bad, bad


# ---- residual / MRF epilogues of two direct launches --------------------------------------------------------------------
@pytest.mark.parametrize("C,k,d", [(64, 3, 1), (128, 7, 3)])
def test_residual_and_mrf_epilogues_every_tile_shape(lib, C, k, d):
    """dissc_respair1d mode 0: conv_d (plain store) then conv_1 with epilogue 1..4 on conv_mfma32_kernel; lengths = 1, 2, 3 mod 4
    end in epi_store1's scalar tail.  Reference and bar: tests/pair_harness.py (float64 per utterance, max error 1e-5)."""
    settings = tile_settings(lib, "conv32_cfg_bm{}", [C], lambda: lib.conv_info(C, C, k, d, 1, 16, 600))
    widths = {bn for _, forms in settings for _, _, bn in forms}
    lengths = [n for n in tile_edge_lengths(widths, (k - 1) * d // 2) if n > 0]
    assert {n % 4 for n in lengths} == {0, 1, 2, 3}
    ld, B = (max(lengths) + 3) // 4 * 4, len(lengths)
    pair = ph.data(C, k, lengths, ld, seed=C + k)
    acc0 = torch.rand(B, C, ld, device=DEV)
    beyond = beyond_mask(lengths, ld).to(DEV).expand(B, C, ld)
    ran = set()

    def ids_in_force(opts):
        ids = {lib.conv_info(C, C, k, dd, 1, B, max(lengths))[0]["cfg"] for dd in (d, 1)}
        assert len(ids) == 1, (opts, ids)  # (both launches: the id depends on M, B and Lmax alone)
        ran.update(ids)
        return ids

    first = pair_epilogues_every_setting(lib, 0, pair, lengths, k, d, acc0, beyond, [opts for opts, _ in settings], ids_in_force)
    assert ran == IDS32[C], ran
    check_pair_epilogues(first, pair, lengths, k, d, acc0, beyond, f"DT pair C {C} k {k} d {d}: ids {sorted(ran)}, ")
