"""conv_wino8_kernel's shared-transform form (option "wino8_sv", template flag SHV: the eight waves of a (4, 2, 2) workgroup
form one double-buffered V between them) against the private-tile form of the same tile: the same bits in every transform
shape, nothing written beyond a length, an utterance alone = its row of the batch; more channel rounds and row tiles (C = 256,
C = 512); the residual / MRF epilogues of a pair whose first conv has the largest window; what dissc_wino8_form reports; an output buffer that starts as
NaN.  "small_grid" = 0 puts the tiny grids of these cases on the (4, 2, 2) tile, and dissc_wino8_info / dissc_wino8_form are asked
before every launch which tile and which form run.  Helpers: tests/tile_harness.py, tests/pair_harness.py.
(tests/test_gpu_wino8_tiles.py holds every tile of a shape to the same bits under the shipped options: since "wino8_sv" = 1 is
shipped, it compares the shared form against the private small tiles.)"""
import ctypes

import pytest
import torch

import pair_harness as ph
import tile_harness as th
from tile_harness import SLOPE, lib  # noqa: F401  (lib: the module fixture)

pytestmark = pytest.mark.gpu
CONV = {3: dict(wino8=2, wino8_r4=0), 4: dict(wino8=2, wino8_r4=2)}  # dissc_conv1d as F(6,3) / F(5,4)
ALL_SHAPES = 0o777777777
PAIR = {3: dict(wino8=1, wino8_mask=ALL_SHAPES, wino8_r4=0),           # mode 4 of dissc_respair1d: both convs as F(6,3) / F(5,4)
        4: dict(wino8=1, wino8_mask=ALL_SHAPES, wino8_r4=1, wino8_r4_mask=ALL_SHAPES)}
BIG = (4, 2, 2)
# (R, k, d) without a shared instance: k = 7, d = 5 as F(6,3) spilled a register in that form and keeps private tiles (conv_wino8.hip)
NOT_SHARED = {(3, 7, 5)}
MAX_ERR = 2e-5  # per element against float64: the bar of tests/test_gpu_wino8_tiles.py


def tile_and_form(lib, C, k, d, R, B, Lmax):
    p = lib.wino8_info(C, k, d, R, B, Lmax)
    return (p["mi"], p["ni"], p["wps"]), lib.wino8_form(C, k, d, R, B, Lmax), p


def ragged(lib, C, k, d, R):
    """about six rows: 1, one unit, OT - 1, OT, OT + 1 and 2 OT + 3 of the (4, 2, 2) tile of the shape"""
    with th.options(lib, small_grid=0):
        p = lib.wino8_info(C, k, d, R, 6, 100000)
    assert (p["mi"], p["ni"], p["wps"]) == BIG, p
    ot, unit = p["ot"], p["unit"]
    return [2 * ot + 3, 1, unit, ot - 1, ot, ot + 1]


def shared_form(R, k, d, sv=1):
    """what dissc_wino8_form must say of the (4, 2, 2) tile of the shape under "wino8_sv" = sv"""
    return 0 if (R, k, d) in NOT_SHARED else sv


def both_forms(lib, C, k, d, R, x, w, b, lengths):
    """the batch under "wino8_sv" = 1 and = 0 on the (4, 2, 2) tile: [shared, private], edges checked"""
    B, Lmax = len(lengths), max(lengths)
    beyond = th.beyond_mask(lengths, x.shape[2]).to(th.DEV)
    ys = []
    for sv in (1, 0):
        with th.options(lib, small_grid=0, wino8_sv=sv, **CONV[R]):
            tile, form, _ = tile_and_form(lib, C, k, d, R, B, Lmax)
            assert tile == BIG and form == shared_form(R, k, d, sv), (C, k, d, R, tile, form, sv)
            y = th.run_conv(lib, x, w, b, lengths, k, d, SLOPE)
        th.check_edges(y, beyond, (C, k, d, R, "wino8_sv", sv))
        ys.append(y)
    return ys


@pytest.mark.parametrize("d", [1, 3, 5])
@pytest.mark.parametrize("k", [7, 11])
@pytest.mark.parametrize("R", [3, 4])
def test_shared_and_private_transform_give_the_same_bits(lib, R, k, d):
    C = 128
    lengths = ragged(lib, C, k, d, R)
    x, w, b, ld = th.make_case(C, k, lengths, seed=100 * R + 10 * k + d)
    shared, private = both_forms(lib, C, k, d, R, x, w, b, lengths)
    assert torch.equal(shared, private), (R, k, d, "the shared form differs from the private one")
    beyond = th.beyond_mask(lengths, ld).to(th.DEV).expand(len(lengths), C, ld)
    err = torch.where(beyond, torch.zeros_like(shared, dtype=torch.float64), shared.double() - th.reference64(x, w, b, lengths, k, d))
    print(f"\nW8 sv C {C} k {k} d {d} F({9 - R},{R}): lengths {lengths}, max err {float(err.abs().max()):.2e}")
    assert float(err.abs().max()) <= MAX_ERR
    with th.options(lib, small_grid=0, wino8_sv=1, **CONV[R]):
        for i, n in enumerate(lengths):
            tile, form, _ = tile_and_form(lib, C, k, d, R, 1, n)
            assert tile == BIG and form == shared_form(R, k, d), (tile, form, n)
            one = th.run_conv(lib, x[i:i + 1].clone(), w, b, [n], k, d, SLOPE)
            assert (one[0, :, n:] == th.SENTINEL).all(), ("alone: wrote beyond the utterance", n)
            assert torch.equal(one[0, :, :n], shared[i, :, :n]), ("alone", R, k, d, n)


@pytest.mark.parametrize("C,k,d,R,rows", [(256, 11, 3, 3, None), (512, 7, 1, 4, 1)], ids=["C256-two-row-tiles", "C512-B1"])
def test_more_rounds_and_row_tiles(lib, C, k, d, R, rows):
    """C = 256: two row tiles and 16 channel rounds, the ragged batch; C = 512: four row tiles, 32 rounds, B = 1, L = OT + 1"""
    lengths = ragged(lib, C, k, d, R)
    if rows == 1:
        lengths = [lengths[5]]
    x, w, b, ld = th.make_case(C, k, lengths, seed=C + k + d)
    shared, private = both_forms(lib, C, k, d, R, x, w, b, lengths)
    assert torch.equal(shared, private), (C, k, d, R, "the shared form differs from the private one")
    beyond = th.beyond_mask(lengths, ld).to(th.DEV).expand(len(lengths), C, ld)
    err = torch.where(beyond, torch.zeros_like(shared, dtype=torch.float64), shared.double() - th.reference64(x, w, b, lengths, k, d))
    assert float(err.abs().max()) <= MAX_ERR, float(err.abs().max())


@pytest.mark.parametrize("R", [3, 4])
def test_all_four_epilogues_of_a_pair_with_the_largest_window(lib, R):
    """dissc_respair1d mode 4 at k = 11, d = 5, both launches on the (4, 2, 2) tile.  conv_d -- k = 11, d = 5, the shape with the largest
    window -- only STORES; the residual and the three MRF epilogues (set, add, add and divide) run on conv_1, which is k = 11, d = 1
    and has a smaller window: no entry that returns its output puts a residual or MRF epilogue behind a d = 5 conv.  Every epilogue
    form reuses the LDS of the window and of both V tiles behind the loop's last barrier, the plain store behind the d = 5 window
    too (here, in the bit-identity cases and in test_output_that_starts_as_nan).  Shared = private bit for bit, the pair against
    float64, the MRF modes exactly."""
    C, k, d = 128, 11, 5
    with th.options(lib, small_grid=0):
        ws = {lib.wino8_info(C, k, dd, R, 6, 100000)["ot"] for dd in (d, 1)}
    lengths = [2 * max(ws) + 3] + sorted({w + e for w in ws for e in (-1, 0, 1)}) + [1]
    B, ld, Lmax = len(lengths), (max(lengths) + 3) // 4 * 4, max(lengths)
    pair = ph.data(C, k, lengths, ld, seed=R)
    acc0 = torch.rand(B, C, ld, device=th.DEV)
    beyond = th.beyond_mask(lengths, ld).to(th.DEV).expand(B, C, ld)
    forms = []

    def inspect(opts):
        got = [tile_and_form(lib, C, k, dd, R, B, Lmax)[:2] for dd in (d, 1)]
        assert got == [(BIG, opts["wino8_sv"])] * 2, (got, opts)
        forms.append(opts["wino8_sv"])

    first = th.pair_epilogues_every_setting(lib, 4, pair, lengths, k, d, acc0, beyond,
                                            [dict(PAIR[R], small_grid=0, wino8_sv=sv) for sv in (1, 0)], inspect=inspect)
    assert forms == [1, 0]
    th.check_pair_epilogues(first, pair, lengths, k, d, acc0, beyond, f"W8 sv pair C {C} k {k} d {d} F({9 - R},{R}): ")


def test_the_form_query(lib):
    """dissc_wino8_form: shared on the (4, 2, 2) tile of every k = 7 / 11 shape but NOT_SHARED under the shipped options, private under
    "wino8_sv" = 0 and on every other tile, and an error where dissc_wino8_info has one"""
    assert lib.get_option("wino8_sv") == 1
    seen = set()
    for R in (3, 4):
        for k in (7, 11):
            for d in (1, 3, 5):
                for C in (128, 256, 512):
                    for B, Lmax in ((32, 10000), (1, 40), (2, 300), (4, 500), (8, 700)):  # the full grid, then down the ladder
                        tile, form, _ = tile_and_form(lib, C, k, d, R, B, Lmax)
                        seen.add(tile)
                        assert form == (shared_form(R, k, d) if tile == BIG else 0), (C, k, d, R, B, Lmax, tile, form)
                        with th.options(lib, wino8_sv=0):
                            assert tile_and_form(lib, C, k, d, R, B, Lmax)[:2] == (tile, 0)
                    with th.options(lib, small_grid=0):
                        assert tile_and_form(lib, C, k, d, R, 1, 1)[:2] == (BIG, shared_form(R, k, d))
                for wide in (0, 1, 2):  # C = 64: the 64-row tiles
                    for sg, B in ((0, 32), (1, 1)):
                        with th.options(lib, small_grid=sg, wino8_c64_wide=wide):
                            tile, form, _ = tile_and_form(lib, 64, k, d, R, B, 4000)
                        seen.add(tile)
                        assert tile != BIG and form == 0, (k, d, R, wide, sg, tile, form)
    assert seen == {(1, 1, 4), (2, 1, 4), (2, 2, 4), (4, 2, 2), (2, 4, 2), (2, 2, 2)}, seen
    assert tile_and_form(lib, 64, 3, 1, 3, 32, 4000)[:2] == ((2, 2, 4), 0)  # the one k = 3 instance
    out = ctypes.c_int(-5)
    assert lib.lib.dissc_wino8_form(128, 5, 1, 3, 1, 100, ctypes.byref(out)) == -1 and out.value == -5
    assert lib.lib.dissc_wino8_form(128, 7, 1, 3, 1, 100, None) == 0  # (the output is optional)


def test_output_that_starts_as_nan(lib):
    """the kernel only stores (epilogue 0): a second call into an output buffer filled with NaN gives the bits of the call into
    one filled with the sentinel, and leaves the NaN beyond every length"""
    C, k, d, R = 128, 11, 5, 3
    lengths = ragged(lib, C, k, d, R)
    x, w, b, ld = th.make_case(C, k, lengths, seed=7)
    B = len(lengths)
    beyond = th.beyond_mask(lengths, ld).to(th.DEV).expand(B, C, ld)
    with th.options(lib, small_grid=0, **CONV[R]):
        assert tile_and_form(lib, C, k, d, R, B, max(lengths))[:2] == (BIG, 1)
        y = th.run_conv(lib, x, w, b, lengths, k, d, SLOPE)
        y2 = torch.full((B, C, ld), float("nan"), device=th.DEV)
        ln = torch.as_tensor(lengths, dtype=torch.int32, device=th.DEV)
        lib.check(lib.lib.dissc_conv1d(x.data_ptr(), w.contiguous().data_ptr(), b.contiguous().data_ptr(), y2.data_ptr(), ln.data_ptr(),
                                       B, C, C, k, d, ld, ld, max(lengths), ctypes.c_float(SLOPE), None), "dissc_conv1d")
        torch.cuda.synchronize()
    th.check_edges(y, beyond[:, :1], "sentinel")
    assert torch.isnan(torch.where(beyond, y2, torch.full_like(y2, float("nan")))).all(), "wrote beyond an utterance"
    assert torch.equal(torch.where(beyond, torch.zeros_like(y), y), torch.where(beyond, torch.zeros_like(y2), y2))
