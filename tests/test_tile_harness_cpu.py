"""The teeth of tests/tile_harness.py itself, without a GPU: check_edges must raise on one overwritten sentinel and on one NaN inside
a length, the masks and edge lengths must be those of the functions the harness replaced (the expected values below were taken
from those functions before they moved: unit 4, tile widths {8, 16}, lengths 0, 1, 7, 8, 9, 17), and assert_float64_bars must
fail one ulp above each bar."""
import numpy as np
import pytest
import torch

import tile_harness as th

LENGTHS, LD, UNIT, WIDTHS = (0, 1, 7, 8, 9, 17), 20, 4, (8, 16)


def columns(mask):
    return [row.nonzero().flatten().tolist() for row in mask[:, 0]]


def clean_output():
    beyond = th.beyond_mask(LENGTHS, LD)
    y = torch.where(beyond.expand(len(LENGTHS), 3, LD), torch.tensor(th.SENTINEL), torch.rand(len(LENGTHS), 3, LD))
    return y, beyond


def test_check_edges_and_held():
    y, beyond = clean_output()
    th.check_edges(y, beyond, "clean")
    assert th.held(y, beyond)[2, 1, 7:].abs().sum() == 0 and torch.equal(th.held(y, beyond)[5, :, :17], y[5, :, :17])
    wrote = y.clone()
    wrote[4, 2, 9] = 0.5  # the first column beyond a length of 9
    with pytest.raises(AssertionError, match="wrote beyond"):
        th.check_edges(wrote, beyond, "one sentinel overwritten")
    with pytest.raises(AssertionError, match="wrote beyond"):
        th.held(wrote, beyond)
    read = y.clone()
    read[5, 0, 16] = float("nan")  # the last column inside a length of 17
    with pytest.raises(AssertionError, match="from beyond"):
        th.check_edges(read, beyond, "one NaN inside")


def test_masks_and_lengths_are_those_of_the_functions_they_replace():
    assert columns(th.beyond_mask(LENGTHS, LD)) == [list(range(n, LD)) for n in LENGTHS]
    assert columns(th.beyond_mask((0, 1, 3), 8, 2)) == [list(range(8)), list(range(2, 8)), [6, 7]]  # ConvTranspose: stride 2
    # a tile of two units is all edge; of four: the first and last unit of each tile, and the last unit of the utterance
    assert columns(th.edge_mask(LENGTHS, LD, UNIT, [8])) == [list(range(n)) for n in LENGTHS]
    assert columns(th.edge_mask(LENGTHS, LD, UNIT, [16])) == [[], [0], list(range(7)), list(range(8)), [0, 1, 2, 3, 5, 6, 7, 8],
                                                              [0, 1, 2, 3, 12, 13, 14, 15, 16]]
    assert th.edge_columns(17, WIDTHS, 2).nonzero().flatten().tolist() == [0, 1, 6, 7, 8, 9, 14, 15, 16]
    assert th.edge_columns(9, (8,), 1, 2).nonzero().flatten().tolist() == [0, 1, 14, 15, 16, 17]
    # the three variants at pad = 3: the direct convs', the split-bf16 kernels' (before the row stride is added), the sweep's
    assert th.edge_lengths(WIDTHS, 3, multiples=(1,), extra=[33]) == [0, 1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 33]
    assert th.edge_lengths(WIDTHS, 3, extra=(3, 10)) == [0, 1, 2, 3, 4, 7, 8, 9, 10, 15, 16, 17, 31, 32, 33]
    assert th.edge_lengths(WIDTHS, 3, extra={UNIT - 1, UNIT + 1}) == [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33]


def test_make_case_poisons_beyond_every_length():
    x, w, b, ld = th.make_case(8, 3, [9, 0, 5], seed=1, device="cpu")
    assert ld == 12 and x.shape == (3, 8, 12) and w.shape == (8, 8, 3) and b.shape == (8,)
    assert torch.equal(torch.isnan(x), th.beyond_mask([9, 0, 5], 12).expand(3, 8, 12))
    assert torch.isfinite(th.reference64(x, w, b, [9, 0, 5], 3, 1)).all()


def test_float64_bars_fail_one_ulp_above_each_bar():
    max_err, k_rms, k_edge, floor = 2e-5, 2.0, 3.0, 1e-8
    up = lambda v: float(np.nextafter(v, np.inf))
    drms, derms = 1e-6, 2e-6
    at = dict(all=(max_err, k_rms * drms + floor), direct=(max_err, drms), edge=[(8, 0.5, (max_err, k_edge * derms + floor), (0.0, derms))])
    th.assert_float64_bars({3: at, 4: at}, max_err, k_rms, k_edge, floor, edge_max=max_err)  # every figure exactly at its bar
    above = [dict(at, all=(up(max_err), at["all"][1])), dict(at, direct=(up(max_err), drms)), dict(at, all=(max_err, up(at["all"][1]))),
             dict(at, edge=[(8, 0.5, (up(max_err), at["edge"][0][2][1]), (0.0, derms))]),
             dict(at, edge=[(8, 0.5, (max_err, up(at["edge"][0][2][1])), (0.0, derms))])]
    for fig in above:
        assert len(th.float64_bars(fig, max_err, k_rms, k_edge, floor, edge_max=max_err)) == 1
        with pytest.raises(AssertionError):
            th.assert_float64_bars({3: at, 4: fig}, max_err, k_rms, k_edge, floor, edge_max=max_err, what="one ulp above")
    with pytest.raises(AssertionError, match=r"\(3, 'max'.*\(4, 'rms'"):  # every form is reported, not the first alone
        th.assert_float64_bars({3: above[0], 4: above[2]}, max_err, k_rms, k_edge, floor, edge_max=max_err)
    th.assert_float64_bars({4: above[3]}, max_err, k_rms, k_edge, floor)  # without edge_max the edge columns are held to rms alone


def test_options_restore_what_they_found_or_what_they_are_told():
    class Lib:
        def __init__(self):
            self.v = {"a": 1, "b": 2}
        get_option = lambda self, k: self.v[k]
        set_option = lambda self, k, v: self.v.__setitem__(k, v)

    lib = Lib()
    with pytest.raises(RuntimeError):
        with th.options(lib, a=5):
            assert lib.v == {"a": 5, "b": 2}
            raise RuntimeError
    assert lib.v == {"a": 1, "b": 2}
    with th.options(lib, restore={"b": 7}, a=5):
        assert lib.v == {"a": 5, "b": 2}
    assert lib.v == {"a": 5, "b": 7}
