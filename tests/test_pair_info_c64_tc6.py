"""dissc_pair_info without a GPU for the six-point pairs of the 64-channel stage (respair64_tc6_kernel; option "pair_tc6_c64":
bit 1 = k = 7, bit 2 = k = 11): the form and the outputs a workgroup owns (Tc6Geo64::WOUT of csrc/respair_f23.h) under the options
that select them, no instance without them, and the pins of tests/pair_harness.py (held by tests/test_pair_info.py) untouched by the option."""
import contextlib
import ctypes

import pytest

import pair_harness as ph
from tile_harness import lib  # noqa: F401  (the module fixture)

C = 64
DILS = ph.DILS
TILES = {7: (184, 172, 172), 11: (176, 176, 168)}  # 4 waves, 64 conv_d columns per workgroup


@contextlib.contextmanager
def c64_options(lib, tc6_c64, **kv):
    """pair_harness.options restores only its own SHIPPED keys: "pair_tc6_c64" goes back to the library's value here"""
    was = ctypes.c_int(-1)
    assert lib.lib.dissc_get_option(b"pair_tc6_c64", ctypes.byref(was)) == 0
    try:
        with ph.options(lib, pair_tc6_c64=tc6_c64, **kv):
            yield
    finally:
        assert lib.lib.dissc_set_option(b"pair_tc6_c64", was.value) == 0


@pytest.mark.parametrize("k", [7, 11])
def test_form_and_tile_under_the_bit_of_k(lib, k):
    bit = 1 if k == 7 else 2
    for mask in (bit, 3):
        for kv in ({}, {"pair_tc6": 0}, {"pair_f23_c64": 0}, {"pair_tc6": 0, "pair_f23_c64": 0}, {"pair_f23": 1}):
            with c64_options(lib, mask, **kv):
                for d, tile in zip(DILS, TILES[k]):
                    assert ph.pair_info(lib, C, k, d) == (ph.TC6, tile), (k, d, mask, kv)
                assert ph.pair_info(lib, C, k, 2) is None and ph.pair_info(lib, C, k, 7) is None


@pytest.mark.parametrize("k", [7, 11])
def test_no_instance_without_the_bit_or_the_master_switch(lib, k):
    bit = 1 if k == 7 else 2
    for mask, kv in ((0, {}), (3 - bit, {}), (3, {"pair_f23": 0}), (bit, {"pair_f23": 0, "pair_tc6": 15})):
        with c64_options(lib, mask, **kv):
            for d in DILS:
                assert ph.pair_info(lib, C, k, d) is None, (k, d, mask, kv)
                assert b"dissc_pair_info: no instance" in lib.lib.dissc_last_error()


def test_the_option_changes_no_other_shape(lib):
    """every pin and refusal of pair_harness.PINS / NONE_* with both bits set; the k = 3 pairs of the stage keep F(2,3)"""
    for Cx, k, opts, form, tiles in ph.PINS:
        with c64_options(lib, 3, **opts):
            for d, tile in zip(DILS, tiles):
                assert ph.pair_info(lib, Cx, k, d) == (form, tile), (Cx, k, d, opts)
    for Cx, k, opts in ph.NONE_ANYWHERE + ([] if ph.experimental(lib) else ph.NONE_DEFAULT):
        with c64_options(lib, 3, **opts):
            for d in DILS:
                assert ph.pair_info(lib, Cx, k, d) is None, (Cx, k, d, opts)


def test_the_option_is_restored(lib):
    v = ctypes.c_int(-1)
    assert lib.lib.dissc_get_option(b"pair_tc6_c64", ctypes.byref(v)) == 0
    with c64_options(lib, 3 - v.value):
        pass
    w = ctypes.c_int(-1)
    assert lib.lib.dissc_get_option(b"pair_tc6_c64", ctypes.byref(w)) == 0 and w.value == v.value
