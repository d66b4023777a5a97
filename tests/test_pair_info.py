"""dissc_pair_info without a GPU: the form mode 3 of dissc_respair1d builds and the outputs one workgroup of that instance owns
(Geo::WOUT of csrc/respair_f23.h), for every shape with an instance, under the shipped options and under the settings that select
each alternative form.  The GPU tests take their tile-edge lengths from this entry; the numbers are pinned here."""
import pytest

import pair_harness as ph

DILS = (1, 3, 5)
# (C, k, options, form, tile at d = 1 / 3 / 5)
PINS = [
    (16, 11, {}, ph.F23, (500, 492, 468)),
    (32, 11, {}, ph.TC6, (360, 360, 348)),
    (32, 11, {"pair_tc6": 0}, ph.F23, (500, 492, 468)),
    (32, 11, {"pair_tc6": 1}, ph.F23, (500, 492, 468)),  # (bit 0 is k = 7's)
    (32, 7, {}, ph.TC6, (376, 372, 352)),
    (32, 7, {"pair_tc6": 1}, ph.TC6, (376, 372, 352)),
    (64, 3, {}, ph.F23, (252, 248, 248)),
]
# DISSC_EXPERIMENTAL=1 builds: the k = 3 instances of the C = 32 / 16 F(2,3) kernels (bits 4 / 8 of "pair_f23"), and the F(4,3)
# pair kernel (no constant outside its kernel file names its tile: 0) wherever the options leave no register-only form
PINS_EXPERIMENTAL = [
    (32, 3, {"pair_f23": 15}, ph.F23, (508, 508, 508)),
    (16, 3, {"pair_f23": 15}, ph.F23, (508, 508, 508)),
    (32, 7, {"pair_f23": 0}, ph.F43, (0, 0, 0)),
    (32, 11, {"pair_f23": 0}, ph.F43, (0, 0, 0)),
    (64, 3, {"pair_f23": 0}, ph.F43, (0, 0, 0)),
    (64, 3, {"pair_f23_c64": 0}, ph.F43, (0, 0, 0)),
]
# no instance in a default build
NONE_DEFAULT = [(32, 7, {"pair_f23": 0}), (32, 11, {"pair_f23": 0}), (64, 3, {"pair_f23": 0}), (64, 3, {"pair_f23_c64": 0}),
                (32, 7, {"pair_f23": 2, "pair_tc6": 15}), (32, 3, {"pair_f23": 15}), (16, 3, {"pair_f23": 15})]
# no instance in either build
NONE_ANYWHERE = [(16, 11, {"pair_f23": 1}), (16, 7, {"pair_tc6": 15}), (32, 3, {}), (16, 3, {}), (128, 3, {}), (256, 11, {}), (32, 5, {})]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import _lib
    return _lib


def _info(lib, C, k, d, opts):
    with ph.options(lib, **opts):
        return ph.pair_info(lib, C, k, d)


def test_form_and_tile_of_every_instance(lib):
    for C, k, opts, form, tiles in PINS + (PINS_EXPERIMENTAL if ph.experimental(lib) else []):
        for d, tile in zip(DILS, tiles):
            assert _info(lib, C, k, d, opts) == (form, tile), (C, k, d, opts)


def test_refusals_are_those_of_mode_3(lib):
    """DISSC_EINVAL with a message where make_pairw has no instance: a switched-off stage, a shape without a kernel, a dilation
    outside 1 / 3 / 5"""
    for C, k, opts in NONE_ANYWHERE + ([] if ph.experimental(lib) else NONE_DEFAULT):
        for d in DILS:
            assert _info(lib, C, k, d, opts) is None, (C, k, d, opts)
            assert b"dissc_pair_info: no instance" in lib.lib.dissc_last_error()
    for C, k in ((32, 11), (16, 11), (64, 3)):
        assert _info(lib, C, k, 2, {}) is None and _info(lib, C, k, 7, {}) is None
    assert lib.lib.dissc_pair_info(32, 11, 1, None, None) == 0  # (either output is optional)
