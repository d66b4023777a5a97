"""dissc_pair_info without a GPU: the form mode 3 of dissc_respair1d builds and the outputs one workgroup of that instance owns
(Geo::WOUT of csrc/respair_f23.h), for every shape with an instance, under the shipped options and under the settings that select
each alternative form.  The GPU tests take their tile-edge lengths from this entry; the numbers are pinned in tests/pair_harness.py (PINS)
and held here."""
import pair_harness as ph
from pair_harness import DILS, NONE_ANYWHERE, NONE_DEFAULT, PINS, PINS_EXPERIMENTAL
from tile_harness import lib  # noqa: F401  (the module fixture)


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
