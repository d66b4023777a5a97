"""ResBlock2 configs ("resblock": "2") without a GPU: the key list and layer order of both generator classes against the
reference's named_parameters() order (recorded in tests/golden/gen_resblock2.npz by make_resblock2_golden.py), what the classes
and dissc_gen_create_rb / dissc_convgrad_create_wide refuse by name, the ABI number, and flops() against a hand count."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gen_train_ref as GT
import resblock2_cases as RB

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_resblock2.npz")


@pytest.fixture(scope="module")
def dissc_amd():
    import __graft_entry__ as ge
    ge.build()
    import dissc_amd
    from dissc_amd import nn  # noqa: F401  (dissc_amd.nn below)
    return dissc_amd


def test_keys_and_layer_order_are_the_references(dissc_amd):
    h = RB.vctk_config()
    order = [str(k) for k in np.load(GOLDEN)["param_order"]]
    assert len(order) == 3 * (1 + 5 + 15 * 2 + 1) + 2 and "resblocks.14.convs.1.weight_v" in order and not any("convs1" in k for k in order)
    G = dissc_amd.nn.CodeGenerator(h)
    assert list(G.named_leaves()) == order and G._keys()[:len(order)] == order
    assert [name for name, _, _ in G.layers] == RB.conv_names(h)
    # the reference registers dict / spkr first; its convs follow in this order
    g = dissc_amd.CodeGenerator(h)
    assert g._conv_names() == RB.conv_names(h)
    sd = RB.state_dict(h, seed=0)
    assert sorted(sd) == sorted(order)
    g.load_state_dict(sd)
    folded = g.remove_weight_norm()._folded
    assert sorted(folded) == sorted(RB.fold(sd)) and all(torch.equal(folded[k], v) for k, v in RB.fold(sd).items())
    # missing and unexpected keys are reported for this layout; a ResBlock1 checkpoint does not load
    bad = dict(sd)
    del bad["resblocks.3.convs.1.bias"]
    bad["resblocks.3.convs2.0.bias"] = sd["resblocks.3.convs.1.bias"]
    for cls in (dissc_amd.CodeGenerator, dissc_amd.nn.CodeGenerator):
        with pytest.raises(RuntimeError, match=r"missing \['resblocks\.3\.convs\.1\.bias'\], unexpected \['resblocks\.3\.convs2\.0\.bias'\]"):
            cls(h).load_state_dict(bad)
    # a folded checkpoint is accepted as before
    g2 = dissc_amd.CodeGenerator(h)
    g2.load_state_dict({k: v for k, v in list(RB.fold(sd).items())})
    # ResBlock1 configs keep their layout
    import synthdata as synth
    assert "resblocks.0.convs1.0" in dissc_amd.CodeGenerator(synth.VCTK_CONFIG)._conv_names()


def test_bad_configs_are_refused_by_name(dissc_amd):
    h = RB.vctk_config()
    # (k - 1) x dilation is even for an odd k: 74 is the first span beyond 72 that a config can ask for
    cases = [(dict(resblock_dilation_sizes=[[1, 2], [2], [3, 12]]), "resblock_dilation_sizes"),
             (dict(resblock_kernel_sizes=[3, 4, 7]), "resblock_kernel_sizes"),
             (dict(resblock_dilation_sizes=[[1, 37], [2, 6], [3, 12]]), "resblock_dilation_sizes")]
    for change, key in cases:
        for cls in (dissc_amd.CodeGenerator, dissc_amd.nn.CodeGenerator):
            with pytest.raises(NotImplementedError, match=key):
                cls(dict(h, **change))
    # as in the reference, entries beyond the first two are not read
    assert dissc_amd.CodeGenerator(dict(h, resblock_dilation_sizes=[[1, 2, 99], [2, 6, 99], [3, 12, 99]]))._config().resblock_dilations[2][1] == 12
    # the limit itself
    dissc_amd.CodeGenerator(dict(h, resblock_dilation_sizes=[[1, 36], [2, 18], [3, 12]]))


def test_create_entries_refuse_on_the_host(dissc_amd):
    from dissc_amd import _lib
    lib = _lib.lib
    assert lib.dissc_abi_version() == 9
    h = RB.config(GT.SMALL_CONFIG)
    table, keep = _lib.make_tensor_table(RB.fold(RB.state_dict(h, seed=1)))

    def create(resblock, precision=0, **change):
        cfg = dissc_amd.CodeGenerator(h)._config()
        for name, (j, m, v) in change.items():
            if name == "k":
                cfg.resblock_kernel_sizes[j] = v
            else:
                cfg.resblock_dilations[j][m] = v
        hnd = ctypes.c_void_p()
        rc = lib.dissc_gen_create_rb(ctypes.byref(cfg), table, len(keep), precision, resblock, ctypes.byref(hnd))
        assert hnd.value is None
        return rc, lib.dissc_last_error().decode()

    for resblock in (0, 3):
        rc, msg = create(resblock)
        assert rc == -1 and "dissc_gen_create_rb: resblock" in msg
    rc, msg = create(2, k=(1, 0, 4))
    assert rc == -1 and "even resblock kernel size 4" in msg
    rc, msg = create(2, d=(0, 1, 0))  # one dilation: the second is missing
    assert rc == -1 and "resblock_dilation_sizes[0][1] = 0" in msg
    rc, msg = create(2, d=(0, 1, 37))  # span 74
    assert rc == -1 and "resblock_dilation_sizes[0][1] = 37" in msg and "72" in msg
    rc, msg = create(1)  # the ResBlock1 layout is not in this table
    assert rc != 0 and "convs1" in msg
    # the differentiable layer: spans up to 72 through the wide entry, 60 through the old one
    hnd = ctypes.c_void_p()
    for k, d, old, wide in ((7, 12, -1, 0), (11, 7, -1, 0), (11, 6, 0, 0), (3, 37, -1, -1), (7, 13, -1, -1)):
        for entry, want in ((lib.dissc_convgrad_create, old), (lib.dissc_convgrad_create_wide, wide)):
            rc = entry(16, 16, k, d, ctypes.byref(hnd))
            assert rc == want and (hnd.value is not None) == (want == 0), (k, d, want)
            if want == 0:
                lib.dissc_convgrad_destroy(hnd)
            else:
                assert b"tap span" in lib.dissc_last_error()
    assert b"dissc_convgrad_create_wide" in lib.dissc_last_error()
    from dissc_amd import nn
    assert nn.wgrad_partials(4, 300, 16, 16, 7)[0] >= 1  # (host-only plan query through the wide entry's handle cache)


def test_resblock2_info_and_the_option(dissc_amd):
    from dissc_amd import _lib
    lib = _lib.lib

    def info(C, k, d0, d1):
        form, tile = ctypes.c_int(-1), ctypes.c_int(-1)
        rc = lib.dissc_resblock2_info(C, k, d0, d1, ctypes.byref(form), ctypes.byref(tile))
        return rc, form.value, tile.value

    default = _lib.get_option("rb2_fused")
    bits = {(32, 3): 1, (32, 5): 2, (32, 7): 4, (16, 3): 8, (16, 5): 16, (16, 7): 32}
    try:
        for (C, k), bit in bits.items():
            d0, d1 = dict(RB.V3_BLOCKS)[k]
            _lib.set_option("rb2_fused", bit)
            assert _lib.get_option("rb2_fused") == bit
            for (C2, k2), _ in bits.items():  # exactly the shape of the bit takes the one-launch form
                e0, e1 = dict(RB.V3_BLOCKS)[k2]
                assert info(C2, k2, e0, e1) == ((0, 1, 256 - (k2 - 1) * e1) if (C2, k2) == (C, k) else (0, 0, 0)), (C, k, C2, k2)
        _lib.set_option("rb2_fused", 63)
        # shapes without an instance take two launches whatever the mask says: other dilations, other widths
        for shape in ((32, 3, 1, 3), (16, 7, 3, 11), (64, 3, 1, 2), (256, 7, 3, 12), (32, 5, 6, 2)):
            assert info(*shape) == (0, 0, 0), shape
        # what no handle takes is refused by name
        for shape in ((32, 4, 1, 2), (32, 3, 0, 2), (32, 7, 3, 13), (0, 3, 1, 2)):
            assert info(*shape)[0] == -1 and b"dissc_resblock2_info" in lib.dissc_last_error(), shape
        # under the 16-row conv family the 32-channel convs are packed for 16x16x4: no one-launch form there
        _lib.set_option("mfma32", 0)
        assert info(32, 3, 1, 2) == (0, 0, 0) and info(16, 3, 1, 2) == (0, 1, 252)
    finally:
        _lib.set_option("mfma32", 1)
        _lib.set_option("rb2_fused", default)
    # the default mask: profiles/resblock2.md
    assert default == RB2_FUSED_DEFAULT
    for (C, k), bit in bits.items():
        d0, d1 = dict(RB.V3_BLOCKS)[k]
        assert info(C, k, d0, d1)[1] == (1 if default & bit else 0)
    # the diagnostic entry refuses on the host what it cannot run
    p = ctypes.c_void_p(64)  # never dereferenced
    for bad in (dict(k=4), dict(d1=0), dict(d1=13, k=7), dict(mode=2), dict(epi=0), dict(epi=5), dict(B=0)):
        a = dict(B=1, C=32, k=3, d0=1, d1=2, epi=1, mode=1)
        a.update(bad)
        rc = lib.dissc_resblock2_1d(p, p, p, p, p, p, p, None, a["B"], a["C"], a["k"], a["d0"], a["d1"], 64, 64, ctypes.c_float(0.1),
                                    a["epi"], ctypes.c_float(3.0), a["mode"], None)
        assert rc == -1 and b"dissc_resblock2_1d" in lib.dissc_last_error(), bad
    rc = lib.dissc_resblock2_1d(p, p, p, p, p, p, p, None, 1, 32, 3, 1, 3, 64, 64, ctypes.c_float(0.1), 1, ctypes.c_float(3.0), 1, None)
    assert rc == -1 and b"no one-launch instance" in lib.dissc_last_error()


RB2_FUSED_DEFAULT = 59  # every shape but C = 32, k = 7: the "rb2_fused" the library ships: the rule's outcome in profiles/resblock2.md


def test_flops_against_a_hand_count():
    h = RB.vctk_config()
    # conv_pre; per stage ConvTranspose at its input rate, then (3 + 5 + 7) x 2 C^2 per output column; conv_post
    macs = 257 * 512 * 7
    macs += 512 * 256 * 11 * 1 + 30 * 256 * 256 * 5
    macs += 256 * 128 * 8 * 5 + 30 * 128 * 128 * 20
    macs += 128 * 64 * 8 * 20 + 30 * 64 * 64 * 80
    macs += 64 * 32 * 4 * 80 + 30 * 32 * 32 * 160
    macs += 32 * 16 * 4 * 160 + 30 * 16 * 16 * 320
    macs += 16 * 7 * 320
    assert RB.flops_per_frame(h) == 2 * macs == 85734400
