"""Host-only checks of nn.conv1d's split-bf16 mode (no GPU): the two C entries' refusals and answers, the plan's independence of the
precision, the handle cache, the modules' precision_report(), and sr/train.py's --precision."""
import ctypes
import importlib.util
import os

import pytest

import gen_train_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nn():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import nn
    return nn


def test_create_prec_refuses_a_bad_prec_by_name(nn):
    from dissc_amd import _lib
    for prec in (-1, 2, 7):
        h = ctypes.c_void_p(1)
        rc = _lib.lib.dissc_convgrad_create_prec(32, 32, 3, 1, prec, ctypes.byref(h))
        assert rc != 0 and not h.value
        msg = _lib.lib.dissc_last_error().decode()
        assert "dissc_convgrad_create_prec" in msg and f"prec {prec}" in msg, msg
    # every shape create_wide takes, and no other
    for shape, ok in (((16, 16, 3, 1), True), ((32, 1, 7, 1), True), ((32, 32, 7, 12), True), ((32, 32, 7, 13), False), ((32, 32, 4, 1), False),
                      ((0, 32, 3, 1), False)):
        for prec in (0, 1):
            h = ctypes.c_void_p()
            rc = _lib.lib.dissc_convgrad_create_prec(*shape, prec, ctypes.byref(h))
            assert (rc == 0) == ok, (shape, prec, _lib.lib.dissc_last_error())
            if ok:
                _lib.lib.dissc_convgrad_destroy.argtypes = [ctypes.c_void_p]
                _lib.lib.dissc_convgrad_destroy(h)
    split = (ctypes.c_int32 * 3)()
    assert _lib.lib.dissc_convgrad_precision_info(None, split) != 0 and "dissc_convgrad_precision_info" in _lib.lib.dissc_last_error().decode()


def test_python_layers_refuse_an_unknown_precision_before_any_launch(nn):
    from dissc_amd._lib import DisscError
    # (the name is checked first: the CPU placeholders never reach the tensor checks)
    for call in (lambda: nn.conv1d(None, None, precision="bf16"), lambda: nn.discriminator_p(None, {}, 2, precision="fp16"),
                 lambda: nn.discriminator_s(None, {}, precision=1), lambda: nn.CodeGenerator(G.SMALL_CONFIG, precision="split"),
                 lambda: nn.MultiPeriodDiscriminator(precision="bf16x3"), lambda: nn.MultiScaleDiscriminator(precision=None)):
        with pytest.raises(DisscError, match="unknown precision"):
            call()


@pytest.mark.parametrize("shape, want", [
    ((16, 16, 3, 1), (False, False, False)),
    ((32, 32, 3, 1), (True, True, True)),
    ((32, 1, 7, 1), (False, True, False)),      # forward fp32: one output row; its data gradient has 32 rows
    ((33, 64, 7, 1), (True, True, True)),
    ((32, 32, 7, 12), (False, False, False)),   # span 72
    ((32, 32, 7, 10), (True, True, True)),      # span 60
    ((1024, 1024, 5, 1), (True, True, True)),
    ((256, 32, 5, 1), (True, True, True)),
    ((1, 32, 5, 1), (True, False, False)),
])
def test_precision_info_per_shape(nn, shape, want):
    assert nn.conv1d_precision(*shape) == want


def test_partials_and_workspace_are_functions_of_the_shape_only(nn):
    for cin, cout, k, d in ((32, 32, 3, 1), (33, 64, 7, 1), (128, 128, 7, 3), (1024, 1024, 5, 1), (16, 16, 3, 1)):
        for B, L in ((1, 64), (6, 56), (22, 260), (32, 8960)):
            hs = [nn._handle(nn.CONV1D, cin, cout, k, d, prec=p) for p in (0, 1)]
            plans = []
            for h in hs:
                P, pairs = ctypes.c_int(0), ctypes.c_int(0)
                assert nn.CONV1D.partials(h, B, L, ctypes.byref(P), ctypes.byref(pairs)) == 0
                plans.append((P.value, pairs.value, int(nn.CONV1D.workspace_bytes(h, B, L))))
            assert plans[0] == plans[1] and plans[0][:2] == nn.wgrad_partials(B, L, cin, cout, k), (cin, cout, k, B, L, plans)


def test_a_split_handle_and_an_fp32_handle_of_one_shape_are_distinct(nn):
    a, b = nn._handle(nn.CONV1D, 32, 32, 3, 1), nn._handle(nn.CONV1D, 32, 32, 3, 1, prec=1)
    assert a.value != b.value
    assert nn._handle(nn.CONV1D, 32, 32, 3, 1).value == a.value and nn._handle(nn.CONV1D, 32, 32, 3, 1, prec=1).value == b.value
    from dissc_amd._lib import DisscError
    with pytest.raises(DisscError, match="fp32 only"):
        nn._handle(nn.CONV1D_STRIDED, 32, 32, 5, 3, prec=1)


def test_module_reports_equal_conv1d_precision_layer_by_layer(nn):
    fp32 = (False, False, False)
    gen = nn.CodeGenerator(G.SMALL_CONFIG, precision="split_bf16")
    rep = gen.precision_report()
    assert list(rep) == [name for name, _, _ in gen.layers]
    for name, (cout, cin, k), _ in gen.layers:
        if name.startswith("ups."):
            assert rep[name] == fp32
        else:
            assert rep[name] == nn.conv1d_precision(cin, cout, k, gen._dilation[name]), name
    c0 = int(G.SMALL_CONFIG["upsample_initial_channel"])
    assert (c0, int(G.SMALL_CONFIG["model_in_dim"])) == (64, 33)
    assert rep["conv_pre"][0] and rep["conv_pre"][2]
    for name, (cout, cin, k), _ in gen.layers:
        if name.startswith("resblocks."):
            assert rep[name] == ((True, True, True) if cin == 32 else fp32), (name, cin)
            assert cin in (16, 32)
    assert rep["conv_post"] == fp32
    assert set(nn.CodeGenerator(G.SMALL_CONFIG).precision_report().values()) == {fp32}

    mpd = nn.MultiPeriodDiscriminator(precision="split_bf16").precision_report()
    assert len(mpd) == 30
    for name, v in mpd.items():
        leaf = name.split(".", 2)[2]
        assert v == {"convs.4": nn.conv1d_precision(1024, 1024, 5), "conv_post": nn.conv1d_precision(1024, 1, 3)}.get(leaf, fp32), name
    assert mpd["discriminators.0.convs.4"] == (True, True, True) and mpd["discriminators.0.conv_post"] == (False, True, False)
    msd = nn.MultiScaleDiscriminator(precision="split_bf16").precision_report()
    assert len(msd) == 24
    for name, v in msd.items():
        leaf = name.split(".", 2)[2]
        assert v == {"convs.6": nn.conv1d_precision(1024, 1024, 5), "conv_post": nn.conv1d_precision(1024, 1, 3)}.get(leaf, fp32), name
    assert set(nn.MultiScaleDiscriminator().precision_report().values()) == {fp32}


def test_train_parser_takes_precision_and_defaults_to_fp32():
    spec = importlib.util.spec_from_file_location("dissc_sr_train_precision", os.path.join(ROOT, "sr", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    parser = mod.get_parser()
    assert parser.parse_args([]).precision == "fp32"
    assert parser.parse_args(["--precision", "split_bf16"]).precision == "split_bf16"
    assert parser.parse_args(["--precision", "fp32"]).precision == "fp32"
    with pytest.raises(SystemExit):
        parser.parse_args(["--precision", "bf16"])
