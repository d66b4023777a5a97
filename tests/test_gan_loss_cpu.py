"""dissc_amd.nn.gan_loss and nn.MultiPeriodDiscriminator without a GPU: the ragged loss definitions of gan_loss_ref equal the
reference's literal torch.mean forms at equal lengths (float64) and read nothing beyond a length; the module's checkpoint keys and
shapes; dissc_ganloss_workspace_bytes as a function of the shapes only; every dissc_ganloss_* entry and the Python layer refuse bad
arguments before any device is touched."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gan_loss_ref as GL
import mpd_cases as M


@pytest.fixture(scope="module")
def nn():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import nn
    return nn


def _paired(rs, R, C, ld):
    return torch.from_numpy(rs.randn(2 * R, C, ld))


def test_ragged_definitions_equal_the_literal_means_at_equal_lengths(nn):
    assert (nn.FM, nn.DISC, nn.GEN) == (GL.FM, GL.DISC, GL.GEN)  # the restatement speaks of the library's ops
    rs = np.random.RandomState(0)
    shapes = [(4, 3, 8), (6, 1, 12), (2, 5, 4)]  # (R, C, ld), every row full
    maps = [_paired(rs, *s) for s in shapes]
    for m in maps:
        m.view(-1)[::7] = 0.0  # exact zeros: the kink
        m[m.shape[0] // 2:, :, ::3] = m[:m.shape[0] // 2, :, ::3]  # exact ties
    lens = [[ld] * r for r, _, ld in shapes]
    Rs = [r for r, _, _ in shapes]
    real, gen = [m[:r] for m, r in zip(maps, Rs)], [m[r:] for m, r in zip(maps, Rs)]
    tol = 1e-14

    slopes = [GL.SLOPE, GL.SLOPE, 1.0]
    act = lambda ts: [[F.leaky_relu(t, s) for t, s in zip(ts, slopes)]]
    total, vals, _ = GL.loss_ref(GL.FM, maps, lens, Rs, slopes, torch.float64)
    assert abs(float(total - GL.literal_feature_loss(act(real), act(gen)))) <= tol
    assert not vals[1].any()

    total, vals, _ = GL.loss_ref(GL.DISC, maps, lens, Rs, [1.0] * 3, torch.float64)
    lit, r_l, g_l = GL.literal_discriminator_loss(real, gen)
    assert abs(float(total - lit)) <= tol
    assert float((vals[0] - torch.stack(r_l)).abs().max()) <= tol and float((vals[1] - torch.stack(g_l)).abs().max()) <= tol

    total, vals, _ = GL.loss_ref(GL.GEN, maps, lens, Rs, [1.0] * 3, torch.float64)
    lit, g_l = GL.literal_generator_loss(gen)
    assert abs(float(total - lit)) <= tol and float((vals[0] - torch.stack(g_l)).abs().max()) <= tol and not vals[1].any()


@pytest.mark.parametrize("name", ["FM", "DISC", "GEN"])
def test_ragged_reference_reads_nothing_beyond_a_length_and_an_empty_map_is_zero(nn, name):
    op = getattr(nn, name)
    assert op == getattr(GL, name)
    rs = np.random.RandomState(1)
    R, C, ld = 6, 3, 12
    lens = [0, 1, 11, 12, 5, 12]
    x = _paired(rs, R, C, ld)
    poisoned = x.clone()
    poisoned[GL.beyond_mask(x.shape, lens, R)] = float("nan")
    empty = torch.full((2 * R, C, ld), float("nan"), dtype=torch.float64)
    a = GL.loss_ref(op, [x, empty], [lens, [0] * R], [R, R], [GL.SLOPE, 1.0], torch.float64, g_vals=torch.ones(2, 2))
    b = GL.loss_ref(op, [poisoned, empty], [lens, [0] * R], [R, R], [GL.SLOPE, 1.0], torch.float64, g_vals=torch.ones(2, 2))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2][0], b[2][0])
    assert torch.isfinite(a[0]) and float(a[1][0, 0]) > 0 and not a[1][:, 1].any()
    assert not a[2][0][GL.beyond_mask(x.shape, lens, R)].any() and not a[2][1].any()
    # the mean is over C sum(lens) elements
    real, _ = GL.valid_halves(x, lens, R)
    assert real.numel() == C * sum(lens)


def test_state_dict_keys_and_shapes(nn):
    D = nn.MultiPeriodDiscriminator()
    want = M.expected_shapes()
    assert len(want) == 90 and sorted(D._keys()) == sorted(want) and len(D.layers) == 30
    assert sorted(M.TorchMPD().state_dict()) == sorted(want)
    assert {k: tuple(v.shape) for k, v in M.TorchMPD().state_dict().items()} == want
    assert {k: tuple(v.shape) for k, v in M.mpd_state_dict(0).items()} == want
    # three flat layouts over the 30 layers, every tensor 16-byte aligned
    assert D.wn.n == 30 and D.wn.total_rows == sum(s[0] for _, s, _ in D.layers) and all(o % 4 == 0 for o in D.wn.off + D.wn.bias_off)
    assert [s for _, s, _ in D.layers[:6]] == [(32, 1, 5), (128, 32, 5), (512, 128, 5), (1024, 512, 5), (1024, 1024, 5), (1, 1024, 3)]
    with pytest.raises(RuntimeError):
        D.parameters()  # nothing loaded
    with pytest.raises(nn.DisscError):
        nn.MultiPeriodDiscriminator(periods=range(2, 13))  # 66 maps: more than one loss launch takes
    with pytest.raises(nn.DisscError):
        nn.MultiPeriodDiscriminator().to("cpu")
    assert nn.MultiPeriodDiscriminator(periods=(2, 3)).wn.n == 12


def test_python_constants_are_the_headers(nn):
    """nn.py restates include/dissc_hip.h's #defines by hand: hold them to the header's text, and the one without a #define
    (the workgroup's span, which the header gives in words) to what the library itself answers"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "dissc_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define\s+(DISSC_GANLOSS_\w+)\s+(\d+)\s*$", src, flags=re.M)}
    assert defs == {"DISSC_GANLOSS_MAX_MAPS": nn.GANLOSS_MAX_MAPS, "DISSC_GANLOSS_FM": nn.FM, "DISSC_GANLOSS_DISC": nn.DISC,
                    "DISSC_GANLOSS_GEN": nn.GEN}, defs
    # the entries agree with the header: MAX_MAPS maps are taken, one more is refused
    n = defs["DISSC_GANLOSS_MAX_MAPS"]
    assert nn.ganloss_workspace_bytes([1] * n, [1] * n, [4] * n) == (n * 16 + 255) // 256 * 256
    with pytest.raises(nn.DisscError):
        nn.ganloss_workspace_bytes([1] * (n + 1), [1] * (n + 1), [4] * (n + 1))
    # one workgroup per GANLOSS_WG_UNITS float4s of a half: 16 workgroups fill 256 bytes of partials, the next unit starts a 17th
    w = nn.GANLOSS_WG_UNITS
    assert nn.ganloss_workspace_bytes([1], [1], [4 * w * 16]) == 256 and nn.ganloss_workspace_bytes([1], [1], [4 * (w * 16 + 1)]) == 512


def test_workspace_bytes_is_a_function_of_the_shapes_only(nn):
    cases = [([6], [1], [8]), ([6, 6, 6, 6, 6], [1, 3, 32, 1024, 2], [8, 12, 260, 4, 16]), ([64] * 64, [32] * 64, [1496] * 64)]
    for R, C, ld in cases:
        a = nn.ganloss_workspace_bytes(R, C, ld)
        assert a == GL.workspace_bytes(R, C, ld) and a == nn.ganloss_workspace_bytes(R, C, ld) and a % 256 == 0 and a > 0
    assert nn.GANLOSS_WG_UNITS == GL.WG_UNITS and nn.GANLOSS_MAX_MAPS == GL.MAX_MAPS
    assert (nn.FM, nn.DISC, nn.GEN) == (GL.FM, GL.DISC, GL.GEN)
    # one more float4 than a workgroup's span: one more workgroup
    assert nn.ganloss_workspace_bytes([1], [1], [4 * GL.WG_UNITS * 16]) == 256
    assert nn.ganloss_workspace_bytes([1], [1], [4 * GL.WG_UNITS * 16 + 4]) == 512
    for R, C, ld in (([6], [1], [10]), ([-1], [1], [8]), ([0], [1], [8]), ([6], [0], [8]), ([6], [1], [0]), ([1] * 65, [1] * 65, [4] * 65),
                     ([1 << 16], [1 << 16], [4])):
        with pytest.raises(nn.DisscError):
            nn.ganloss_workspace_bytes(R, C, ld)
    with pytest.raises(nn.DisscError):
        nn.ganloss_workspace_bytes([], [], [])


def _arrays(n, R=6, C=3, ld=12, op=0):
    i32 = lambda v: (ctypes.c_int * n)(*([v] * n))
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below returns before a launch
    ptrs = (ctypes.c_void_p * n)(*([p.value] * n))
    return dict(maps=ptrs, lens=ptrs, R=i32(R), C=i32(C), ld=i32(ld), ops=i32(op), slopes=(ctypes.c_float * n)(*([0.1] * n)), p=p)


def _fwd(lib, n, a, out=True, ws=True, nws=1 << 20, **over):
    a = dict(a, **over)
    return lib.dissc_ganloss_forward(n, a["maps"], a["lens"], a["R"], a["C"], a["ld"], a["ops"], a["slopes"], a["p"] if out else None,
                                     a["p"] if ws else None, nws, None)


def _bwd(lib, n, a, g_total=True, gmaps=True, **over):
    a = dict(a, **over)
    return lib.dissc_ganloss_backward(n, a["maps"], a["lens"], a["R"], a["C"], a["ld"], a["ops"], a["slopes"], a["p"] if g_total else None,
                                      None, a["maps"] if gmaps else None, None)


def test_host_entries_refuse_bad_arguments_without_a_gpu(nn):
    from dissc_amd import lib
    EINVAL = -1
    a = _arrays(2)
    for call, who in ((_fwd, b"dissc_ganloss_forward"), (_bwd, b"dissc_ganloss_backward")):
        for key in ("maps", "lens", "R", "C", "ld", "ops", "slopes"):  # a null array
            assert call(lib, 2, a, **{key: None}) == EINVAL, key
            assert lib.dissc_last_error().startswith(who), lib.dissc_last_error()
        null_in = (ctypes.c_void_p * 2)(4096, None)
        assert call(lib, 2, a, maps=null_in) == EINVAL and b"map 1" in lib.dissc_last_error()
        assert call(lib, 2, a, lens=null_in) == EINVAL and b"map 1" in lib.dissc_last_error()
        assert call(lib, 2, a, maps=(ctypes.c_void_p * 2)(4096, 4100)) == EINVAL and b"aligned" in lib.dissc_last_error()
        assert call(lib, 0, a) == EINVAL
        big = _arrays(GL.MAX_MAPS + 1)
        assert call(lib, GL.MAX_MAPS + 1, big) == EINVAL and b"65 maps" in lib.dissc_last_error()
        assert call(lib, 2, _arrays(2, ld=10)) == EINVAL and b"multiple of 4" in lib.dissc_last_error()
        assert call(lib, 2, _arrays(2, ld=0)) == EINVAL
        assert call(lib, 2, _arrays(2, R=-3)) == EINVAL and b"R -3" in lib.dissc_last_error()
        assert call(lib, 2, _arrays(2, R=0)) == EINVAL
        assert call(lib, 2, _arrays(2, C=0)) == EINVAL
        assert call(lib, 2, _arrays(2, op=3)) == EINVAL and b"op 3" in lib.dissc_last_error()
        assert call(lib, 2, _arrays(2, op=-1)) == EINVAL
        assert call(lib, 2, a, slopes=(ctypes.c_float * 2)(0.1, float("nan"))) == EINVAL
        assert lib.dissc_last_error().startswith(who)
    assert _fwd(lib, 2, a, out=False) == EINVAL and _fwd(lib, 2, a, ws=False) == EINVAL
    assert _fwd(lib, 2, a, nws=255) == EINVAL and b"256 bytes" in lib.dissc_last_error()  # two maps of one workgroup each
    assert _bwd(lib, 2, a, g_total=False) == EINVAL and _bwd(lib, 2, a, gmaps=False) == EINVAL
    assert lib.dissc_ganloss_workspace_bytes(2, None, a["C"], a["ld"]) == 0


def test_python_layer_refuses_before_any_launch(nn):
    """CPU tensors stand in: every check below fails before a device pointer is taken"""
    x = torch.zeros(12, 3, 8)
    ln = torch.zeros(6, dtype=torch.int32)
    with pytest.raises(nn.DisscError):
        nn.gan_loss(nn.FM, [x], [ln], [6])  # not on the device
    with pytest.raises(nn.DisscError):
        nn.gan_loss(nn.FM, [], [], [])
    with pytest.raises(nn.DisscError):
        nn.gan_loss(nn.FM, [x] * 65, [ln] * 65, [6] * 65)  # more maps than the table holds
    D = nn.MultiPeriodDiscriminator()
    sd = M.mpd_state_dict(0)
    for bad in ({k: v for k, v in sd.items() if k != "discriminators.3.conv_post.weight_g"}, dict(sd, extra=torch.zeros(1)),
                dict(sd, **{"discriminators.0.convs.1.weight_v": torch.zeros(128, 32, 5)}),
                dict(sd, **{"discriminators.4.convs.0.weight_g": torch.zeros(32, 1, 1)}),
                dict(sd, **{"discriminators.2.conv_post.bias": torch.zeros(2)})):
        with pytest.raises(RuntimeError):
            D.load_state_dict(bad)
    assert D.v_flat is None
