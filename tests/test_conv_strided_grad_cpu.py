"""dissc_amd.nn.conv1d_strided and nn.discriminator_p without a GPU: what dissc_convsgrad_create accepts and refuses, the calls
that return before any device is touched, the partial plan of the weight gradient (a function of the shape only) and the
workspace, and the references of tests/test_gpu_conv_strided_grad.py: conv_grad_ref.layer_ref with strided_op agrees with finite
differences in float64, the bars it is used with catch seeded defects on the ragged lengths of the GPU file, and the Conv2d
restatement of DiscriminatorP equals the period-major Conv1d composition the library runs."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_grad_harness as H
import conv_strided_ref as R


@pytest.fixture(scope="module")
def nn():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import nn
    return nn


def _create(lib, cin, cout, k, s):
    h = ctypes.c_void_p()
    rc = lib.dissc_convsgrad_create(cin, cout, k, s, ctypes.byref(h))
    return rc, h


def test_shape_rules(nn):
    from dissc_amd import lib
    good = R.DISC_P + [(16, 16, 3, 2), (16, 16, 7, 2), (16, 16, 7, 4), (16, 16, 11, 8)] + R.TAP_TABLE
    #      even k         k = 13           stride 1       stride > k     stride 9        no channels
    bad = [(16, 16, 4, 2), (16, 16, 13, 2), (16, 16, 5, 1), (16, 16, 3, 4), (16, 16, 11, 9), (0, 16, 5, 3), (16, 0, 5, 3),
           (16, 16, 1, 1), (16, 16, 5, 0), (-1, 16, 5, 3), (65536, 16, 5, 3)]
    for cin, cout, k, s in bad:
        rc, h = _create(lib, cin, cout, k, s)
        assert rc == -1 and h.value is None, (cin, cout, k, s)  # DISSC_EINVAL
        assert lib.dissc_last_error().startswith(b"dissc_convsgrad_create"), lib.dissc_last_error()
    # the message names the rule
    _create(lib, 16, 16, 4, 2)
    assert b"odd" in lib.dissc_last_error()
    _create(lib, 16, 16, 3, 4)
    assert b"stride <= min(k" in lib.dissc_last_error()
    _create(lib, 0, 16, 5, 3)
    assert b"channels" in lib.dissc_last_error()
    assert lib.dissc_convsgrad_create(16, 16, 5, 3, None) == -1  # a null out
    assert lib.dissc_last_error().startswith(b"dissc_convsgrad_create")
    for cin, cout, k, s in good:
        rc, h = _create(lib, cin, cout, k, s)
        assert rc == 0 and h.value, (cin, cout, k, s)
        nn.CONV1D_STRIDED.destroy(h)


def test_null_and_zero_size_calls_touch_no_device(nn):
    from dissc_amd import lib
    K = nn.CONV1D_STRIDED
    P, pairs = ctypes.c_int(), ctypes.c_int()
    rc, h = _create(lib, 32, 128, 5, 3)
    assert rc == 0
    assert K.partials(None, 32, 64, ctypes.byref(P), ctypes.byref(pairs)) == -1
    assert K.partials(h, 0, 64, ctypes.byref(P), ctypes.byref(pairs)) == -1
    assert K.partials(h, 32, 0, ctypes.byref(P), ctypes.byref(pairs)) == -1
    assert K.partials(h, 32, 64, None, None) == 0
    assert K.workspace_bytes(None, 32, 64) == 0 and K.workspace_bytes(h, 0, 64) == 0 and K.workspace_bytes(h, 32, 0) == 0
    for B, L in ((1, 192), (0, 192), (1, 0)):
        for hh in (None, h):
            assert K.forward(hh, None, None, None, B, L, 64, L, 1.0, None) == -1
            assert lib.dissc_last_error().startswith(b"dissc_convsgrad_forward")
            assert K.backward(hh, None, None, None, B, L, 64, L, 1.0, None, None, None, None, 0, None) == -1
            assert lib.dissc_last_error().startswith(b"dissc_convsgrad_backward")
    # nothing was packed: forward and backward refuse before any launch, after the row strides
    assert K.forward(h, None, None, None, 1, 192, 64, 192, 1.0, None) == -1
    assert b"dissc_convsgrad_set_weights first" in lib.dissc_last_error()
    assert K.forward(h, None, None, None, 1, 192, 60, 192, 1.0, None) == -1  # a row of y holds ceil(192 / 3) = 64
    assert b"ceil(Lmax / 3) = 64" in lib.dissc_last_error()
    assert K.forward(h, None, None, None, 1, 190, 64, 192, 1.0, None) == -1
    assert b"row strides" in lib.dissc_last_error()
    assert K.set_weights(h, None, None, None) == -1 and K.set_weights(None, None, None, None) == -1
    lib.dissc_convsgrad_packed.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.dissc_convsgrad_packed.restype = ctypes.c_longlong
    assert lib.dissc_convsgrad_packed(h, 0, None, None) == 4 * 5 * 4 * 256 and lib.dissc_convsgrad_packed(h, 1, None, None) == 5 * 16 * 256
    assert lib.dissc_convsgrad_packed(None, 0, None, None) == -1 and lib.dissc_convsgrad_packed(h, 2, None, None) == -1
    K.destroy(h)
    for fn in (lib.dissc_period_fold_fwd, lib.dissc_period_fold_bwd):
        assert fn(None, None, 1, 16, 2, 16, 8, None, None) == -1
    with pytest.raises(nn.DisscError):
        nn.wgrad_partials_strided(32, 64, 16, 16, 5, 1)


def test_partials_depend_on_the_shape_only_and_the_workspace_is_cg_workspaces(nn):
    T = nn.WGRAD_CHUNK
    rup = lambda x, m: (x + m - 1) // m * m
    L = 4480  # the first layer's rows at period 2, 8 960 samples
    for cin, cout, k, s in R.DISC_P:
        B = 64
        P, pairs = nn.wgrad_partials_strided(B, L, cin, cout, k, s)
        nch = R.cdiv(R.cdiv(L, s), T)  # chunks of OUTPUT positions
        assert P >= 1 and (P - 1) * pairs < B * nch <= P * pairs, (cin, cout, k, s, L, P, pairs)  # every pair once, no empty partial
        assert (P, pairs) == nn.wgrad_partials_strided(B, L, cin, cout, k, s)
        # the plan is the stride-1 layer's for the same reduction: the shape only
        assert (P, pairs) == nn.wgrad_partials(B, R.cdiv(L, s), cin, cout, k)
        # conv_grad.h's cg_workspace: the partials (one per time slice of a narrow layer) rounded to 256, the bias gradient's
        # doubles rounded to 256, 256 for the alignment of the base
        WT = 4 // (4 if cin > 64 else (2 if cin > 32 else 1))
        ws = nn.workspace_bytes_strided(B, L, cin, cout, k, s)
        assert ws == rup(P * WT * cout * cin * k * 4, 256) + rup(B * cout * 8, 256) + 256, (cin, cout, ws)
        assert ws <= 64 << 20
        print(f"plan {cin:4d} -> {cout:4d} k {k} s {s} L {L:5d}: P {P:4d} x {pairs:3d} pairs, workspace {ws / 2**20:6.2f} MB")
        L = R.cdiv(L, s)
    assert nn.wgrad_partials_strided(2, 388, 16, 16, 7, 2) != nn.wgrad_partials_strided(3, 388, 16, 16, 7, 2)


# ---------------------------------------------------------------------------------------------------------
# the reference, and the bars
# ---------------------------------------------------------------------------------------------------------
def test_layer_ref_agrees_with_finite_differences():
    rs = np.random.RandomState(0)
    B, cin, cout, k, s, L, slope = 2, 3, 2, 5, 3, 8, 0.1
    lengths = [8, 4]
    x = torch.from_numpy(rs.randn(B, cin, L))
    x = torch.where(x.abs() < 0.05, torch.full_like(x, 0.3), x)  # no kink inside a finite-difference step
    w, b, gy = (torch.from_numpy(rs.randn(*sh)) for sh in ((cout, cin, k), (cout,), (B, cout, R.out_ld(L, s))))
    y, gx, gw, gb = R.layer_ref(x, w, b, gy, lengths, R.strided_op(s), slope, torch.float64)
    vi, vo = R.valid_masks(lengths, L, R.strided_op(s))
    assert not y[(vo == 0).expand_as(y)].any() and not gx[(vi == 0).expand_as(gx)].any()
    assert y[0, :, :3].abs().min() > 0 and y[1, :, :2].abs().min() > 0  # ceil(8 / 3) = 3 and ceil(4 / 3) = 2 outputs

    def loss(x_, w_, b_):
        return float((R.layer_ref(x_, w_, b_, gy, lengths, R.strided_op(s), slope, torch.float64)[0] * gy).sum())

    eps = 1e-6
    for t, g, arg in ((x, gx, 0), (w, gw, 1), (b, gb, 2)):
        num = torch.zeros_like(t)
        flat, nflat = t.reshape(-1), num.reshape(-1)
        for i in range(flat.numel()):
            args = [x.clone(), w.clone(), b.clone()]
            args[arg].reshape(-1)[i] = flat[i] + eps
            up = loss(*args)
            args[arg].reshape(-1)[i] = flat[i] - eps
            nflat[i] = (up - loss(*args)) / (2 * eps)
        assert float((num - g).abs().max()) <= 1e-8 * max(1.0, float(g.abs().max())), arg
    assert not gx[1, :, 4:].any()


def test_bars_catch_seeded_defects(nn):
    """an fp32 "kernel result" (torch on the CPU, in the kernels' phase form) with one seeded defect fails its bar by a wide
    margin on the ragged lengths tests/test_gpu_conv_strided_grad.py runs; the clean one passes"""
    spec, slope = H.Spec("strided", 12, 10, 5, 3), 0.1
    s = spec.p
    lengths, ld, _ = H.lengths_for(nn, spec)
    assert any(n % s for n in lengths)  # floor and ceil differ
    x, w, b, gy = H.case(spec, len(lengths), ld, seed=3)
    r64 = R.layer_ref(x, w, b, gy, lengths, spec.op, slope, torch.float64)
    r32 = R.layer_ref(x, w, b, gy, lengths, spec.op, slope, torch.float32)
    for name, kind, y, a, c in zip(("y", "gx", "gw", "gb"), ("act", "act", "weight", "vec"), r32, r64, r32):
        assert not R.check("clean " + name, kind, y.clone(), a, c)
    assert R.taps(5, 3) == [(1, -1), (2, -1), (0, 0), (1, 0), (2, 0)]
    vi, vo = R.valid_masks(lengths, ld, spec.op)
    xa = F.leaky_relu(x, slope) * vi

    def wide(tag, kind, y, i, margin=10.0):
        m = R.compare(kind, y, r64[i], r32[i])
        print(f"defect: {tag:50s} ratio {m['ratio']:.3g} worst channel {m['ch_ratio']:.3g}")
        assert max(m["ratio"] / R.K_WHOLE, m["ch_ratio"] / R.K_CH) > margin, (tag, m)

    y, gw = R.phase_layer(xa, w, b, gy, lengths, s)
    assert not R.check("phase restatement y", "act", y, r64[0], r32[0], verbose=False)
    assert not R.check("phase restatement gw", "weight", gw, r64[2], r32[2], verbose=False)
    for tag, kw in (("a dropped tap", {"drop_tap": 1}), ("a plane shifted by one", {"plane_shift": (2, 1)}),
                    ("floor(n / s) outputs in place of ceil", {"floor_len": True})):
        y, gw = R.phase_layer(xa, w, b, gy, lengths, s, **kw)
        wide(tag + " in y", "act", y, 0)
        wide(tag + " in gw", "weight", gw, 2)


@pytest.mark.parametrize("p", R.PERIODS)
def test_conv2d_restatement_equals_the_period_major_composition(p):
    w = R.disc_p_weights(seed=p, dtype=torch.float64)
    for T in (p * 9, p * 9 + 1, p * 10 - 1):
        wav = torch.from_numpy(np.random.RandomState(T).randn(2, 1, T))
        for lengths in (None, [T, T - p]):
            a, c = R.disc_p_conv2d(w, wav, p, lengths), R.disc_p_conv1d(w, wav, p, lengths)
            masks = R.map_masks(T, p, lengths, 2)
            for j, (ma, mc, mk) in enumerate(zip(a, c, masks)):
                assert ma.shape == mc.shape == (2 * p, R.DISC_P_CHANNELS[j + 1], mk.shape[2])
                assert float((ma - mc).abs().max()) <= 1e-12, (p, T, j)
                assert not ma[(mk == 0).expand_as(ma)].any() and ma[(mk == 1).expand_as(ma)].abs().min() > 0
