"""dissc_amd.nn.conv_transpose1d without a GPU: what dissc_convtgrad_create refuses and accepts, the partial plan of the
weight gradient (a function of the shape only, inside 64 MB for the five upsamplers), and the reference of
tests/test_gpu_conv_transpose_grad.py: conv_grad_ref.layer_ref with conv_transpose_op agrees with finite differences in float64, and
the bars it is used with catch seeded defects."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_transpose_grad_ref as R


@pytest.fixture(scope="module")
def nn():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import nn
    return nn


def _create(lib, cin, cout, k, s):
    h = ctypes.c_void_p()
    rc = lib.dissc_convtgrad_create(cin, cout, k, s, ctypes.byref(h))
    return rc, h


def test_invalid_shapes_are_refused_and_the_upsamplers_accepted(nn):
    from dissc_amd import lib
    assert R.ups_from_config() == R.UPS
    #      k < s          k - s odd       k = 12           s = 9           s = 0          no channels
    bad = [(16, 16, 3, 4), (16, 16, 5, 2), (16, 16, 12, 2), (16, 16, 9, 9), (16, 16, 11, 9), (16, 16, 4, 0), (0, 16, 4, 2),
           (16, 0, 4, 2), (16, 16, 4, -2), (-1, 16, 4, 2)]
    for cin, cout, k, s in bad:
        rc, h = _create(lib, cin, cout, k, s)
        assert rc == -1 and h.value is None, (cin, cout, k, s)  # DISSC_EINVAL
        assert b"dissc_convtgrad_create" in lib.dissc_last_error()
    # the message names the rule
    _create(lib, 16, 16, 5, 2)
    assert b"k - stride even" in lib.dissc_last_error()
    _create(lib, 16, 16, 9, 9)
    assert b"stride 9" in lib.dissc_last_error()
    assert lib.dissc_convtgrad_create(16, 16, 4, 2, None) == -1
    P, pairs = ctypes.c_int(), ctypes.c_int()
    # the five upsamplers and the limits themselves
    for cin, cout, k, s in R.UPS + R.OFF_GRID + R.OTHER_STRIDES + [(16, 16, 11, 1), (16, 16, 8, 8), (1, 1, 1, 1), (16, 16, 11, 7)]:
        rc, h = _create(lib, cin, cout, k, s)
        assert rc == 0 and h.value, (cin, cout, k, s)
        assert lib.dissc_convtgrad_partials(h, 32, 28, ctypes.byref(P), ctypes.byref(pairs)) == 0 and P.value >= 1
        assert lib.dissc_convtgrad_partials(h, 0, 28, ctypes.byref(P), ctypes.byref(pairs)) == -1
        assert lib.dissc_convtgrad_partials(h, 32, 0, ctypes.byref(P), ctypes.byref(pairs)) == -1
        # nothing was packed: forward and backward refuse before any launch
        assert lib.dissc_convtgrad_forward(h, None, None, None, 1, 64, 64 * s, 64, 1.0, None) == -1
        assert b"set_weights first" in lib.dissc_last_error()
        assert lib.dissc_convtgrad_backward(h, None, None, None, 1, 64, 64 * s, 64, 1.0, None, None, None, None, 0, None) == -1
        assert b"set_weights first" in lib.dissc_last_error()
        lib.dissc_convtgrad_destroy(h)
    assert lib.dissc_convtgrad_partials(None, 32, 64, ctypes.byref(P), ctypes.byref(pairs)) == -1
    assert lib.dissc_convtgrad_workspace_bytes(None, 32, 64) == 0
    with pytest.raises(nn.DisscError):
        nn.wgrad_partials_transpose(32, 64, 16, 16, 5, 2)


def test_partials_depend_on_the_shape_only_and_fit_64_mb(nn):
    T = nn.WGRAD_CHUNK
    for (cin, cout, k, s), L in zip(R.UPS, R.UPS_L):
        P, pairs = nn.wgrad_partials_transpose(32, L, cin, cout, k, s)
        nch = -(-L // T)
        assert P >= 1 and (P - 1) * pairs < 32 * nch <= P * pairs, (cin, cout, k, s, L, P, pairs)  # every pair once, no empty partial
        assert (P, pairs) == nn.wgrad_partials_transpose(32, L, cin, cout, k, s)
        ws = nn.workspace_bytes_transpose(32, L, cin, cout, k, s)
        assert 4 * cin * cout * k <= ws <= 64 << 20, (cin, cout, k, s, L, ws)
        print(f"plan {cin:4d} -> {cout:4d} k {k:2d} s {s} L {L:5d}: P {P:4d} x {pairs:3d} pairs, workspace {ws / 2**20:6.2f} MB")
    # the narrowest layer's long reduction is spread over at least one workgroup per CU
    assert nn.wgrad_partials_transpose(32, 4480, 32, 16, 4, 2)[0] >= 256
    # the plan is the stride-1 layer's for the same reduction: input positions, the shape only
    for (cin, cout, k, s), L in zip(R.UPS, R.UPS_L):
        if k % 2:
            assert nn.wgrad_partials_transpose(32, L, cin, cout, k, s) == nn.wgrad_partials(32, L, cin, cout, k)
    assert nn.wgrad_partials_transpose(2, 129, 24, 8, 4, 2) == (6, 1)
    assert nn.wgrad_partials_transpose(3, 129, 24, 8, 4, 2) != (6, 1)


# ---------------------------------------------------------------------------------------------------------
# the reference, and the bars
# ---------------------------------------------------------------------------------------------------------
def test_layer_ref_agrees_with_finite_differences():
    rs = np.random.RandomState(0)
    B, cin, cout, k, s, L, slope = 2, 3, 2, 4, 2, 7, 0.1
    lengths = [7, 4]
    x = torch.from_numpy(rs.randn(B, cin, L))
    x = torch.where(x.abs() < 0.05, torch.full_like(x, 0.3), x)  # no kink inside a finite-difference step
    w, b, gy = (torch.from_numpy(rs.randn(*sh)) for sh in ((cin, cout, k), (cout,), (B, cout, s * L)))
    y, gx, gw, gb = R.layer_ref(x, w, b, gy, lengths, R.conv_transpose_op(s), slope, torch.float64)
    vi, vo = R.valid_masks(lengths, L, R.conv_transpose_op(s))
    assert not y[(vo == 0).expand_as(y)].any() and not gx[(vi == 0).expand_as(gx)].any()
    assert y[1, :, :s * 4].abs().min() > 0

    def loss(x_, w_, b_):
        return float((R.layer_ref(x_, w_, b_, gy, lengths, R.conv_transpose_op(s), slope, torch.float64)[0] * gy).sum())

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
    # a position beyond its utterance's length has no influence: exactly zero gradient
    assert not gx[1, :, 4:].any()


def test_bars_catch_seeded_defects():
    """an fp32 "kernel result" (torch on the CPU) with one seeded defect fails its bar by a wide margin; the clean one
    passes"""
    rs = np.random.RandomState(3)
    B, cin, cout, k, s, L, slope = 3, 12, 10, 8, 4, 152, 0.1
    lengths = [150, 70, 1]
    pad = (k - s) // 2
    x = torch.from_numpy(rs.randn(B, cin, L).astype(np.float32))
    x[torch.from_numpy(rs.rand(B, cin, L) < 0.05)] = 0.0  # exact zeros: torch's rule there is the slope
    w = torch.from_numpy((rs.uniform(-1, 1, (cin, cout, k)) / np.sqrt(cin * k)).astype(np.float32))
    b = torch.from_numpy(rs.uniform(-1, 1, cout).astype(np.float32))
    gy = torch.from_numpy(rs.randn(B, cout, s * L).astype(np.float32))
    r64 = R.layer_ref(x, w, b, gy, lengths, R.conv_transpose_op(s), slope, torch.float64)
    r32 = R.layer_ref(x, w, b, gy, lengths, R.conv_transpose_op(s), slope, torch.float32)
    kinds = ("act", "act", "weight", "vec")
    for name, kind, y, a, c in zip(("y", "gx", "gw", "gb"), kinds, r32, r64, r32):
        assert not R.check("clean " + name, kind, y.clone(), a, c)
    vi, vo = R.valid_masks(lengths, L, R.conv_transpose_op(s))
    gym, xa = gy * vo, F.leaky_relu(x, slope) * vi
    mask = torch.where(x > 0, 1.0, slope) * vi

    def wide(tag, kind, y, i, margin=10.0):
        m = R.compare(kind, y, r64[i], r32[i])
        print(f"defect: {tag:50s} ratio {m['ratio']:.3g} worst channel {m['ch_ratio']:.3g}")
        assert max(m["ratio"] / R.K_WHOLE, m["ch_ratio"] / R.K_CH) > margin, (tag, m)

    # the weight gradient in the kernel's phase form
    assert not R.check("phase restatement", "weight", R.phase_wgrad(xa, gym, k, s), r64[2], r32[2], verbose=False)
    wide("one phase's taps dropped from gw", "weight", R.phase_wgrad(xa, gym, k, s, drop_phase=1), 2)
    wide("two phases swapped in gw", "weight", R.phase_wgrad(xa, gym, k, s, swap=(0, 2)), 2)
    wide("one phase's plane offset by one in gw", "weight", R.phase_wgrad(xa, gym, k, s, plane_shift=(3, 1)), 2)
    # the mask one column long (t <= len): the column at len of x and the s columns from s len of gy take part
    vi1, vo1 = R.valid_masks([n + 1 for n in lengths], L, R.conv_transpose_op(s))
    vi1, vo1 = vi1[:, :, :L], vo1[:, :, :s * L]
    wide("t <= len in the weight gradient", "weight", R.phase_wgrad(F.leaky_relu(x, slope) * vi1, gy * vo1, k, s), 2)
    plain = F.conv1d(gym, w, stride=s, padding=pad)  # the data gradient before the mask: a stride-s correlation with w[ci][co][kk]
    assert not R.check("strided-conv restatement", "act", plain * mask, r64[1], r32[1], verbose=False)
    long1 = F.conv1d(gy * vo1, w, stride=s, padding=pad) * torch.where(x > 0, 1.0, slope) * vi1
    wide("t <= len in the data gradient", "act", long1, 1)
    wide("flipped tap order in the data gradient", "act", F.conv1d(gym, w.flip(2), stride=s, padding=pad) * mask, 1)
    wide("no leaky-ReLU mask", "act", plain * vi, 1)
    # x = 0 is rare (5 % of the positions): the bar catches it, by a smaller margin
    wide("x = 0 taken as 1", "act", plain * torch.where(x >= 0, 1.0, slope) * vi, 1, margin=1.0)
    yl = r32[0].clone()
    for i, n in enumerate(lengths):  # the forward written one input column long
        if n < L:
            yl[i, :, s * n:s * (n + 1)] = F.conv_transpose1d(F.leaky_relu(x[i:i + 1, :, :n + 1], slope), w, b, stride=s,
                                                             padding=pad)[0, :, s * n:]
    wide("t <= len in the forward", "act", yl, 0)
    wide("bias gradient over the padding too", "vec", gy.sum((0, 2)), 3)
