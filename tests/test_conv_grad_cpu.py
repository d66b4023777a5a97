"""dissc_amd.nn without a GPU: what dissc_convgrad_create refuses and accepts, the partial plan of the weight gradient
(a function of the shape only, inside 64 MB for the generator), and the reference of tests/test_gpu_conv_grad.py:
conv_grad_ref.layer_ref agrees with finite differences in float64, the bars it is used with catch seeded defects, and the
harness the four conv-layer GPU files call (conv_grad_harness: lengths_for, assert_layer_gradients) keeps its pinned lengths,
passes the reference for every kind and reports each seeded defect by the one assertion meant for it."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_grad_harness as H
import conv_grad_ref as R


@pytest.fixture(scope="module")
def nn():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import nn
    return nn


def _create(lib, cin, cout, k, d):
    h = ctypes.c_void_p()
    rc = lib.dissc_convgrad_create(cin, cout, k, d, ctypes.byref(h))
    return rc, h


def test_invalid_shapes_are_refused_and_the_generators_accepted(nn):
    from dissc_amd import lib
    assert lib.dissc_abi_version() >= 5
    bad = [(16, 16, 4, 1), (16, 16, 0, 1), (16, 16, 13, 1), (16, 16, 11, 7), (16, 16, 3, 31), (16, 16, 7, 11), (0, 16, 3, 1),
           (16, 0, 3, 1), (-1, 16, 3, 1), (16, 16, 3, 0), (16, 16, -3, 1)]
    for cin, cout, k, d in bad:
        rc, h = _create(lib, cin, cout, k, d)
        assert rc == -1 and h.value is None, (cin, cout, k, d)  # DISSC_EINVAL
        assert b"dissc_convgrad_create" in lib.dissc_last_error()
    assert lib.dissc_convgrad_create(16, 16, 3, 1, None) == -1
    # the limits themselves: k = 11 with span 60, one channel
    for cin, cout, k, d in [(16, 16, 11, 6), (1, 1, 1, 1), (16, 16, 3, 30)]:
        rc, h = _create(lib, cin, cout, k, d)
        assert rc == 0 and h.value, (cin, cout, k, d)
        lib.dissc_convgrad_destroy(h)
    P, pairs = ctypes.c_int(), ctypes.c_int()
    for cin, cout, k, d, L in R.generator_layer_shapes():
        rc, h = _create(lib, cin, cout, k, d)
        assert rc == 0 and h.value, (cin, cout, k, d)
        assert lib.dissc_convgrad_partials(h, 32, L, ctypes.byref(P), ctypes.byref(pairs)) == 0 and P.value >= 1
        assert lib.dissc_convgrad_partials(h, 0, L, ctypes.byref(P), ctypes.byref(pairs)) == -1
        assert lib.dissc_convgrad_partials(h, 32, 0, ctypes.byref(P), ctypes.byref(pairs)) == -1
        # nothing was packed: forward and backward refuse before any launch
        assert lib.dissc_convgrad_forward(h, None, None, None, None, 1, 64, 64, 64, 1.0, None) == -1
        assert lib.dissc_convgrad_backward(h, None, None, None, 1, 64, 64, 64, 1.0, None, None, None, None, 0, None) == -1
        lib.dissc_convgrad_destroy(h)
    assert lib.dissc_convgrad_partials(None, 32, 64, ctypes.byref(P), ctypes.byref(pairs)) == -1
    assert lib.dissc_convgrad_workspace_bytes(None, 32, 64) == 0
    with pytest.raises(nn.DisscError):
        nn.wgrad_partials(32, 64, 16, 16, 4)


def test_partials_depend_on_the_shape_only_and_fit_64_mb(nn):
    assert nn.WGRAD_CHUNK == 64
    shapes = R.generator_layer_shapes(28)
    assert len({s[:3] + s[4:] for s in shapes}) == 17 and len(shapes) == 47  # conv_pre, 5 stages x 3 kernels, conv_post
    assert max(s[4] for s in shapes) == 8960
    for cin, cout, k, d, L in shapes:
        P, pairs = nn.wgrad_partials(32, L, cin, cout, k)
        nch = -(-L // nn.WGRAD_CHUNK)
        assert P >= 1 and (P - 1) * pairs < 32 * nch <= P * pairs, (cin, cout, k, L, P, pairs)  # every pair once, no empty partial
        assert (P, pairs) == nn.wgrad_partials(32, L, cin, cout, k)
        ws = nn.workspace_bytes(32, L, cin, cout, k)
        assert 4 * cin * cout * k <= ws <= 64 << 20, (cin, cout, k, L, ws)
        print(f"plan {cin:4d} -> {cout:4d} k {k:2d} L {L:5d}: P {P:4d} x {pairs:3d} pairs, workspace {ws / 2**20:6.2f} MB")
    # the narrow layers' long reductions are spread over at least one workgroup per CU
    assert nn.wgrad_partials(32, 8960, 16, 16, 11)[0] >= 256 and nn.wgrad_partials(32, 4480, 32, 32, 11)[0] >= 256
    # a different batch or length is a different plan; the dilation is not part of it
    assert nn.wgrad_partials(2, 129, 16, 16, 3) == (6, 1)


# ---------------------------------------------------------------------------------------------------------
# the reference, and the bars
# ---------------------------------------------------------------------------------------------------------
def test_layer_ref_agrees_with_finite_differences():
    rs = np.random.RandomState(0)
    B, cin, cout, k, d, L, slope = 2, 3, 2, 3, 2, 9, 0.1
    lengths = [9, 5]
    x = torch.from_numpy(rs.randn(B, cin, L))
    x = torch.where(x.abs() < 0.05, torch.full_like(x, 0.3), x)  # no kink inside a finite-difference step
    w, b, gy = (torch.from_numpy(rs.randn(*s)) for s in ((cout, cin, k), (cout,), (B, cout, L)))
    y, gx, gw, gb = R.layer_ref(x, w, b, gy, lengths, R.conv_op(d), slope, torch.float64)
    valid = torch.zeros(B, 1, L, dtype=torch.bool)
    for i, n in enumerate(lengths):
        valid[i, :, :n] = True
    assert not y[~valid.expand_as(y)].any() and not gx[~valid.expand_as(gx)].any()

    def loss(x_, w_, b_):
        return float((R.layer_ref(x_, w_, b_, gy, lengths, R.conv_op(d), slope, torch.float64)[0] * gy).sum())

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
    assert not gx[1, :, 5:].any()


def _setup(seed=3):
    rs = np.random.RandomState(seed)
    B, cin, cout, k, d, L, slope = 3, 12, 10, 5, 2, 152, 0.1
    lengths = [150, 70, 1]
    x = torch.from_numpy(rs.randn(B, cin, L).astype(np.float32))
    x[torch.from_numpy(rs.rand(B, cin, L) < 0.05)] = 0.0  # exact zeros: torch's rule there is the slope
    w = torch.from_numpy((rs.uniform(-1, 1, (cout, cin, k)) / np.sqrt(cin * k)).astype(np.float32))
    b = torch.from_numpy(rs.uniform(-1, 1, cout).astype(np.float32))
    gy = torch.from_numpy(rs.randn(B, cout, L).astype(np.float32))
    return B, cin, cout, k, d, L, slope, lengths, x, w, b, gy


def test_bars_catch_seeded_defects():
    """an fp32 "kernel result" (torch on the CPU) with one seeded defect fails its bar; the clean one passes"""
    B, cin, cout, k, d, L, slope, lengths, x, w, b, gy = _setup()
    pad = (k - 1) * d // 2
    r64 = R.layer_ref(x, w, b, gy, lengths, R.conv_op(d), slope, torch.float64)
    r32 = R.layer_ref(x, w, b, gy, lengths, R.conv_op(d), slope, torch.float32)
    Y = [t.clone() for t in r32]
    kinds = ("act", "act", "weight", "vec")
    for name, kind, y, a, c in zip(("y", "gx", "gw", "gb"), kinds, Y, r64, r32):
        assert not R.check("clean " + name, kind, y, a, c)
    valid = torch.zeros(B, 1, L)
    for i, n in enumerate(lengths):
        valid[i, :, :n] = 1
    gym, xa = gy * valid, F.leaky_relu(x, slope) * valid

    def terms(bs, t0, t1, dil=d):  # the weight gradient's terms of utterances bs, positions t0 .. t1 - 1
        p = (k - 1) * dil // 2
        xp = F.pad(xa, (p, p))
        return torch.stack([torch.einsum("bot,bit->oi", gym[bs, :, t0:t1], xp[bs, :, t0 + j * dil:t1 + j * dil]) for j in range(k)], -1)

    full = terms(slice(None), 0, L)
    assert not R.check("einsum restatement", "weight", full, r64[2], r32[2], verbose=False)

    def fails(tag, kind, y, i):
        bad = R.check("defect: " + tag, kind, y, r64[i], r32[i])
        assert bad, tag

    mask = torch.where(x > 0, 1.0, slope) * valid
    plain = F.conv1d(gym, w.transpose(0, 1).flip(2).contiguous(), padding=pad, dilation=d) * valid  # before the mask
    assert not R.check("conv^T restatement", "act", plain * mask, r64[1], r32[1], verbose=False)
    fails("taps not flipped", "act", F.conv1d(gym, w.transpose(0, 1).contiguous(), padding=pad, dilation=d) * valid * mask, 1)
    fails("one partial dropped", "weight", Y[2] - terms(slice(1, 2), 0, 64), 2)
    fails("last chunk dropped", "weight", Y[2] - terms(slice(0, 1), 128, 150), 2)
    fails("last column of a chunk dropped", "weight", Y[2] - terms(slice(0, 1), 63, 64), 2)
    fails("dilation 1 in the weight gradient", "weight", terms(slice(None), 0, L, dil=1), 2)
    fails("no leaky-ReLU mask", "act", plain, 1)
    fails("x = 0 taken as 1", "act", plain * torch.where(x >= 0, 1.0, slope) * valid, 1)
    fails("activation missing in the weight gradient", "weight",
          torch.stack([torch.einsum("bot,bit->oi", gym, F.pad(x * valid, (pad, pad))[:, :, j * d:j * d + L]) for j in range(k)], -1), 2)
    fails("bias gradient over the padding too", "vec", gy.sum((0, 2)), 3)


def test_resblock_ref_masks():
    """with the masks of its own inputs resblock1_ref equals the unmasked block; the engine's masks make float64 take
    the engine's branches (the backward is then linear in its inputs)"""
    rs = np.random.RandomState(1)
    Cc, k, L = 4, 3, 21
    w = {}
    for m in range(3):
        for c in ("convs1", "convs2"):
            w[f"{c}.{m}.weight"] = torch.from_numpy(rs.uniform(-1, 1, (Cc, Cc, k)) / np.sqrt(Cc * k))
            w[f"{c}.{m}.bias"] = torch.from_numpy(rs.uniform(-1, 1, Cc))
    x, gy = torch.from_numpy(rs.randn(2, Cc, L)), torch.from_numpy(rs.randn(2, Cc, L))
    lengths = [21, 6]
    y, gx, g = R.resblock1_ref(w, x, k, (1, 3, 5), torch.float64, lengths=lengths, gy=gy)
    # its own pre-activations, taken from a second evaluation
    taps, h = [], x.clone()
    valid = torch.zeros(2, 1, L, dtype=torch.bool)
    for i, n in enumerate(lengths):
        valid[i, :, :n] = True
    for m, d in enumerate((1, 3, 5)):
        taps.append(h)
        t = torch.zeros_like(h)
        for i, n in enumerate(lengths):
            t[i:i + 1, :, :n] = F.conv1d(F.leaky_relu(h[i:i + 1, :, :n], 0.1), w[f"convs1.{m}.weight"], w[f"convs1.{m}.bias"],
                                         padding=(k - 1) * d // 2, dilation=d)
        taps.append(t)
        u = torch.zeros_like(h)
        for i, n in enumerate(lengths):
            u[i:i + 1, :, :n] = F.conv1d(F.leaky_relu(t[i:i + 1, :, :n], 0.1), w[f"convs2.{m}.weight"], w[f"convs2.{m}.bias"],
                                         padding=(k - 1) // 2) + h[i:i + 1, :, :n]
        h = u
    assert torch.equal(h * valid, y)
    masks = [t > 0 for t in taps]
    y2, gx2, g2 = R.resblock1_ref(w, x, k, (1, 3, 5), torch.float64, masks=masks, lengths=lengths, gy=gy)
    assert torch.equal(y2, y) and torch.equal(gx2, gx) and all(torch.equal(g2[n], g[n]) for n in g)
    flipped = [~m for m in masks]
    assert not torch.equal(R.resblock1_ref(w, x, k, (1, 3, 5), torch.float64, masks=flipped, lengths=lengths), y)


# ---------------------------------------------------------------------------------------------------------
# the harness of the four GPU files (tests/conv_grad_harness.py)
# ---------------------------------------------------------------------------------------------------------
def test_lengths_for_keeps_its_pinned_lists(nn):
    """the measured ratios of profiles/*.md belong to these lengths: the widest strided layer at max_b = 4, and a grouped layer
    whose plan (23 partials of 2 pairs over 15 x 3 chunks) puts partial boundaries inside utterances"""
    assert H.lengths_for(nn, H.Spec("strided", 512, 1024, 5, 3), max_b=4) == ([4, 383, 192, 385], 388, (4, 3))
    assert H.lengths_for(nn, H.Spec("grouped", 128, 128, 41, 2, 4)) == \
        ([1, 2, 2, 3, 20, 21, 41, 129, 128, 129, 257, 256, 255, 128, 127], 260, (23, 2))


def _stand_in(spec, defect=None):
    """conv_grad_harness.run's contract on the CPU: the float32 reference, with one seeded defect"""
    calls = []

    def run(x, w, b, gy, lengths, slope, add=None, need=(True, True, True), nan_workspace=False):
        y, gx, gw, gb = (t.clone() for t in R.layer_ref(x, w, b, gy, lengths, spec.op, slope, torch.float32))
        vi, vo = R.valid_masks(lengths, x.shape[2], spec.op)
        calls.append(lengths)
        alone = len(lengths) == 1
        if add is not None:
            y += add * vo
        if defect == "gx beyond a length" and not alone:
            gx[1, 0, lengths[1]] = 1e-3
        if defect == "gw reads beyond the lengths":  # too small to move a bit of gw until the poison arrives
            gw.view(-1)[0] += 1e-12 * float((x * (1 - vi)).sum())
        if defect == "one tap of gw zeroed" or (defect == "one tap of gw zeroed in one utterance alone" and lengths == [4]):
            gw[:, :, 1] = 0
        if defect == "y differs on the second call" and len(calls) == 2:
            y[0, 0, 0] += 1e-3
        if defect == "the workspace is read before it is written" and nan_workspace:
            gb[0] += 1e-3
        if defect == "gw depends on whether gx is wanted" and not need[0]:
            gw[0, 0, 0] += 1e-3
        if defect == "alone y differs" and alone:
            y[0, 0, 0] += 1e-3
        if defect == "alone gx differs" and alone:
            gx[0, 0, 0] += 1e-3
        gadd = None if add is None else gy * (0.5 if defect == "the gradient of add is halved" else 1.0)
        return [y] + [g if on else None for g, on in zip((gx, gw, gb), need)] + [gadd]
    return run


SPECS = [H.Spec("conv1d", 3, 2, 3, 1), H.Spec("transposed", 3, 2, 4, 2), H.Spec("strided", 3, 2, 3, 2), H.Spec("grouped", 4, 4, 3, 2, 2)]
DEFECTS = [("gx beyond a length", "beyond the lengths"), ("gw reads beyond the lengths", "poison beyond the lengths changes gw"),
           ("one tap of gw zeroed", "batch gw"), ("y differs on the second call", "y is not bit-reproducible"),
           ("the workspace is read before it is written", "a workspace full of NaNs changes gb"),
           ("gw depends on whether gx is wanted", r"needs_input_grad \(False, True, True\): gw"),
           ("alone gx differs", "alone gx differs from the batch's"),
           ("one tap of gw zeroed in one utterance alone", r"^\[\('alone len 4 gw'")]


@pytest.mark.parametrize("spec", SPECS, ids=["conv1d", "conv_transpose1d", "conv1d_strided", "conv1d_grouped"])
def test_harness_passes_the_reference_and_catches_seeded_defects(spec):
    """assert_layer_gradients, as the four GPU files call it, passes the float32 reference of every kind, and each of its
    assertions reports the defect seeded for it -- and no other assertion does: the message is the first one raised"""
    lengths, ld = [9, 4, 1], 12
    H.assert_layer_gradients(_stand_in(spec), spec, lengths, ld, seed=5)
    own = [("the gradient of add is halved", "the gradient of add is gy itself")] if spec.kind == "conv1d" else \
        [("alone y differs", "alone y differs from the batch's")]  # (the Conv1d's alone runs are made without add)
    for defect, said in DEFECTS + own:
        with pytest.raises(AssertionError, match=said):
            H.assert_layer_gradients(_stand_in(spec, defect), spec, lengths, ld, seed=5)
