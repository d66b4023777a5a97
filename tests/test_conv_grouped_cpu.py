"""dissc_amd.nn.conv1d_grouped, nn.mean_pool and nn.discriminator_s without a GPU: what dissc_convggrad_create accepts and
refuses, the partial plan of the weight gradient (a function of the shape only, at most 56 MB of partials) and the workspace, and
the references of tests/test_gpu_conv_grouped.py: the kernels' phase form equals conv_grad_ref.layer_ref in float64 for every
layer, pool_ref equals F.avg_pool1d, the length chain equals torch's output shapes, the restated DiscriminatorS is held to a
golden recorded from the reference's own module (tests/golden/make_disc_s_golden.py), and the bars catch seeded defects."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_grad_harness as H
import conv_grouped_ref as R

LENGTHS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 513, 4481, 8960]


@pytest.fixture(scope="module")
def nn():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import nn
    return nn


# ---------------------------------------------------------------------------------------------------------
# the host-only entries
# ---------------------------------------------------------------------------------------------------------
def _create(lib, *a):
    h = ctypes.c_void_p()
    lib.dissc_convggrad_create.argtypes = [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_void_p)]
    return lib.dissc_convggrad_create(*a, ctypes.byref(h)), h


def test_shape_rules(nn):
    from dissc_amd import lib
    #      k even               k = 43                 stride 3              Cin % groups          Cout / g = 8
    bad = [(16, 16, 4, 1, 1), (16, 16, 43, 1, 1), (16, 16, 5, 3, 1), (15, 16, 5, 1, 2), (16, 16, 5, 1, 2),
           #  k = 1            stride 0 / 8                            Cout % groups        Cin / g = 4        72           144 rows
           (16, 16, 1, 1, 1), (16, 16, 5, 0, 1), (16, 16, 5, 8, 1), (16, 24, 5, 1, 16), (4, 16, 5, 1, 1), (72, 16, 5, 1, 1),
           (16, 144, 5, 1, 1), (16, 16, 5, 1, 0), (0, 16, 5, 1, 1), (16, 65536, 5, 1, 1)]
    for a in bad:
        rc, h = _create(lib, *a)
        assert rc == -1 and h.value is None, a  # DISSC_EINVAL
        assert lib.dissc_last_error().startswith(b"dissc_convggrad_create"), lib.dissc_last_error()
    for a, word in (((16, 16, 4, 1, 1), b"odd"), ((16, 16, 43, 1, 1), b"3 .. 41"), ((16, 16, 5, 3, 1), b"stride 3"),
                    ((15, 16, 5, 1, 2), b"groups must divide"), ((16, 16, 5, 1, 2), b"8 output channels per group")):
        _create(lib, *a)
        assert word in lib.dissc_last_error(), lib.dissc_last_error()
    assert lib.dissc_convggrad_create(16, 16, 5, 1, 1, None) == -1  # a null out
    assert lib.dissc_last_error().startswith(b"dissc_convggrad_create")
    for cin, cout, k, s, g in R.DISC_S + R.SMALL + [(64, 128, 3, 4, 1), (56, 112, 9, 2, 1)]:
        rc, h = _create(lib, cin, cout, k, s, g)
        assert rc == 0 and h.value, (cin, cout, k, s, g)
        nn.CONV1D_GROUPED.destroy(h)
    with pytest.raises(nn.DisscError):
        nn.wgrad_partials_grouped(32, 64, 16, 16, 5, 3, 1)


def test_null_and_unpacked_calls_touch_no_device(nn):
    from dissc_amd import lib
    K = nn.CONV1D_GROUPED
    P, pairs = ctypes.c_int(), ctypes.c_int()
    rc, h = _create(lib, 128, 256, 41, 2, 16)
    assert rc == 0
    assert K.partials(None, 32, 64, ctypes.byref(P), ctypes.byref(pairs)) == -1
    assert K.partials(h, 0, 64, ctypes.byref(P), ctypes.byref(pairs)) == -1
    assert K.partials(h, 32, 64, None, None) == 0
    assert K.workspace_bytes(None, 32, 64) == 0 and K.workspace_bytes(h, 0, 64) == 0
    assert K.forward(h, None, None, None, 1, 192, 96, 192, 1.0, None) == -1
    assert b"dissc_convggrad_set_weights first" in lib.dissc_last_error()
    assert K.forward(h, None, None, None, 1, 192, 92, 192, 1.0, None) == -1  # a row of y holds ceil(192 / 2) = 96
    assert lib.dissc_last_error().startswith(b"dissc_convggrad_forward") and b"row strides" in lib.dissc_last_error()
    assert K.backward(None, None, None, None, 1, 192, 96, 192, 1.0, None, None, None, None, 0, None) == -1
    assert lib.dissc_last_error().startswith(b"dissc_convggrad_backward")
    assert K.set_weights(h, None, None, None) == -1 and K.set_weights(None, None, None, None) == -1
    lib.dissc_convggrad_packed.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.dissc_convggrad_packed.restype = ctypes.c_longlong
    # 16 groups of 8 -> 16 channels, PO = pad = 20: K4 = 11
    assert lib.dissc_convggrad_packed(h, 0, None, None) == 16 * 1 * 2 * 11 * 256
    assert lib.dissc_convggrad_packed(h, 1, None, None) == 16 * 1 * 4 * 11 * 256
    assert lib.dissc_convggrad_packed(None, 0, None, None) == -1 and lib.dissc_convggrad_packed(h, 2, None, None) == -1
    K.destroy(h)
    for fn in (lib.dissc_mean_pool_fwd, lib.dissc_mean_pool_bwd):
        assert fn(None, None, None, 1, 1, 16, 16, 12, None) == -1
        assert lib.dissc_last_error().startswith(b"dissc_mean_pool")


def test_partials_depend_on_the_shape_only_and_stay_under_56_mb(nn):
    T = nn.WGRAD_CHUNK
    rup = lambda x, m: (x + m - 1) // m * m
    for scale_rows in (R.TRAIN_L, [4481, 4481, 2241, 1121, 281, 71]):
        for (cin, cout, k, s, g), L in zip(R.DISC_S, scale_rows):
            B = 64
            P, pairs = nn.wgrad_partials_grouped(B, L, cin, cout, k, s, g)
            nch = R.cdiv(R.cdiv(L, s), T)  # chunks of OUTPUT positions
            assert P >= 1 and (P - 1) * pairs < B * nch <= P * pairs, (cin, cout, L, P, pairs)  # every pair once, no empty partial
            assert (P, pairs) == nn.wgrad_partials_grouped(B, L, cin, cout, k, s, g)
            gw_bytes = cout * (cin // g) * k * 4
            assert P * gw_bytes <= 56 << 20, (cin, cout, P)
            ws = nn.workspace_bytes_grouped(B, L, cin, cout, k, s, g)
            assert ws == rup(P * gw_bytes, 256) + rup(B * cout * 8, 256) + 256, (cin, cout, ws)
            assert ws <= 64 << 20
            print(f"plan {cin:4d} -> {cout:4d} k {k} s {s} g {g:2d} L {L:5d}: P {P:4d} x {pairs:4d} pairs, workspace {ws / 2**20:6.2f} MB")
    assert nn.wgrad_partials_grouped(64, 140, 1024, 1024, 41, 1, 16)[0] <= 5  # a 10.7 MB gradient
    assert nn.wgrad_partials_grouped(2, 388, 16, 32, 7, 2, 2) != nn.wgrad_partials_grouped(3, 388, 16, 32, 7, 2, 2)


# ---------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,k,s,g", R.DISC_S + R.SMALL)
def test_phase_form_equals_layer_ref_in_float64(cin, cout, k, s, g):
    lengths, spec = [44, 2 * s + 1, 1, 41], H.Spec("grouped", cin, cout, k, s, g)
    x, w, b, gy = (t.double() for t in H.case(spec, len(lengths), 44, seed=cin + k + s))
    y64, _, gw64, _ = R.layer_ref(x, w, b, gy, lengths, spec.op, 0.1, torch.float64)
    vi, _ = R.valid_masks(lengths, 44, spec.op)
    y, gw = R.phase_layer(F.leaky_relu(x, 0.1) * vi.double(), w, b, gy, lengths, s, g)
    assert float((y - y64).abs().max()) <= 1e-12 * max(1.0, float(y64.abs().max()))
    assert float((gw - gw64).abs().max()) <= 1e-12 * max(1.0, float(gw64.abs().max()))
    pad = (k - 1) // 2
    assert all(kk - pad == s * dl + p and 0 <= p < s for kk, (p, dl) in enumerate(R.taps(k, s)))


def test_pool_ref_equals_avg_pool1d():
    for n in list(range(1, 10)) + [513]:
        rs = np.random.RandomState(n)
        wav = torch.from_numpy(rs.randn(1, 1, n)).requires_grad_(True)
        ref = F.avg_pool1d(wav, 4, 2, padding=2)
        assert ref.shape[2] == R.pool_len(n) == n // 2 + 1
        g = torch.from_numpy(rs.randn(1, 1, R.ceil4(n // 2 + 1)))
        (ref * g[:, :, :ref.shape[2]]).sum().backward()
        out, gx = R.pool_ref(wav, None, g)
        assert float((out[:, :, :ref.shape[2]] - ref.detach()).abs().max()) <= 1e-15 and not out[:, :, ref.shape[2]:].any()
        assert float((gx - wav.grad).abs().max()) <= 1e-15
    # a ragged batch: every utterance alone, zero-padded at its own end
    wav = torch.from_numpy(np.random.RandomState(0).randn(3, 1, 9))
    out, _ = R.pool_ref(wav, [9, 4, 0])
    assert torch.equal(out[1, 0, :3], F.avg_pool1d(wav[1:2, :, :4], 4, 2, padding=2)[0, 0]) and not out[1, 0, 3:].any() and not out[2].any()


def test_length_chain_equals_torch_output_shapes():
    for n in LENGTHS:
        x, got = torch.zeros(1, 1, n), []
        for s, _, k in R.layer_params():
            x = F.conv1d(x, torch.zeros(1, 1, k), stride=s, padding=(k - 1) // 2)
            got.append(x.shape[2])
        assert got == R.map_lengths(n), n
        assert F.avg_pool1d(torch.zeros(1, 1, n), 4, 2, padding=2).shape[2] == R.pool_len(n)
    assert R.map_lengths(8960) == [8960, 4480, 2240, 560, 140, 140, 140, 140]
    assert R.map_lengths(513)[-1] == 9
    assert R.TRAIN_L == [8960] + R.map_lengths(8960)[:5]


def test_restated_discriminator_s_is_held_to_the_reference_golden(golden_dir):
    """the fixture holds what the reference's own DiscriminatorS returned for disc_s_weights(seed): results only"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_disc_s_golden", os.path.join(golden_dir, "make_disc_s_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)  # SEEDS, T and the seeded waveform; main(), which needs the reference, is not run
    path = os.path.join(golden_dir, "disc_s.npz")
    assert os.path.getsize(path) < 100 * 1024
    gold = np.load(path)
    for seed in mk.SEEDS:
        w = R.disc_s_weights(seed, torch.float64)
        wav = mk.wave(seed)
        maps = R.disc_s_chain(w, wav)
        ragged = R.disc_s_ragged(w, torch.cat([wav, F.pad(wav[:, :, :300], (0, mk.T - 300))]), [mk.T, 300])
        assert gold[f"s{seed}/score"].shape == (9,)
        assert np.abs(maps[7].reshape(-1).numpy() - gold[f"s{seed}/score"]).max() <= 1e-12
        for j, m in enumerate(maps):
            r = m if j == 7 else F.leaky_relu(m, R.SLOPE)  # the reference appends the activated map
            assert list(r.shape) == list(gold[f"s{seed}/map{j}/shape"]), j
            s_ref, a_ref = gold[f"s{seed}/map{j}/sum"]
            assert abs(r.sum().item() - s_ref) <= 1e-11 * a_ref and abs(r.abs().sum().item() - a_ref) <= 1e-11 * a_ref, j
            assert np.abs(r.reshape(-1)[:16].numpy() - gold[f"s{seed}/map{j}/head"]).max() <= 1e-12, j
            # the ragged composition: row 0 is the chain, zero beyond its length; row 1 is the chain of the shorter utterance
            n0 = m.shape[2]
            assert torch.equal(ragged[j][0:1, :, :n0], m) and not ragged[j][0, :, n0:].any()
            n1 = R.map_lengths(300)[j]
            assert not ragged[j][1, :, n1:].any() and ragged[j][1, :, :n1].abs().min() > 0
        assert torch.equal(ragged[7][1:2, :, :R.map_lengths(300)[7]], R.disc_s_chain(w, wav[:, :, :300])[7])


# ---------------------------------------------------------------------------------------------------------
# the bars
# ---------------------------------------------------------------------------------------------------------
def test_bars_catch_seeded_defects(nn):
    """an fp32 "kernel result" (torch on the CPU, in the kernels' phase form) with one seeded defect misses its K = 4 bar by at
    least 10 x on the ragged case tests/test_gpu_conv_grouped.py runs; the clean one passes"""
    spec, slope = H.Spec("grouped", 24, 48, 41, 4, 3), 0.1
    s, g = spec.p, spec.groups
    lengths, ld, _ = H.lengths_for(nn, spec)
    x, w, b, gy = H.case(spec, len(lengths), ld, seed=5)
    r64 = R.layer_ref(x, w, b, gy, lengths, spec.op, slope, torch.float64)
    r32 = R.layer_ref(x, w, b, gy, lengths, spec.op, slope, torch.float32)
    for name, kind, y, a, c in zip(("y", "gx", "gw", "gb"), ("act", "act", "weight", "vec"), r32, r64, r32):
        assert not R.check("clean " + name, kind, y.clone(), a, c)
    vi, vo = R.valid_masks(lengths, ld, spec.op)
    xa = F.leaky_relu(x, slope) * vi

    def wide(tag, kind, y, a, c, margin=10.0):
        m = R.compare(kind, y, a, c)
        print(f"defect: {tag:50s} ratio {m['ratio']:.3g} worst channel {m['ch_ratio']:.3g}")
        assert max(m["ratio"] / R.K_WHOLE, m["ch_ratio"] / R.K_CH) > margin, (tag, m)

    y, gw = R.phase_layer(xa, w, b, gy, lengths, s, g)
    assert not R.check("phase restatement y", "act", y, r64[0], r32[0], verbose=False)
    assert not R.check("phase restatement gw", "weight", gw, r64[2], r32[2], verbose=False)
    for tag, kw in (("a dropped tap", {"drop_tap": 17}), ("a tap's shift off by one", {"tap_shift": (30, 1)}),
                    ("group g reads group g + 1's input channels", {"next_group": True}),
                    ("floor(n / s) outputs in place of ceil", {"floor_len": True}), ("padding 19 for 20", {"pad": 19})):
        y, gw = R.phase_layer(xa, w, b, gy, lengths, s, g, **kw)
        wide(tag + " in y", "act", y, r64[0], r32[0])
        wide(tag + " in gw", "weight", gw, r64[2], r32[2])
    # the pool dividing by the number of valid taps (count_include_pad=False)
    n = [0, 1, 2, 3, 4, 5, 8, 9, 513]
    wav = torch.from_numpy(np.random.RandomState(9).randn(len(n), 1, 513).astype(np.float32))
    p64, p32 = R.pool_ref(wav.double(), n)[0], R.pool_ref(wav, n)[0]
    assert not R.check("clean pool", "act", p32.clone(), p64, p32)
    wide("the pool divides by the valid taps", "act", R.pool_ref(wav, n, valid_taps=True)[0], p64, p32)
