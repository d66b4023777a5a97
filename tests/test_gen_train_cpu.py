"""csrc/gen_train.hip and nn.CodeGenerator without a GPU: what the host-only entries refuse, the flat layout of the
multi-tensor weight norm, the ABI number, and the reference of tests/test_gpu_gen_train.py -- gen_train_ref is pinned bit for
bit to oracle.generator_ref on folded weights, its gradients agree with central finite differences in float64, and the bars
it is used with (conv_grad_ref.check at K = 4) catch five seeded defects."""
import ctypes

import numpy as np
import pytest
import torch

import conv_grad_ref as R
import gen_train_ref as GT
import synthdata as synth
from oracle import generator_ref as G


@pytest.fixture(scope="module")
def nn():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import nn
    return nn


def _create(lib, shapes):
    n = len(shapes)
    rows = (ctypes.c_int * max(n, 1))(*[s[0] for s in shapes])
    cols = (ctypes.c_int * max(n, 1))(*[s[1] for s in shapes])
    h = ctypes.c_void_p()
    return lib.dissc_wnorm_create(n, rows, cols, ctypes.byref(h)), h


def test_wnorm_create_refusals(nn):
    from dissc_amd import lib
    big = 2 ** 31 - 1
    for shapes in ([], [(0, 4)], [(4, 0)], [(-1, 4)], [(4, 4), (4, -2)], [(big, 1), (big, 1)], [(big, big)],
                   [(2 ** 22, 1), (1, 1)], [(2 ** 20, 2 ** 20), (1, 1)]):
        rc, h = _create(lib, shapes)
        assert rc == -1 and h.value is None, shapes  # DISSC_EINVAL
        assert b"dissc_wnorm_create" in lib.dissc_last_error()
    rows = (ctypes.c_int * 1)(4)
    assert lib.dissc_wnorm_create(1, rows, rows, None) == -1
    assert lib.dissc_wnorm_create(1, None, rows, ctypes.byref(ctypes.c_void_p())) == -1
    rc, h = _create(lib, [(1, 1)])
    assert rc == 0 and h.value
    # no device pointers: refused before any launch
    assert lib.dissc_wnorm_forward(h, None, None, None, None, None, None, 0, None) == -1
    assert lib.dissc_wnorm_backward(h, None, None, None, None, None, None, None, None, None) == -1
    assert lib.dissc_wnorm_offsets(None, None, None, None, None) == -1
    lib.dissc_wnorm_destroy(h)
    with pytest.raises(nn.DisscError):
        nn.WeightNorm([(3, 0)])


def test_embed_and_rowwise_entries_refuse_bad_arguments_on_the_host(nn):
    from dissc_amd import lib
    p = ctypes.c_void_p(64)  # never dereferenced: every call below is refused before its launch
    ok = dict(B=2, T=8, E=16, n_codes=20, n_spk=200, ldx=8)
    for bad in (dict(B=0), dict(T=0), dict(E=0), dict(n_codes=0), dict(n_spk=0), dict(ldx=7), dict(B=70000), dict(E=40000),
                dict(B=2 ** 20, T=2 ** 20)):
        a = dict(ok, **bad)
        assert lib.dissc_embed_concat_fwd(p, p, p, p, p, None, a["B"], a["T"], a["E"], a["n_codes"], a["n_spk"], p, a["ldx"], None) == -1, bad
        assert b"dissc_embed_concat_fwd" in lib.dissc_last_error()
        assert lib.dissc_embed_concat_bwd(p, p, 1, p, None, a["B"], a["T"], a["E"], a["n_codes"], a["n_spk"], a["ldx"], p, p, None) == -1, bad
        assert b"dissc_embed_concat_bwd" in lib.dissc_last_error()
    # the gradient kernel's table width
    assert lib.dissc_embed_concat_bwd(p, p, 1, p, None, 2, 8, 257, 20, 200, 8, p, p, None) == -1
    assert b"257" in lib.dissc_last_error()
    # null pointers; a speaker id without its table
    assert lib.dissc_embed_concat_fwd(None, p, p, p, p, None, 2, 8, 16, 20, 200, p, 8, None) == -1
    assert lib.dissc_embed_concat_fwd(p, p, p, None, p, None, 2, 8, 16, 20, 200, p, 8, None) == -1
    assert lib.dissc_embed_concat_fwd(p, p, p, p, None, None, 2, 8, 16, 20, 200, p, 8, None) == -1
    assert lib.dissc_embed_concat_fwd(p, p, p, p, p, None, 2, 8, 16, 20, 200, None, 8, None) == -1
    assert lib.dissc_embed_concat_bwd(None, p, 1, p, None, 2, 8, 16, 20, 200, 8, p, p, None) == -1
    assert lib.dissc_embed_concat_bwd(p, p, 1, p, None, 2, 8, 16, 20, 200, 8, p, None, None) == -1
    # MRF mean and tanh: nk outside 1 .. 4, rows that are no multiple of 4, Lmax beyond the row
    ptrs = (ctypes.c_void_p * 4)(64, 64, 64, 64)
    for nk in (0, 5):
        assert lib.dissc_mrf_mean_fwd(ptrs, nk, p, None, 1, 16, 12, 12, None) == -1
        assert lib.dissc_mrf_mean_bwd(p, nk, p, None, 1, 16, 12, 12, None) == -1
    assert lib.dissc_mrf_mean_fwd(ptrs, 2, p, None, 1, 16, 10, 10, None) == -1
    assert lib.dissc_mrf_mean_bwd(p, 2, p, None, 1, 16, 12, 13, None) == -1
    assert lib.dissc_mrf_mean_fwd(None, 2, p, None, 1, 16, 12, 12, None) == -1
    assert lib.dissc_tanh_fwd(p, p, None, 1, 1, 8, 4, 8, None) == -1
    assert lib.dissc_tanh_fwd(p, None, None, 1, 1, 8, 8, 8, None) == -1
    assert lib.dissc_tanh_bwd(p, None, p, None, 1, 1, 8, 8, 8, None) == -1
    assert lib.dissc_tanh_bwd(p, p, p, None, 0, 1, 8, 8, 8, None) == -1


def test_wnorm_layout_and_abi(nn):
    from dissc_amd import lib
    assert lib.dissc_abi_version() == 9
    assert nn.WNORM_WAVE_COLS == lib.dissc_wnorm_wave_cols() and nn.WNORM_WAVE_COLS >= 4
    for shapes in ([(1, 112), (16, 48), (512, 1799), (3, 1)], [(3, 1), (1, 112), (2, 3), (7, 1799)]):
        wn = nn.WeightNorm(shapes)
        end, rend = 0, 0
        for (r, c), off, roff in zip(shapes, wn.off, wn.row_off):
            assert off % 4 == 0 and end <= off < end + 4 and roff == rend, (shapes, wn.off, wn.row_off)
            end, rend = off + r * c, roff + r
        assert wn.total % 4 == 0 and end <= wn.total < end + 4 and wn.total_rows == rend
    assert nn.WeightNorm([(3, 1), (1, 112)]).off == [0, 4]
    # the generator's own: 97 tensors, one slice, about 14 M parameters in 10 433 rows
    g = nn.CodeGenerator(synth.VCTK_CONFIG)
    assert g.wn.n == 97 and g.wn.total_rows == 10433 and 13_600_000 < g.wn.total < 13_800_000
    assert max(c for _, c in g.wn.shapes) == 2816 and min(c for _, c in g.wn.shapes) == 48
    assert (512, 1799) in g.wn.shapes
    for k in ("lambda_commit", "lambda_commit_code", "f0_quantizer_path"):
        with pytest.raises(NotImplementedError):
            nn.CodeGenerator(dict(synth.VCTK_CONFIG, **{k: 1}))
    with pytest.raises(RuntimeError):
        g.parameters()


def _inputs(h, B, T, lengths, seed):
    code, f0, spkr, _ = synth.synth_generator_inputs(B, T, seed=seed, n_spk=200, n_codes=h["num_embeddings"])
    return torch.from_numpy(code), torch.from_numpy(f0), torch.from_numpy(spkr), np.asarray(lengths)


def test_reference_is_pinned_to_the_oracle_bit_for_bit():
    h = GT.SMALL_CONFIG
    sd = synth.synth_generator_state_dict(h, seed=3)
    code, f0, spkr, lengths = _inputs(h, 3, 13, [13, 7, 1], seed=5)
    mine = GT.generator_ref(sd, h, code, f0, spkr, lengths, torch.float32)
    ref = G.code_generator(G.fold_state_dict(sd), h, code, f0, spkr, lengths=lengths)
    assert mine.shape == ref.shape == (3, 1, 8 * 13) and torch.equal(mine, ref) and ref.abs().sum() > 0
    # under autograd, and with its own branch decisions handed back as masks: the same bits
    taps = []
    again, _ = GT.generator_ref(sd, h, code, f0, spkr, lengths, torch.float32, gwav=torch.ones_like(ref), taps=taps)
    assert torch.equal(again, ref) and len(taps) == len(GT.conv_input_rates(h)) == 2 + 2 * 13
    masked = GT.generator_ref(sd, h, code, f0, spkr, lengths, torch.float32, masks=[t > 0 for t in taps])
    assert torch.equal(masked, ref)


def _fd(f, params, grads, n_dir=4, eps=1e-6, seed=0):
    """worst relative gap between d f / d direction by central differences and by ``grads`` over a few random directions"""
    rs = np.random.RandomState(seed)
    worst = 0.0
    for _ in range(n_dir):
        ds = {k: torch.from_numpy(rs.randn(*p.shape)) for k, p in params.items()}
        up = float(f({k: p + eps * ds[k] for k, p in params.items()}))
        dn = float(f({k: p - eps * ds[k] for k, p in params.items()}))
        fd = (up - dn) / (2 * eps)
        an = float(sum((grads[k] * ds[k]).sum() for k in params))
        worst = max(worst, abs(fd - an) / max(abs(fd), abs(an), 1e-12))
    return worst


def test_reference_gradients_agree_with_finite_differences():
    rs = np.random.RandomState(1)
    # weight norm, a ConvTranspose-shaped tensor (dim 0 is the input channel)
    v, g, gw = (torch.from_numpy(rs.randn(*s)) for s in ((5, 3, 4), (5,), (5, 3, 4)))
    _, gv, gg = GT.weight_norm_ref(v, g, gw, torch.float64)
    f = lambda p: (GT.weight_norm_ref(p["v"], p["g"], None, torch.float64)[0] * gw).sum()
    assert _fd(f, {"v": v, "g": g}, {"v": gv, "g": gg}) < 1e-7
    # the embedding scatter: a repeated id, two utterances of one speaker, ragged
    E, B, T, lengths = 3, 3, 6, [6, 4, 0]
    dw, sw, gx, f0 = (torch.from_numpy(rs.randn(*s)) for s in ((5, E), (4, E), (B, 2 * E + 1, T), (B, T)))
    code = torch.tensor([[1, 1, 1, 2, 0, 1], [4, 4, 1, 1, 3, 3], [0, 0, 0, 0, 0, 0]])
    spkr = torch.tensor([2, 2, 1])
    _, gd, gs = GT.embed_ref(dw, sw, code, f0, spkr, lengths, gx, torch.float64)
    f = lambda p: (GT.embed_ref(p["d"], p["s"], code, f0, spkr, lengths, None, torch.float64)[0] * gx).sum()
    assert _fd(f, {"d": dw, "s": sw}, {"d": gd, "s": gs}) < 1e-7
    assert not gd[3].any() and not gs[[0, 1, 3]].any() and gd[1].abs().sum() > 0  # beyond lengths / unused: exact zeros
    # one whole tiny generator, the branch decisions frozen at the unperturbed point (no kink inside a step)
    h = GT.TINY_CONFIG
    sd = {k: t.double() for k, t in synth.synth_generator_state_dict(h, seed=2).items()}
    code, f0, spkr, lengths = _inputs(h, 2, 5, [5, 3], seed=7)
    gwav = torch.from_numpy(rs.randn(2, 1, 10))
    taps = []
    _, grads = GT.generator_ref(sd, h, code, f0, spkr, lengths, torch.float64, gwav=gwav, taps=taps)
    masks = [t > 0 for t in taps]
    f = lambda p: (GT.generator_ref(p, h, code, f0, spkr, lengths, torch.float64, masks=masks) * gwav).sum()
    assert set(grads) == set(sd) and all(float(t.abs().sum()) > 0 for k, t in grads.items() if k != "spkr.weight")
    assert _fd(f, sd, grads, eps=1e-6) < 1e-6


def test_seeded_defects_fail_the_bars():
    rs = np.random.RandomState(2)
    t32 = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32))
    # 1. weight norm's gradient without the v (v . gw) / ||v||^2 term
    v, g, gw = t32(16, 48), t32(16), t32(16, 48)
    w64, gv64, gg64 = GT.weight_norm_ref(v, g, gw, torch.float64)
    w32, gv32, gg32 = GT.weight_norm_ref(v, g, gw, torch.float32)
    assert not R.check("gv", "weight", gv32, gv64, gv32) and not R.check("w", "weight", w32, w64, w32)
    dropped = (g / v.norm(dim=1))[:, None] * gw
    assert R.check("gv, term dropped", "weight", dropped, gv64, gv32)
    # 2. a ConvTranspose's g taken per OUTPUT channel (dim 1) instead of dim 0
    vt, gt = t32(8, 8, 4), t32(8).abs() + 0.5
    wt64, _, _ = GT.weight_norm_ref(vt, gt, None, torch.float64)
    wt32, _, _ = GT.weight_norm_ref(vt, gt, None, torch.float32)
    per_out = torch._weight_norm(vt, gt.reshape(1, 8, 1), 1)
    assert not R.check("w", "weight", wt32, wt64, wt32) and R.check("w, g per output channel", "weight", per_out, wt64, wt32)
    # 3. the MRF mean without 1 / nk
    a, b, c = t32(2, 16, 12), t32(2, 16, 12), t32(2, 16, 12)
    m64, m32 = ((a.double() + b.double()) + c.double()) / 3, ((a + b) + c) / 3
    assert not R.check("mrf", "act", m32, m64, m32) and R.check("mrf, no 1 / nk", "act", (a + b) + c, m64, m32)
    # 4. tanh' as 1 - y
    x, gy = 3 * t32(2, 1, 64), t32(2, 1, 64)
    y64, y32 = torch.tanh(x.double()), torch.tanh(x)
    t64, t32_ = gy.double() * (1 - y64 * y64), gy * (1 - y32 * y32)
    assert not R.check("tanh'", "act", t32_, t64, t32_) and R.check("tanh' as 1 - y", "act", gy * (1 - y32), t64, t32_)
    # 5. the speaker gradient summed over the whole row instead of the utterance's length
    E, B, T, lengths = 4, 2, 12, [12, 5]
    dw, sw, gx, f0 = t32(6, E), t32(3, E), t32(B, 2 * E + 1, T), t32(B, T)
    code, spkr = torch.from_numpy(rs.randint(0, 6, (B, T))), torch.tensor([1, 2])
    _, _, gs64 = GT.embed_ref(dw, sw, code, f0, spkr, lengths, gx, torch.float64)
    _, _, gs32 = GT.embed_ref(dw, sw, code, f0, spkr, lengths, gx, torch.float32)
    whole = torch.zeros_like(gs32)
    for bb in range(B):
        whole[spkr[bb]] += gx[bb, E + 1:].sum(dim=1)
    assert not R.check("g_spkr", "weight", gs32, gs64, gs32) and R.check("g_spkr over ld", "weight", whole, gs64, gs32)
