"""CPU checks of what tests/test_gpu_msd.py measures dissc_amd.nn.SpectralNorm and nn.MultiScaleDiscriminator against: the torch
restatement of tests/msd_cases.py equals the REFERENCE's own module (tests/golden/msd.npz: two training-mode forwards, four power
iterations) at float64 round-off; the hand-written float64 spectral norm (snorm_ref) and its gradient formula equal torch's
spectral_norm in both modes; every seeded defect is reported by the assertion meant for it; the lengths table of the three scales
is what torch's own layers give for ragged inputs."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_grouped_ref as R
import msd_cases as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msd.npz")
TOL = 1e-11  # relative, float64: sums of up to 5 120 products behind eight layers


def _close(a, b, tol=TOL):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= tol * max(1.0, float(np.abs(b).max()))))


# ---- 1. the restatement against the reference's own module ------------------------------------------------------------------------
def golden_violations(one_sigma=False):
    """runs the restatement twice as make_msd_golden.py runs the reference -> the names of what differs from msd.npz"""
    g = np.load(GOLDEN)
    rs = np.random.RandomState(1000)
    y, y_hat = (torch.from_numpy(rs.uniform(-1, 1, (1, 1, 1030))) for _ in range(2))
    m = M.torch_msd(M.msd_state_dict(0), torch.float64)
    bad = []
    for f in range(2):
        with torch.no_grad():
            maps = m(y, y_hat, one_sigma=one_sigma)
        for i in range(3):
            for h, half in enumerate("rg"):
                pre = f"f{f}/d{i}/{half}"
                for j in range(8):
                    shape = tuple(g[f"{pre}/map{j}/shape"])
                    x = maps[i][j][h:h + 1, :, :shape[2]]
                    assert not maps[i][j][h:h + 1, :, shape[2]:].any()  # the restatement's rows are padded with zeros
                    x = F.leaky_relu(x, R.SLOPE) if j < 7 else x        # the reference returns the activated maps
                    ok = tuple(x.shape) == shape and _close([x.sum().item(), x.abs().sum().item()], g[f"{pre}/map{j}/sum"]) and \
                        _close(x.reshape(-1)[:16].numpy(), g[f"{pre}/map{j}/head"])
                    if not ok:
                        bad.append(f"{pre}/map{j}")
                if not _close(maps[i][7][h, 0, :len(g[pre + "/score"])].numpy(), g[pre + "/score"]):
                    bad.append(pre + "/score")
        for j, (name, conv) in enumerate(m.discriminators[0].named_convs()):
            for what in ("weight_u", "weight_v"):
                t = getattr(conv, what).detach()
                k = f"f{f}/{name}/{what}"
                ok = _close(t.numpy(), g[k], 1e-7) and _close([t.sum().item(), t.abs().sum().item()], g[k + "/sum"]) and \
                    _close(t[:16].numpy(), g[k + "/head"])
                if not ok:
                    bad.append(k)
            if not _close([m.sigmas[1, j].item()], g[f"f{f}/{name}/sigma"]):
                bad.append(f"f{f}/{name}/sigma")
    return bad


def test_restatement_equals_the_reference_after_one_and_two_forwards():
    assert golden_violations() == []


def test_one_sigma_for_both_halves_is_not_the_reference():
    bad = golden_violations(one_sigma=True)
    # the real half and scales 1 and 2 are untouched; the generated half of scale 0 and everything the lost iteration feeds differ
    assert "f0/d0/g/map0" in bad and "f0/d0/g/score" in bad and "f0/convs.0/sigma" in bad
    assert not any(k.startswith(("f0/d0/r", "f0/d1", "f0/d2", "f1/d1", "f1/d2")) for k in bad)


# ---- 2. spectral norm by hand against torch's ---------------------------------------------------------------------------------------
def _torch_snorm(W, u, v, iterate, gw):
    """torch.nn.utils.spectral_norm on a Conv1d(4, 16, 5) holding W [16, 20], in float64 -> (w, u, v, sigma, weight_orig.grad)"""
    conv = torch.nn.utils.spectral_norm(torch.nn.Conv1d(4, 16, 5)).double()
    with torch.no_grad():
        conv.weight_orig.copy_(W.reshape(16, 4, 5))
        conv.weight_u.copy_(u)
        conv.weight_v.copy_(v)
    conv.train(iterate)
    w = M._sn_hook(conv).compute_weight(conv, do_power_iteration=iterate)
    (w.reshape(16, 20) * gw).sum().backward()
    sigma = torch.dot(conv.weight_u, torch.mv(W, conv.weight_v))
    return w.detach().reshape(16, 20), conv.weight_u.clone(), conv.weight_v.clone(), sigma, conv.weight_orig.grad.reshape(16, 20)


def snorm_violations(iterate, defect=None):
    """the names of snorm_ref's results that differ from torch's at float64 round-off"""
    rs = np.random.RandomState(3)
    W, gw = torch.from_numpy(rs.randn(16, 20)), torch.from_numpy(rs.randn(16, 20))
    u, v = (torch.from_numpy(x / np.sqrt((x * x).sum())) for x in (rs.randn(16), rs.randn(20)))
    got = M.snorm_ref(W, u, v, iterate, gw, defect)
    want = _torch_snorm(W, u, v, iterate, gw)
    return [name for name, a, b in zip(("w", "u", "v", "sigma", "gW"), got, want) if not _close(a.numpy(), b.numpy(), 1e-12)]


@pytest.mark.parametrize("iterate", [True, False])
def test_snorm_ref_equals_torch_spectral_norm(iterate):
    assert snorm_violations(iterate) == []


# defect -> (the mode it shows in, the assertion meant for it)
MEANT = {"skip_second_normalize": (True, "u"), "sigma_from_u_in": (True, "sigma"), "drop_uv_term": (False, "gW"),
         "float_reciprocal": (False, "w")}


@pytest.mark.parametrize("defect", sorted(MEANT))
def test_every_seeded_defect_is_reported_by_the_assertion_meant_for_it(defect):
    iterate, name = MEANT[defect]
    bad = snorm_violations(iterate, defect)
    assert name in bad
    if defect == "drop_uv_term":
        assert bad == ["gW"]
    if defect == "float_reciprocal":
        assert bad == ["w"]
    assert set(MEANT) | {"one_sigma"} == set(M.DEFECTS)  # one_sigma: test_one_sigma_for_both_halves_is_not_the_reference


# ---- 3. the lengths of all three scales ------------------------------------------------------------------------------------------------
def test_lengths_table_of_the_three_scales_for_ragged_inputs():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import nn
    lengths, T = [1030, 517, 130, 1, 0], 1030
    table = nn.msd_row_lengths(lengths)
    want = M.map_lens(lengths, len(lengths), T)
    for i in range(3):
        assert len(table[i]) == 7 and all(t.shape == (2 * len(lengths),) for t in table[i])
        assert [int(n) for n in table[i][0][:len(lengths)]] == M.scale_lengths(lengths, len(lengths), T)[i]
        for j in range(8):
            got = table[i][min(j + 1, 6)]
            assert [int(n) for n in got[:len(lengths)]] == [int(n) for n in got[len(lengths):]] == want[i][j], (i, j)
    # and what torch's own pool and conv arithmetic gives for one utterance of every scale
    for n0 in lengths:
        n = n0
        for i in range(3):
            if i:
                n = F.avg_pool1d(torch.zeros(1, 1, n), 4, 2, padding=2).shape[2] if n else 0
            m = n
            for j, (_, cin, cout, k, s, g) in enumerate(M.LAYERS):
                m = F.conv1d(torch.zeros(1, 1, m), torch.zeros(1, 1, k), stride=s, padding=(k - 1) // 2).shape[2] if m else 0
                assert want[i][j][lengths.index(n0)] == m, (n0, i, j)


def test_the_differentiable_pool_of_the_restatement_is_pool_ref():
    rs = np.random.RandomState(8)
    wav = torch.from_numpy(rs.uniform(-1, 1, (4, 1, 1030)))
    lengths = [1030, 517, 1, 0]
    got = M.pool_ragged(wav, lengths)
    want, _ = R.pool_ref(wav, lengths)
    assert got.shape == want.shape and _close(got.numpy(), want.numpy(), 1e-15)


def test_the_references_own_decisions_reproduce_it():
    """the masked evaluation (branches from a Decisions) with the float64 maps' OWN decisions is the plain evaluation"""
    B, T, L = 2, 260, [260, 131]
    sd = M.msd_state_dict(4)
    y, y_hat = M.wav_pair(5, B, T)
    with torch.no_grad():
        maps = M.torch_msd(sd, torch.float64)(y.double(), y_hat.double(), L)
    dec = M.Decisions(maps)
    plain, masked = M.g_step_ref(sd, y, y_hat, L, torch.float64), M.g_step_ref(sd, y, y_hat, L, torch.float64, decisions=dec)
    for a, b in zip(plain[:4], masked[:4]):
        assert _close(a.numpy(), b.numpy(), 1e-13)
    md, mm = M.d_step_ref(sd, y, y_hat, L, torch.float64), M.d_step_ref(sd, y, y_hat, L, torch.float64, decisions=dec)
    for (k, p), (_, q) in zip(md[0].named_parameters(), mm[0].named_parameters()):
        assert _close(p.grad.numpy(), q.grad.numpy(), 1e-13), k
    # and a flipped decision is seen: the masks do reach the result
    dec.masks[0][3] = ~dec.masks[0][3]
    flipped = M.g_step_ref(sd, y, y_hat, L, torch.float64, decisions=dec)
    assert not _close(plain[3].numpy(), flipped[3].numpy(), 1e-6)
