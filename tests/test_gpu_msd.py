"""dissc_amd.nn.SpectralNorm and nn.MultiScaleDiscriminator on the GPU.  The spectral norm kernels alone (csrc/spectral_norm.hip): w,
u, v, sigma and the gradient against the hand-written float64 form of tests/msd_cases.py with float32 torch as the yardstick, on
shapes that stand at every edge the kernels export (rows per partial chunk, columns per span, the wave / workgroup threshold, the
flat span) and on the module's real eight matrices, in both modes; bit-reproducible, a tensor's results independent of the list
it is in, inputs unchanged, alignment gaps untouched, NULL gradients as zeros, refusals by name.  The module: the discriminator's
and the generator's step against the spectral_norm / weight_norm restatement in float64, the two sigmas of one forward, the
buffers after one, two and three forwards, the composition bit for bit against nn.discriminator_s, param_grads=False, the
checkpoint round trip through one AdamW step, one full alternation with nn.CodeGenerator and both discriminators.  Everything is
held to the project's bars 4 / 4 (tests/train_stage_cases.py) but the eight tensors listed in EXCEPTIONS; the step references
run on the engine's own branch decisions (msd_cases.Decisions); measured ratios: profiles/msd_train.md."""
import numpy as np
import pytest
import torch

import conv_grouped_ref as R
import gan_loss_ref as GL
import gen_train_ref as GT
import mpd_cases as MP
import msd_cases as M
import synthdata as synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def nn():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import nn
    return nn


def bits(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.int32)


# ---- 1. nn.SpectralNorm alone ----------------------------------------------------------------------------------------------------
def edge_shapes(nn):
    """the issue's seven shapes, then for each exported constant a tensor one below, at and one above it"""
    shapes = [(1, 3072), (128, 15), (1, 1), (16, 1), (5, 7), (33, 1025), (257, 64)]
    c = nn.SNORM_CHUNK_ROWS
    shapes += [(c - 1, 20), (c, 20), (c + 1, 20)]
    for c in (nn.SNORM_SPAN_COLS, nn.SNORM_WAVE_COLS):
        shapes += [(3, c - 1), (3, c), (3, c + 1)]
    c = nn.SNORM_FLAT_SPAN
    shapes += [(1, c - 1), (2, c // 2), (1, c + 1)]
    return shapes


def draw(shapes, seed):
    """per tensor (W, u, v, gw) on the host: W uniform / sqrt(cols), u and v unit vectors, gw normal"""
    rs = np.random.RandomState(seed)
    out = []
    for r, c in shapes:
        W = torch.from_numpy((rs.uniform(-1, 1, (r, c)) / np.sqrt(c)).astype(np.float32))
        out.append((W, M._unit(rs, r), M._unit(rs, c), torch.from_numpy(rs.randn(r, c).astype(np.float32))))
    return out


def flat(sn, data, which, offs, total):
    t = torch.zeros(total)
    for o, d in zip(offs, data):
        t[o:o + d[which].numel()] = d[which].reshape(-1)
    return t.to(DEV)


def run_sn(nn, shapes, data, iterate, null=()):
    """forward + backward of one handle -> per tensor (w, u, v, sigma, gW) on the host, and the raw device results"""
    sn = nn.SpectralNorm(shapes)
    Wf, uf, vf = flat(sn, data, 0, sn.off, sn.total), flat(sn, data, 1, sn.u_off, sn.u_total), flat(sn, data, 2, sn.v_off, sn.v_total)
    keep = [t.clone() for t in (Wf, uf, vf)]
    w, state = sn.forward(Wf, uf, vf, iterate)
    gws = [None if i in null else d[3].to(DEV) for i, d in enumerate(data)]
    gW = sn.backward(Wf, state, gws)
    torch.cuda.synchronize()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(keep, (Wf, uf, vf))), "an input buffer was written"
    u, v, sg = sn.split(state)
    per = []
    for i, (r, c) in enumerate(shapes):
        per.append((w[sn.off[i]:sn.off[i] + r * c].view(r, c).cpu(), u[sn.u_off[i]:sn.u_off[i] + r].cpu(),
                    v[sn.v_off[i]:sn.v_off[i] + c].cpu(), sg[i:i + 1].cpu(), gW[sn.off[i]:sn.off[i] + r * c].view(r, c).cpu()))
    return sn, per, (w, state, gW)


def gap_mask(offs, sizes, total):
    m = torch.ones(total, dtype=torch.bool)
    for o, n in zip(offs, sizes):
        m[o:o + n] = False
    return m


@pytest.fixture(scope="module")
def sn_runs(nn):
    """both lists in both modes, each run once; the references once"""
    lists = {"edges": edge_shapes(nn), "real": M.SN_SHAPES}
    runs = {}
    for name, shapes in lists.items():
        data = draw(shapes, 5 if name == "edges" else 6)
        for iterate in (True, False):
            sn, per, raw = run_sn(nn, shapes, data, iterate)
            r64 = [M.snorm_ref(W, u, v, iterate, gw) for W, u, v, gw in data]
            r32 = [M.snorm_torch(W, u, v, iterate, gw, torch.float32) for W, u, v, gw in data]
            runs[name, iterate] = dict(shapes=shapes, data=data, sn=sn, per=per, raw=raw, r64=r64, r32=r32)
    return runs


@pytest.mark.parametrize("iterate", [True, False])
@pytest.mark.parametrize("name", ["edges", "real"])
def test_spectral_norm_against_float64(nn, sn_runs, name, iterate):
    c = sn_runs[name, iterate]
    bad = []
    for i, (shape, got, a, b) in enumerate(zip(c["shapes"], c["per"], c["r64"], c["r32"])):
        tag = f"{name} it={int(iterate)} {shape}"
        for what, kind, j in (("w", "weight", 0), ("u", "vec", 1), ("v", "vec", 2), ("sigma", "vec", 3), ("gW", "weight", 4)):
            y, r64, r32 = got[j], a[j].reshape(got[j].shape), b[j].reshape(got[j].shape)
            assert torch.isfinite(y).all(), (tag, what)
            if what == "gW" and shape == (1, 1):
                # one element: gw / sigma and (gw W / sigma^2) u v cancel exactly in real arithmetic (|u| = |v| = 1, sigma = |W|),
                # so there is no reference size to be relative to; each term is accurate to 2^-24 of itself
                lim = 2.0 ** -23 * float((c["data"][i][3].double() / a[3]).abs())
                print(f"CG {tag} gW: |gW| {float(y.abs()):.3e} limit {lim:.3e}")
                assert float(y.abs()) <= lim, (tag, float(y.abs()), lim)
                continue
            if kind == "weight":
                y, r64, r32 = y[:, :, None], r64[:, :, None], r32[:, :, None]
            bad += R.check(f"{tag} {what}", kind, y, r64, r32)
    assert not bad, bad


@pytest.mark.parametrize("iterate", [True, False])
def test_two_calls_give_equal_bits_and_gaps_stay_zero(nn, sn_runs, iterate):
    c = sn_runs["edges", iterate]
    sn, per, raw = run_sn(nn, c["shapes"], c["data"], iterate)
    for a, b in zip(raw, c["raw"]):
        assert torch.equal(bits(a), bits(b)), "two calls differ"
    w, state, gW = (t.cpu() for t in raw)
    sizes = [r * k for r, k in c["shapes"]]
    assert sn.has_gaps and gap_mask(sn.off, sizes, sn.total).any()
    assert not w[gap_mask(sn.off, sizes, sn.total)].any() and not gW[gap_mask(sn.off, sizes, sn.total)].any()
    n = len(sizes)
    st_off = list(sn.u_off) + [sn.u_total + o for o in sn.v_off] + [sn.u_total + sn.v_total]
    st_sizes = [r for r, _ in c["shapes"]] + [k for _, k in c["shapes"]] + [n]
    gaps = gap_mask(st_off, st_sizes, sn.state_total)
    assert gaps.any() and not state[gaps].any()
    # outputs handed in: poisoned gaps are left alone, everything else is overwritten
    Wf = flat(sn, c["data"], 0, sn.off, sn.total)
    uf, vf = flat(sn, c["data"], 1, sn.u_off, sn.u_total), flat(sn, c["data"], 2, sn.v_off, sn.v_total)
    out, st = torch.full((sn.total,), 7.0, device=DEV), torch.full((sn.state_total,), 7.0, device=DEV)
    sn.forward(Wf, uf, vf, iterate, out=out, state=st)
    torch.cuda.synchronize()
    gm = gap_mask(sn.off, sizes, sn.total)
    assert bool((out.cpu()[gm] == 7.0).all()) and torch.equal(bits(out.cpu()[~gm]), bits(w[~gm]))
    assert bool((st.cpu()[gaps] == 7.0).all()) and torch.equal(bits(st.cpu()[~gaps]), bits(state[~gaps]))


@pytest.mark.parametrize("iterate", [True, False])
def test_a_tensor_does_not_depend_on_its_list_and_null_gradients_are_zeros(nn, sn_runs, iterate):
    c = sn_runs["edges", iterate]
    pick = [0, 2, 4, 5, 11, 17]  # some alone, in another order, with other neighbours
    for group in ([i] for i in pick[:3]), [pick[::-1]]:
        for idx in group:
            _, per, _ = run_sn(nn, [c["shapes"][i] for i in idx], [c["data"][i] for i in idx], iterate)
            for got, i in zip(per, idx):
                for a, b in zip(got, c["per"][i]):
                    assert torch.equal(bits(a), bits(b)), (idx, i)
    null = (1, 5, 9)
    _, per, _ = run_sn(nn, c["shapes"], c["data"], iterate, null=null)
    for i, (got, want) in enumerate(zip(per, c["per"])):
        if i in null:
            assert not got[4].any(), i
        else:
            assert torch.equal(bits(got[4]), bits(want[4])), i


def test_spectral_norm_refusals_by_name(nn):
    for shapes in ([], [(0, 3)], [(3, 0)], [(2, 2)] * 129, [(1 << 22, 1), (1, 1)], [(1, (1 << 26) + 1)], [(1 << 17, 1 << 15), (1, 1)]):
        with pytest.raises(nn.DisscError, match="dissc_snorm_create"):
            nn.SpectralNorm(shapes)
    sn = nn.SpectralNorm([(5, 7), (3, 4)])
    W, u, v = (torch.zeros(n, device=DEV) for n in (sn.total, sn.u_total, sn.v_total))
    with pytest.raises(nn.DisscError, match="SpectralNorm.forward"):
        sn.forward(W[:-4], u, v)
    with pytest.raises(nn.DisscError, match="SpectralNorm.forward"):
        sn.forward(W.double(), u, v)
    with pytest.raises(nn.DisscError, match="SpectralNorm.forward"):
        sn.forward(W, u.cpu(), v)
    with pytest.raises(nn.DisscError, match="dissc_snorm_forward"):
        sn.forward(W, u, v, out=W)  # an input as the output
    big = torch.zeros(sn.total + 4, device=DEV)
    with pytest.raises(nn.DisscError, match="dissc_snorm_forward"):
        sn.forward(big[1:1 + sn.total], u, v)  # not 16-byte aligned
    _, state = sn.forward(W + 1, u + 1, v + 1)
    with pytest.raises(nn.DisscError, match="SpectralNorm.backward"):
        sn.backward(W, state, [None])
    with pytest.raises(nn.DisscError, match="SpectralNorm.backward"):
        sn.backward(W, state, [torch.zeros(5, 6, device=DEV), None])
    g = torch.zeros(40, device=DEV)
    with pytest.raises(nn.DisscError, match="dissc_snorm_backward"):
        sn.backward(W, state, [g[1:36], None])  # a gradient that is not 16-byte aligned


# ---- 2. the module against float64 -------------------------------------------------------------------------------------------------
CASES = {"ragged": (3, 1030, [1030, 517, 130]), "full": (2, 1024, None)}


def _module(nn, sd):
    D = nn.MultiScaleDiscriminator().to(DEV)
    D.load_state_dict(sd)
    return D


def _buffers(D):
    return {k: v for k, v in D.state_dict().items() if k.startswith("discriminators.0.") and k.endswith(("weight_u", "weight_v"))}


@pytest.fixture(scope="module", params=list(CASES))
def msd(nn, request):
    """the checkpoint, the batch, the module's discriminator step (forward 1), generator step (forward 2) and a third forward, and
    the references of the same sequence in both dtypes"""
    B, T, L = CASES[request.param]
    sd = M.msd_state_dict(21)
    y, y_hat = M.wav_pair(22, B, T)
    D = _module(nn, sd)
    yd = y.to(DEV)
    out = D(yd, y_hat.to(DEV), L)
    loss_d, r_losses, g_losses = nn.discriminator_loss(out)
    loss_d.backward()
    torch.cuda.synchronize()
    dec_d = M.Decisions(out.fmaps)  # the references run on the branches the engine took (msd_cases.Decisions says why)
    d = dict(loss=loss_d.detach().cpu(), r=r_losses.detach().cpu(), g=g_losses.detach().cpu(), sigma=out.sigma.cpu(),
             grads={k: t.cpu().clone() for k, t in D.named_grads().items()}, buffers=_buffers(D))
    D.zero_grad()
    yh = y_hat.to(DEV).requires_grad_(True)
    out = D(yd, yh, L)
    fm, (gen, gen_losses) = nn.feature_loss(out), nn.generator_loss(out)
    (fm + gen).backward()
    torch.cuda.synchronize()
    dec_g = M.Decisions(out.fmaps)
    g = dict(fm=fm.detach().cpu(), gen=gen.detach().cpu(), gen_losses=gen_losses.detach().cpu(), grad=yh.grad.cpu(), sigma=out.sigma.cpu(),
             leaf_grads=[p.grad is not None for p in D.parameters()], buffers=_buffers(D))
    with torch.no_grad():
        third = D(yd, y_hat.to(DEV), L).sigma.cpu()
    ref_d = {dt: M.d_step_ref(sd, y, y_hat, L, dt, decisions=dec_d) for dt in (torch.float64, torch.float32)}
    ref_g = {dt: M.g_step_ref(sd, y, y_hat, L, dt, forwards_before=1, decisions=dec_g) for dt in (torch.float64, torch.float32)}
    # the engine's decisions are the float64 reference's own but for the elements float32 cannot resolve
    own = M.Decisions(ref_g[torch.float64][4].maps)
    differ = sum(int((a != b).sum()) for ra, rb in zip(own.masks, dec_g.masks) for a, b in zip(ra, rb))
    total = sum(a.numel() for ra in own.masks for a in ra)
    print(f"CG decisions of the G step that differ from float64's own: {differ} of {total}")
    assert differ <= 1e-5 * total
    seq = {dt: M.sigmas_after(sd, dt, 3) for dt in (torch.float64, torch.float32)}
    return dict(case=request.param, B=B, T=T, L=L, sd=sd, y=y, y_hat=y_hat, D=D, d=d, g=g, third=third, ref_d=ref_d, ref_g=ref_g, seq=seq)


def _kind(key, t):
    """(kind, tensor as the bars take it) of a checkpoint tensor"""
    return ("weight", t) if t.dim() == 3 and t.shape[1:] != (1, 1) else ("vec", t.reshape(-1))


def test_discriminator_step_against_float64(nn, msd):
    d = msd["d"]
    (m64, l64, r64, g64), (m32, l32, r32, g32) = msd["ref_d"][torch.float64], msd["ref_d"][torch.float32]
    bad = GL.check("D step loss", "vec", d["loss"].reshape(1), l64.reshape(1), l32.reshape(1))
    bad += GL.check("D step r_losses", "vec", d["r"], r64, r32)
    bad += GL.check("D step g_losses", "vec", d["g"], g64, g32)
    for i in range(3):  # per-scale values, each on its own
        bad += GL.check(f"D step r / g of scale {i}", "vec", torch.stack([d["r"][i], d["g"][i]]), torch.stack([r64[i], g64[i]]),
                        torch.stack([r32[i], g32[i]]), verbose=False)
    p64, p32 = dict(m64.named_parameters()), dict(m32.named_parameters())
    assert sorted(d["grads"]) == sorted(p64) and len(p64) == 8 * 2 + 16 * 3
    for k in sorted(d["grads"]):
        kind, got = _kind(k, d["grads"][k])
        bad += GL.check(f"D step grad {k}", kind, got, _kind(k, p64[k].grad)[1], _kind(k, p32[k].grad)[1], *_bars(msd["case"], "grad", k))
    assert not bad, bad


def test_generator_step_terms_against_float64(nn, msd):
    g, B, T, L = msd["g"], msd["B"], msd["T"], msd["L"]
    (fm64, gen64, gl64, gy64, _), (fm32, gen32, gl32, gy32, _) = msd["ref_g"][torch.float64], msd["ref_g"][torch.float32]
    bad = GL.check("G step feature_loss", "vec", g["fm"].reshape(1), fm64.reshape(1), fm32.reshape(1))
    bad += GL.check("G step generator_loss", "vec", g["gen"].reshape(1), gen64.reshape(1), gen32.reshape(1))
    bad += GL.check("G step gen_losses", "vec", g["gen_losses"], gl64, gl32)
    bad += GL.check("G step grad y_hat", "act", g["grad"], gy64, gy32)
    assert g["grad"].shape == (B, 1, T) and torch.isfinite(g["grad"]).all()
    for b, n in enumerate(L or [T] * B):
        assert not g["grad"][b, :, n:].any() and g["grad"][b, :, :n].any()
    assert all(g["leaf_grads"])  # param_grads=True: the reference's discarded gradients are there
    assert not bad, bad


def test_two_sigmas_per_forward_and_the_buffers_after_one_two_and_three(nn, msd):
    d, g, seq64, seq32 = msd["d"], msd["g"], msd["seq"][torch.float64], msd["seq"][torch.float32]
    bad = []
    for f, got in enumerate((d["sigma"], g["sigma"], msd["third"])):
        assert got.shape == (2, 8)
        # conv_post has ONE row: u = +-1 whatever v, so one iteration reaches its fixed point and its two sigmas agree
        assert bool((got[0, :7] != got[1, :7]).all()), ("the halves of one forward must see different sigmas", f, got)
        for h in range(2):
            bad += GL.check(f"forward {f + 1} half {h} sigma", "vec", got[h], seq64[f][0][h], seq32[f][0][h])
    for f, got in enumerate((d["buffers"], g["buffers"])):
        assert sorted(got) == sorted(seq64[f][1])
        for k in sorted(got):
            bad += GL.check(f"after forward {f + 1} {k}", "vec", got[k], seq64[f][1][k], seq32[f][1][k], verbose=k.endswith("convs.6.weight_v"))
    assert not bad, bad


def test_power_iteration_false_is_eval(nn, msd):
    D, B, L = msd["D"], msd["B"], msd["L"]
    before = _buffers(D)
    with torch.no_grad():
        out = D(msd["y"].to(DEV), msd["y_hat"].to(DEV), L, power_iteration=False)
        w = D.folded(0)
        halves = [nn.discriminator_s(wav.to(DEV), w, L) for wav in (msd["y"], msd["y_hat"])]
    assert torch.equal(bits(out.sigma[0]), bits(out.sigma[1]))
    after = _buffers(D)
    assert all(torch.equal(bits(before[k]), bits(after[k])) for k in before)
    for h, (score, fmaps, lens) in enumerate(halves):
        for j in range(8):
            assert torch.equal(bits(out.fmaps[0][j][h * B:(h + 1) * B]), bits(fmaps[j])), (h, j)
    m = M.torch_msd(D.state_dict(), torch.float64, train=False)
    with torch.no_grad():
        m(msd["y"].double(), msd["y_hat"].double(), L)
    assert not GL.check("eval sigma", "vec", out.sigma[0].cpu(), m.sigmas[0], m.sigmas[0].float())


# ---- 3. composition, bit for bit ---------------------------------------------------------------------------------------------------
def test_scale_0_halves_equal_discriminator_s_with_their_own_sigma(nn, msd):
    B, L = msd["B"], msd["L"]
    D = _module(nn, msd["sd"])
    yd, yh = msd["y"].to(DEV), msd["y_hat"].to(DEV)
    sn = D.sn
    with torch.no_grad():
        w1, s1 = sn.forward(D.w_orig.detach(), D.u, D.v, True)
        u1, v1, sg1 = sn.split(s1)
        w2, s2 = sn.forward(D.w_orig.detach(), u1, v1, True)
        out = D(yd, yh, L)
    assert torch.equal(bits(out.sigma[0]), bits(sg1)) and torch.equal(bits(out.sigma[1]), bits(sn.split(s2)[2]))
    named = D._named(*(p.detach() for p in D.parameters()))
    assert out.R == [B, B, B] and all(out.scores[i] is out.fmaps[i][7] and len(out.fmaps[i]) == len(out.lens[i]) == 8 for i in range(3))
    for h, (wav, wf) in enumerate(((yd, w1), (yh, w2))):
        w = {}
        for j, (name, shape, _) in enumerate(D.layers0):
            short = name.split(".", 2)[2]
            w[short + ".weight"] = wf[sn.off[j]:sn.off[j] + shape[0] * shape[1] * shape[2]].view(shape)
            w[short + ".bias"] = named[name + ".bias"]
        with torch.no_grad():
            score, fmaps, lens = nn.discriminator_s(wav, w, L)
        for j in range(8):
            got = out.fmaps[0][j][h * B:(h + 1) * B]
            assert got.shape == fmaps[j].shape and torch.equal(bits(got), bits(fmaps[j])), (h, j)
            assert torch.equal(out.lens[0][j][h * B:(h + 1) * B], lens[j]), (h, j)


@pytest.mark.parametrize("i", [1, 2])
def test_scales_1_and_2_equal_discriminator_s_on_each_pooled_input_alone(nn, msd, i):
    D, B, L = msd["D"], msd["B"], msd["L"]
    yd, yh = msd["y"].to(DEV), msd["y_hat"].to(DEV)
    with torch.no_grad():
        out = D(yd, yh, L)
        w = D.folded(i)
        for h, wav in enumerate((yd, yh)):
            ln = L
            for _ in range(i):
                wav, ln = nn.mean_pool(wav, ln)
            score, fmaps, lens = nn.discriminator_s(wav, w, ln)
            for j in range(8):
                got = out.fmaps[i][j][h * B:(h + 1) * B]
                assert got.shape == fmaps[j].shape and torch.equal(bits(got), bits(fmaps[j])), (i, h, j)
                assert torch.equal(out.lens[i][j][h * B:(h + 1) * B], lens[j]), (i, h, j)


# ---- 4. param_grads=False ----------------------------------------------------------------------------------------------------------
def test_param_grads_false_skips_the_leaves_advances_the_buffers_and_keeps_every_bit(nn, msd):
    L = msd["L"]
    res = []
    for pg in (True, False):
        D = _module(nn, msd["sd"])
        yh = msd["y_hat"].to(DEV).requires_grad_(True)
        out = D(msd["y"].to(DEV), yh, L, param_grads=pg)
        fm, (gen, gen_losses) = nn.feature_loss(out), nn.generator_loss(out)
        (fm + gen).backward()
        torch.cuda.synchronize()
        assert all((p.grad is not None) == pg for p in D.parameters())
        res.append((yh.grad, fm, gen, gen_losses, out.sigma, _buffers(D)))
    for a, b in zip(res[0][:5], res[1][:5]):
        assert torch.equal(bits(a), bits(b))
    start = {k: v for k, v in msd["sd"].items() if k in res[1][5]}
    for k, v in res[1][5].items():
        assert torch.equal(bits(v), bits(res[0][5][k])), k
        if not k.endswith("conv_post.weight_u"):  # one row: u = +-1 before and after
            assert not torch.equal(v, start[k]), ("the buffers did not advance", k)
    assert torch.equal(bits(res[1][5]["discriminators.0.convs.3.weight_u"]), bits(msd["d"]["buffers"]["discriminators.0.convs.3.weight_u"]))


# ---- 5. the checkpoint round trip --------------------------------------------------------------------------------------------------
# The bars are the project's 4 / 4, with the exceptions below by the rule of tests/test_gpu_mpd.py: K = 2 x the measured worst ratio,
# rounded up, never above k_cap(n), n = the products in one element's sum of that layer's weight (or bias) gradient: its valid
# output positions, both halves.  The ratio's denominator is float32 torch's own error, and the worst-row figure is a maximum over
# up to 1 024 rows of a quotient of two such errors: heavy-tailed.  For the stepped tensors the mechanism is the one described
# there: AdamW's first step hands the gradient's error dg on as  lr eps / (|g| + eps)^2 dg,  so a stepped tensor is compared in the
# summation error of its gradient on its few elements with the smallest |g|, in the engine and in torch's fp32 alike.
# (case, what, key) -> (whole, worst row); measured on an MI355X (profiles/msd_train.md), every other tensor inside 4 / 4:
#   full    grad     discriminators.0.convs.1.weight_orig  2.37 / 5.19  ->   4 / 11  (n = 2048, cap 32)
#   full    grad     discriminators.0.convs.4.weight_orig  1.60 / 4.33  ->   4 /  8  (n = 64, cap 8: twice the measured value would be 9)
#   ragged  stepped  discriminators.0.convs.4.weight_orig  2.14 / 5.15  ->   4 /  7  (n = 58, cap 7.6: ... 11)
#   full    stepped  discriminators.0.convs.1.weight_orig  5.88 / 6.06  ->  12 / 13  (n = 2048, cap 32)
#   full    stepped  discriminators.0.convs.2.weight_orig  4.42 / 5.28  ->   9 / 11  (n = 1024, cap 32)
#   full    stepped  discriminators.0.convs.4.weight_orig  2.84 / 7.11  ->   6 /  8  (n = 64, cap 8: ... 15)
#   full    stepped  discriminators.1.convs.3.bias         7.64         ->  11       (n = 132, cap 11.5: ... 16)
#   full    stepped  discriminators.2.convs.2.bias         9.30         ->  16       (n = 260, cap 16.1: ... 19)
EXCEPTIONS = {("full", "grad", "discriminators.0.convs.1.weight_orig"): (4.0, 11.0),
              ("full", "grad", "discriminators.0.convs.4.weight_orig"): (4.0, 8.0),
              ("ragged", "stepped", "discriminators.0.convs.4.weight_orig"): (4.0, 7.0),
              ("full", "stepped", "discriminators.0.convs.1.weight_orig"): (12.0, 13.0),
              ("full", "stepped", "discriminators.0.convs.2.weight_orig"): (9.0, 11.0),
              ("full", "stepped", "discriminators.0.convs.4.weight_orig"): (6.0, 8.0),
              ("full", "stepped", "discriminators.1.convs.3.bias"): (11.0, 4.0),
              ("full", "stepped", "discriminators.2.convs.2.bias"): (16.0, 4.0)}


def _bars(case, what, key):
    kw, kc = EXCEPTIONS.get((case, what, key), (GL.K_WHOLE, GL.K_CH))
    if (case, what, key) in EXCEPTIONS:
        B, T, L = CASES[case]
        _, i, rest = key.split(".", 2)
        j = 7 if rest.startswith("conv_post") else int(rest.split(".")[1])
        n = 2 * sum(M.map_lens(L, B, T)[int(i)][j])
        assert key.endswith(("weight_orig", "weight_v", "bias")) and max(kw, kc) <= GL.k_cap(n), (key, n)
    return kw, kc


def test_checkpoint_round_trip_through_one_optimiser_step(nn, msd):
    sd, y, y_hat, L = msd["sd"], msd["y"], msd["y_hat"], msd["L"]
    D = _module(nn, sd)
    assert len(D.parameters()) == 5 and all(p.is_leaf and p.requires_grad for p in D.parameters())
    before = D.state_dict()
    assert sorted(before) == sorted(sd) and all(torch.equal(before[k], sd[k]) for k in sd)
    opt = torch.optim.AdamW(D.parameters())
    loss_d, _, _ = nn.discriminator_loss(D(y.to(DEV), y_hat.to(DEV).detach(), L))
    loss_d.backward()
    opt.step()
    torch.cuda.synchronize()
    after = D.state_dict()
    M.TorchMSD().load_state_dict(after, strict=True)
    assert {k: tuple(v.shape) for k, v in after.items()} == M.expected_shapes()
    replay = {}
    for dt in (torch.float64, torch.float32):
        stepped = msd["ref_d"][dt][0]  # the shared reference step: its gradients stay as they are, its buffers have advanced
        m = M.torch_msd(sd, dt)
        for (k, q), (k2, r) in zip(m.named_parameters(), stepped.named_parameters()):
            assert k == k2
            q.grad = r.grad.clone()
        torch.optim.AdamW(m.parameters()).step()
        replay[dt] = {k: v.detach() for k, v in m.state_dict().items()}
        replay[dt].update(M.buffers(stepped))
    bad = []
    for k in sorted(after):
        if not k.endswith("conv_post.weight_u"):
            assert not torch.equal(after[k], sd[k]), ("the step left a tensor as it was", k)
        kind, got = _kind(k, after[k])
        bad += GL.check(f"stepped {k}", kind, got, _kind(k, replay[torch.float64][k])[1], _kind(k, replay[torch.float32][k])[1],
                        *_bars(msd["case"], "stepped", k))
    assert not bad, bad
    for broken in ({k: v for k, v in sd.items() if k != "discriminators.0.convs.2.weight_u"}, dict(sd, extra=torch.zeros(1)),
                   dict(sd, **{"discriminators.0.conv_post.weight_v": torch.zeros(1, 1024, 3)})):
        with pytest.raises(RuntimeError):
            nn.MultiScaleDiscriminator().to(DEV).load_state_dict(broken)


# ---- 6. one full alternation with both discriminators ------------------------------------------------------------------------------
def test_one_full_alternation_with_both_discriminators(nn):
    """both lines of the reference's loop (sr/train.py:157-190) once each at the small shapes of tests/test_gpu_mpd.py"""
    import dissc_amd
    h = GT.TINY_CONFIG
    G = nn.CodeGenerator(h).to(DEV)
    G.load_state_dict(synth.synth_generator_state_dict(h, seed=1))
    P = nn.MultiPeriodDiscriminator().to(DEV)
    P.load_state_dict(MP.mpd_state_dict(2))
    S = _module(nn, M.msd_state_dict(3))
    frames, lengths = 40, [40, 33]
    code, f0, spkr, _ = synth.synth_generator_inputs(2, frames, seed=3, n_spk=200, n_codes=h["num_embeddings"])
    ns = [G.hop * n for n in lengths]
    y = torch.from_numpy(0.5 * np.random.RandomState(4).uniform(-1, 1, (2, 1, G.hop * frames)).astype(np.float32)).to(DEV)
    ms = dissc_amd.MelSpectrogram(n_fft=64, num_mels=20, hop_size=16, win_size=64).to(DEV)
    params_d = P.parameters() + S.parameters()
    optim_g, optim_d = torch.optim.AdamW(G.parameters(), 2e-4, betas=(0.8, 0.99)), torch.optim.AdamW(params_d, 2e-4, betas=(0.8, 0.99))
    y_hat = G(code=torch.from_numpy(code), f0=torch.from_numpy(f0), spkr=torch.from_numpy(spkr), lengths=lengths)
    loss_p, loss_s = nn.discriminator_loss(P(y, y_hat.detach(), ns))[0], nn.discriminator_loss(S(y, y_hat.detach(), ns))[0]
    (loss_s + loss_p).backward()
    grads_d = [p.grad.clone() for p in params_d]
    optim_d.step()
    P.zero_grad(), S.zero_grad()
    out_p, out_s = P(y, y_hat, ns, param_grads=False), S(y, y_hat, ns, param_grads=False)
    loss_g = nn.feature_loss(out_s) + nn.feature_loss(out_p) + nn.generator_loss(out_s)[0] + nn.generator_loss(out_p)[0] + \
        45 * ms.l1_loss(y, y_hat, n_samples=ns)
    y_hat.retain_grad()
    loss_g.backward()
    assert all(p.grad is None for p in params_d)
    optim_g.step()
    torch.cuda.synchronize()
    tensors = [loss_p, loss_s, loss_g, y_hat, y_hat.grad, out_s.sigma] + grads_d + [p.grad for p in G.parameters()] + params_d + list(G.parameters())
    assert all(torch.isfinite(t).all() for t in tensors)
    for p, g in zip(params_d, grads_d):
        assert g.shape == p.shape and g.any()
    assert all(p.grad.any() for p in G.parameters())
    for b, n in enumerate(ns):  # exact zeros beyond the lengths: the waveform's gradient and every map of the scale side
        assert not y_hat.grad[b, :, n:].any() and y_hat.grad[b, :, :n].any()
    for i in range(3):
        for j, (m, ln) in enumerate(zip(out_s.fmaps[i], out_s.lens[i])):
            assert not m.detach().cpu()[GL.beyond_mask(m.shape, ln.cpu()[:2], 2)].any(), (i, j)


# ---- refusals: all before any launch ------------------------------------------------------------------------------------------------
def test_module_refusals(nn, msd):
    D, B, T = msd["D"], msd["B"], msd["T"]
    y = msd["y"].to(DEV)
    before = _buffers(D)
    with pytest.raises(nn.DisscError):
        D(y, y[:, :, :-4].contiguous())  # different shapes
    with pytest.raises(nn.DisscError):
        D(y, y[:1].contiguous())
    with pytest.raises(nn.DisscError):
        D(y, torch.zeros(B, 1, 2 * T, device=DEV)[:, :, ::2])  # not contiguous
    with pytest.raises(nn.DisscError):
        D(y, y.double())
    with pytest.raises(nn.DisscError):
        D(y, y.cpu())
    with pytest.raises(ValueError):
        D(y, y, [T + 1] * B)
    with pytest.raises(RuntimeError):
        nn.MultiScaleDiscriminator().parameters()
    with pytest.raises(nn.DisscError):
        D.folded(3)
    after = _buffers(D)
    assert all(torch.equal(before[k], after[k]) for k in before)  # a refused call runs no power iteration
