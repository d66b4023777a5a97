"""Times of what csrc/gen_train.hip adds, and of one whole training step of nn.CodeGenerator, at the trainer's shape: the shipped
VCTK config, 32 segments of 28 frames (8 960 samples).

    python tools/gen_train_bench.py [--batch 32] [--frames 28] [--launches 1000] [--steps 50] [--markdown]

Kernels (each through the C ABI or its thin Python wrapper, `--launches` calls between two device events after a warm-up), next
to the bytes they must move (every operand read once, every result written once) and the GB/s that implies:
  the multi-tensor weight norm, forward and backward over the generator's 97 tensors, against a loop of torch._weight_norm
  and its autograd backward over the same 97 tensors on the same GPU (this one has a bar: ours must not be slower);
  the embeddings' forward and gradient; the MRF mean (the five stages' rows, summed) and the tanh tail, both directions.
Step: forward + 45 x mel L1 + backward of nn.CodeGenerator against the same model in eager torch (torch._weight_norm -- what
weight_norm's hook evaluates --, F.embedding, F.conv1d / conv_transpose1d, F.l1_loss of torch log-mels) with the same weights,
`--steps` steps each after a warm-up; and the number of GPU kernels one step of each launches (torch.profiler's device
activities; null where the profiler gives none).  One JSON line per figure; --markdown adds the tables of profiles/gen_train.md.

    python tools/gen_train_bench.py --mpd [--batch 32] [--frames 28] [--launches 1000] [--steps 50] [--markdown]

times the period half of the GAN step instead (mpd_bench below; profiles/mpd_train.md): the fused loss launches of
csrc/gan_loss.hip on the 30 paired maps of nn.MultiPeriodDiscriminator, and the discriminator's and the generator's period-side
steps against the reference's MultiPeriodDiscriminator and loss functions in eager torch.

    python tools/gen_train_bench.py --msd [--batch 32] [--frames 28] [--launches 200] [--steps 20] [--markdown]

times the scale half (msd_bench below; profiles/msd_train.md): every dissc_snorm_* launch of csrc/spectral_norm.hip on the eight
matrices of discriminator 0 next to the bytes it must move, the two joined-map copies per map of scale 0, and the discriminator's
and the generator's scale-side steps against spectral_norm / weight_norm Conv1d modules in eager torch, in alternated runs.

    python tools/gen_train_bench.py --gan [--batch 32] [--frames 28] [--steps 20] [--blocks 3] [--markdown] [--precision split_bf16]

times what the GAN trainer adds (gan_bench below; profiles/gan_train.md): nn.AdamW against torch.optim.AdamW on the same leaves,
the gather launch against the host path, and GanTrainer.step against the same step in eager torch; with --precision split_bf16 the
whole-step blocks alternate GanTrainer.step with GanTrainer(precision="split_bf16").step instead (profiles/conv1d_split_bf16.md)."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
DEV = "cuda:0"
MIN_WINDOW_MS = 200.0  # --mpd: the least a timed window of loss launches covers


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def kernel_count(fn):
    """GPU kernels of one call of fn, or None where the profiler records no device activity"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception as e:  # a figure, not a requirement
        print(f"# kernel count unavailable: {e}", file=sys.stderr)
        return None


def row(name, ms, mbytes, extra=None):
    out = {"what": name, "us": round(1e3 * ms, 2), "MB": round(mbytes, 2), "GBps": round(mbytes / 1e3 / (ms * 1e-3), 1)}
    out.update(extra or {})
    print(json.dumps(out), flush=True)
    return out


def torch_mel(y, basis, window, n_fft=1024, hop=256):
    p = (n_fft - hop) // 2
    y = torch.nn.functional.pad(y[:, None], (p, p), mode="reflect")[:, 0]
    spec = torch.view_as_real(torch.stft(y, n_fft, hop_length=hop, win_length=n_fft, window=window, center=False, normalized=False,
                                         onesided=True, return_complex=True))
    return torch.log(torch.clamp(torch.matmul(basis, torch.sqrt(spec.pow(2).sum(-1) + 1e-9)), min=1e-5))


def mpd_bench(a):
    """--mpd: the period half of the GAN step at the trainer's shape (32 segments of 8 960 samples, the five periods): the two
    fused loss launches on the 30 paired maps next to the bytes they must move, the discriminator's step and the generator's
    period-side step (down to y_hat.grad, param_grads both ways) against eager torch on the same GPU with the same weights."""
    import gan_loss_ref as GL
    import mpd_cases as M
    from dissc_amd import nn
    from dissc_amd._lib import check, lib
    F = torch.nn.functional
    B, T = a.batch, 320 * a.frames
    sd = M.mpd_state_dict(0)
    D = nn.MultiPeriodDiscriminator().to(DEV)
    D.load_state_dict(sd)
    y, y_hat = (t.to(DEV) for t in M.wav_pair(1, B, T))
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    rows = []

    # ---- the loss launches, straight through the C ABI on the maps of one forward ----
    with torch.no_grad():
        out = D(y, y_hat)
    torch.cuda.synchronize()
    fm_maps = [m for fm in out.fmaps for m in fm]
    fm_lens = [t for ls in out.lens for t in ls]
    fm_R = [r for r in out.R for _ in range(6)]
    fm_slopes = [0.1 if j < 5 else 1.0 for _ in out.R for j in range(6)]
    sc_lens = [ls[5] for ls in out.lens]

    def launches(tag, op, maps, lens, R, slopes, halves_read):
        n = len(maps)
        args = nn._GanLossArgs([op] * n, maps, lens, R, slopes)
        nws = nn.ganloss_workspace_bytes(R, [m.shape[1] for m in maps], [m.shape[2] for m in maps])
        ws, res = torch.empty(nws, dtype=torch.uint8, device=DEV), torch.empty(1 + 2 * n, device=DEV)
        gmaps = [torch.empty_like(m) for m in maps]
        pg = (ctypes.c_void_p * n)(*[g.data_ptr() for g in gmaps])
        one = torch.ones((), device=DEV)
        fwd = lambda: check(lib.dissc_ganloss_forward(*args.head(), p(res), p(ws), nws, None))
        bwd = lambda: check(lib.dissc_ganloss_backward(*args.head(), p(one), None, pg, None))
        timed(fwd, 3), timed(bwd, 3)
        # valid elements of ONE half: C sum(lens[:R]); the forward reads halves_read halves, the backward reads them and writes both
        half = sum(m.shape[1] * int(l[:r].sum()) for m, l, r in zip(maps, lens, R))
        for what, fn, mb in ((f"{tag} forward, {n} maps, stage 1 + stage 2", fwd, 4e-6 * halves_read * half),
                             (f"{tag} backward, {n} maps, one launch", bwd, 4e-6 * (halves_read + 2) * half)):
            calls = a.launches
            ms = timed(fn, calls)
            if ms * calls < MIN_WINDOW_MS:  # a launch of a few us: time enough of them to fill the window
                calls = int(MIN_WINDOW_MS / ms) + 1
                ms = timed(fn, calls)
            rows.append(row(what, ms, mb, {"calls": calls, "window_ms": round(ms * calls, 1)}))

    launches("feature_loss (FM)", nn.FM, fm_maps, fm_lens, fm_R, fm_slopes, 2)
    launches("discriminator_loss (DISC)", nn.DISC, out.scores, sc_lens, out.R, [1.0] * 5, 2)
    launches("generator_loss (GEN)", nn.GEN, out.scores, sc_lens, out.R, [1.0] * 5, 1)
    del out, fm_maps

    # ---- eager torch: the reference's MultiPeriodDiscriminator (sr/models.py:228-286) in its batch form, the same weights ----
    P = {k: t.to(DEV).requires_grad_(True) for k, t in sd.items()}

    def torch_mpd(wav, grads):
        scores, fmaps = [], []
        for i, period in enumerate(M.PERIODS):
            x = wav
            if T % period:
                x = F.pad(x, (0, period - T % period), "reflect")
            x = x.view(x.shape[0], 1, -1, period)
            fm = []
            for j, (name, _, _, k) in enumerate(M.LAYERS):
                pre = f"discriminators.{i}.{name}"
                v, g, b = (P[pre + s] if grads else P[pre + s].detach() for s in (".weight_v", ".weight_g", ".bias"))
                x = F.conv2d(x, torch._weight_norm(v, g, 0), b, stride=(3, 1) if j < 4 else 1, padding=((k - 1) // 2, 0))
                if j < 5:
                    x = F.leaky_relu(x, 0.1)
                fm.append(x)
            scores.append(torch.flatten(x, 1, -1))
            fmaps.append(fm)
        return scores, fmaps

    def torch_d_step():
        for t in P.values():
            t.grad = None
        (s_r, _), (s_g, _) = torch_mpd(y, True), torch_mpd(y_hat, True)
        loss = GL.literal_discriminator_loss(s_r, s_g)[0]
        loss.backward()
        return loss

    def ours_d_step():
        D.zero_grad()
        loss = nn.discriminator_loss(D(y, y_hat))[0]
        loss.backward()
        return loss

    yh_o, yh_t = y_hat.clone().requires_grad_(True), y_hat.clone().requires_grad_(True)

    def torch_g_step(grads=True):
        yh_t.grad = None
        for t in P.values():
            t.grad = None
        (_, f_r), (s_g, f_g) = torch_mpd(y, grads), torch_mpd(yh_t, grads)
        loss = GL.literal_feature_loss(f_r, f_g) + GL.literal_generator_loss(s_g)[0]
        loss.backward()
        return loss

    def ours_g_step(param_grads=True):
        yh_o.grad = None
        D.zero_grad()
        out = D(y, yh_o, param_grads=param_grads)
        loss = nn.feature_loss(out) + nn.generator_loss(out)[0]
        loss.backward()
        return loss

    steps = []
    for tag, ours, ref in (("D step: D(y, y_hat.detach()), discriminator_loss, backward", ours_d_step, torch_d_step),
                           ("G step, param_grads=True: D(y, y_hat), feature_loss + generator_loss, backward to y_hat", ours_g_step, torch_g_step),
                           ("G step, param_grads=False (torch: detached parameters)", lambda: ours_g_step(False), lambda: torch_g_step(False))):
        lo, lt = float(ours().detach()), float(ref().detach())
        gd = None
        if ours is not ours_d_step:
            gd = float(f"{float((yh_o.grad - yh_t.grad).norm() / yh_t.grad.norm()):.2e}")
        timed(ours, 3), timed(ref, 3)
        ts = []
        for _ in range(2):  # the two alternate: other work shares the machine
            ts.append((timed(ours, a.steps), timed(ref, a.steps)))
        s = {"what": tag, "batch": B, "samples": T, "ours_ms": round(min(t[0] for t in ts), 3), "torch_ms": round(min(t[1] for t in ts), 3),
             "ours_ms_runs": [round(t[0], 3) for t in ts], "torch_ms_runs": [round(t[1], 3) for t in ts], "loss_ours": lo, "loss_torch": lt,
             "y_hat_grad_rel_diff": gd, "ours_kernels": kernel_count(ours), "torch_kernels": kernel_count(ref)}
        print(json.dumps(s), flush=True)
        steps.append(s)
    if a.markdown:
        print("\n| launch | calls timed | us | MB moved | GB/s |\n|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['what']} | {r['calls']} | {r['us']} | {r['MB']} | {r['GBps']} |")
        print("\n| step | ours ms | eager torch ms | ours / torch kernels |\n|---|---|---|---|")
        for s in steps:
            print(f"| {s['what']} | {s['ours_ms']} | {s['torch_ms']} | {s['ours_kernels']} / {s['torch_kernels']} |")
    return rows, steps


def kernel_times(fn, iters):
    """{kernel name: mean device us per call of fn} from torch.profiler, or {} where it records no device activity"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            t = getattr(e, "self_device_time_total", None)
            if t is None:
                t = getattr(e, "self_cuda_time_total", 0.0)
            if t and str(getattr(e, "device_type", "")).endswith("CUDA"):
                out[e.key] = t / iters
        return out
    except Exception as e:  # a figure, not a requirement
        print(f"# kernel times unavailable: {e}", file=sys.stderr)
        return {}


def msd_bench(a):
    """--msd: the scale half of the GAN step at the trainer's shape (32 segments of 8 960 samples): the spectral norm launches on
    discriminator 0's eight matrices next to the bytes they must move, the joined-map copies of scale 0, and both steps against
    eager torch's spectral_norm / weight_norm modules on the same GPU with the same weights, alternated."""
    import gan_loss_ref as GL
    import msd_cases as M
    from dissc_amd import nn
    from dissc_amd._lib import check, lib
    F = torch.nn.functional
    B, T = a.batch, 320 * a.frames
    sd = M.msd_state_dict(0)
    D = nn.MultiScaleDiscriminator().to(DEV)
    D.load_state_dict(sd)
    y, y_hat = (t.to(DEV) for t in M.wav_pair(1, B, T))
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    rows = []

    # ---- the spectral norm launches, straight through the C ABI ----
    sn = D.sn
    W, u, v = D.w_orig.detach(), D.u, D.v
    w_out, state = torch.zeros(sn.total, device=DEV), torch.zeros(sn.state_total, device=DEV)
    gws = [torch.randn(r, c, device=DEV) for r, c in sn.shapes]
    pw = (ctypes.c_void_p * sn.n)(*[t.data_ptr() for t in gws])
    gW = torch.zeros(sn.total, device=DEV)
    fwd1 = lambda: check(lib.dissc_snorm_forward(sn._h, p(W), p(u), p(v), 1, p(w_out), p(state), None))
    fwd0 = lambda: check(lib.dissc_snorm_forward(sn._h, p(W), p(u), p(v), 0, p(w_out), p(state), None))
    bwd = lambda: check(lib.dissc_snorm_backward(sn._h, p(W), p(state), pw, p(gW), None))
    for fn in (fwd1, fwd0, bwd):
        timed(fn, 3)
    mb = 4e-6 * sum(r * c for r, c in sn.shapes)  # one pass over the eight matrices
    part_mb = 8e-6 * sum(-(-r // nn.SNORM_CHUNK_ROWS) * c for r, c in sn.shapes)  # the W^T u partials, doubles
    small = 4e-6 * (sn.u_total + sn.v_total)
    rows.append(row("dissc_snorm_forward, iterate = 1: six launches", timed(fwd1, a.launches), 4 * mb + 2 * part_mb))
    rows.append(row("dissc_snorm_forward, iterate = 0: three launches", timed(fwd0, a.launches), 3 * mb))
    rows.append(row("dissc_snorm_backward: three launches", timed(bwd, a.launches), 4 * mb))
    must = {"snorm_wtu_kernel": mb + part_mb, "snorm_colsum_kernel": part_mb + 3 * small, "snorm_vnorm_kernel": 3 * small,
            "snorm_rowdot_kernel": mb, "snorm_usigma_kernel": 3 * small, "snorm_scale_kernel": 2 * mb, "snorm_gdot_kernel": 2 * mb,
            "snorm_coef_kernel": 0.03, "snorm_bwd_kernel": 2 * mb}
    per = kernel_times(lambda: (fwd1(), bwd()), 20)
    for name, need in must.items():
        us = [t for k, t in per.items() if name in k]
        if us:
            rows.append(row(f"{name} (one launch, profiler)", 1e-3 * us[0], need))

    # ---- the joined-map copies of scale 0: two device copies per map, eight maps ----
    with torch.no_grad():
        out = D(y, y_hat)
    halves = [(m[:B].clone(), m[B:].clone()) for m in out.fmaps[0]]
    join = lambda: [nn._JoinFn.apply(x, z) for x, z in halves]
    timed(join, 3)
    t_join = timed(join, max(20, a.launches // 10))
    rows.append(row("scale 0: the eight joined maps (16 device copies)", t_join, 2 * 4e-6 * sum(m.numel() for m in out.fmaps[0])))
    del out, halves

    # ---- eager torch: spectral_norm / weight_norm Conv1d modules in train() mode (reference sr/models.py:285-333), the same weights ----
    E = M.torch_msd(sd, torch.float32).to(DEV)
    pools = [torch.nn.AvgPool1d(4, 2, padding=2), torch.nn.AvgPool1d(4, 2, padding=2)]

    def disc(d, x):
        fmap = []
        for conv in d.convs:
            x = F.leaky_relu(conv(x), 0.1)
            fmap.append(x)
        x = d.conv_post(x)
        fmap.append(x)
        return torch.flatten(x, 1, -1), fmap

    def torch_msd(yr, yg):
        s_r, s_g, f_r, f_g = [], [], [], []
        for i, d in enumerate(E.discriminators):
            if i:
                yr, yg = pools[i - 1](yr), pools[i - 1](yg)
            a_, b_ = disc(d, yr), disc(d, yg)
            s_r.append(a_[0]), f_r.append(a_[1]), s_g.append(b_[0]), f_g.append(b_[1])
        return s_r, s_g, f_r, f_g

    def torch_d_step():
        E.zero_grad(set_to_none=True)
        s_r, s_g, _, _ = torch_msd(y, y_hat)
        loss = GL.literal_discriminator_loss(s_r, s_g)[0]
        loss.backward()
        return loss

    def ours_d_step():
        D.zero_grad()
        loss = nn.discriminator_loss(D(y, y_hat))[0]
        loss.backward()
        return loss

    yh_o, yh_t = y_hat.clone().requires_grad_(True), y_hat.clone().requires_grad_(True)

    def torch_g_step(grads=True):
        yh_t.grad = None
        E.zero_grad(set_to_none=True)
        for q in E.parameters():
            q.requires_grad_(grads)
        _, s_g, f_r, f_g = torch_msd(y, yh_t)
        loss = GL.literal_feature_loss(f_r, f_g) + GL.literal_generator_loss(s_g)[0]
        loss.backward()
        for q in E.parameters():
            q.requires_grad_(True)
        return loss

    def ours_g_step(param_grads=True):
        yh_o.grad = None
        D.zero_grad()
        out = D(y, yh_o, param_grads=param_grads)
        loss = nn.feature_loss(out) + nn.generator_loss(out)[0]
        loss.backward()
        return loss

    steps = []
    for tag, ours, ref in (("D step: D(y, y_hat.detach()), discriminator_loss, backward", ours_d_step, torch_d_step),
                           ("G step, param_grads=True: D(y, y_hat), feature_loss + generator_loss, backward to y_hat", ours_g_step, torch_g_step),
                           ("G step, param_grads=False (torch: parameters without requires_grad)", lambda: ours_g_step(False), lambda: torch_g_step(False))):
        # both sides advance their buffers at every call: reload them so that the two losses are of one state
        D.load_state_dict(sd), E.load_state_dict(sd)
        lo, lt = float(ours().detach()), float(ref().detach())
        gd = None
        if ours is not ours_d_step:
            gd = float(f"{float((yh_o.grad - yh_t.grad).norm() / yh_t.grad.norm()):.2e}")
        timed(ours, 2), timed(ref, 2)
        ts = []
        for _ in range(3):  # the two alternate: other work shares the machine
            ts.append((timed(ours, a.steps), timed(ref, a.steps)))
        s = {"what": tag, "batch": B, "samples": T, "ours_ms": round(min(t[0] for t in ts), 3), "torch_ms": round(min(t[1] for t in ts), 3),
             "ours_ms_runs": [round(t[0], 3) for t in ts], "torch_ms_runs": [round(t[1], 3) for t in ts], "loss_ours": lo, "loss_torch": lt,
             "y_hat_grad_rel_diff": gd, "join_ms": round(t_join, 3), "join_share_of_ours": round(t_join / min(t[0] for t in ts), 4),
             "ours_kernels": kernel_count(ours), "torch_kernels": kernel_count(ref)}
        print(json.dumps(s), flush=True)
        steps.append(s)
    if a.markdown:
        print("\n| launch | us | MB moved | GB/s |\n|---|---|---|---|")
        for r in rows:
            print(f"| {r['what']} | {r['us']} | {r['MB']} | {r['GBps']} |")
        print("\n| step | ours ms (runs) | eager torch ms (runs) | joins ms (share) | ours / torch kernels |\n|---|---|---|---|---|")
        for s in steps:
            print(f"| {s['what']} | {s['ours_ms']} {s['ours_ms_runs']} | {s['torch_ms']} {s['torch_ms_runs']} | {s['join_ms']} "
                  f"({100 * s['join_share_of_ours']:.1f} %) | {s['ours_kernels']} / {s['torch_kernels']} |")
    return rows, steps


def gan_bench(a):
    """--gan: what the GAN trainer adds, at 32 x 8 960 samples with the shipped VCTK config's model (profiles/gan_train.md):
    nn.AdamW.step() on optim_d's and optim_g's leaves against torch.optim.AdamW (default, foreach=True, fused=True) on copies of
    the same leaves with the same grads, in alternating blocks; the gather launch against the host path that builds the same
    batch and uploads it; GanTrainer.step against the same lines composed from eager torch modules and torch.optim.AdamW, from the same
    weights on the same batch, in alternating blocks."""
    import time

    import numpy as np
    import synthdata as synth
    from dissc_amd import gan_train, nn
    h = dict(synth.VCTK_CONFIG, learning_rate=2e-4, adam_b1=0.8, adam_b2=0.99, lr_decay=0.999, seed=1234, batch_size=a.batch,
             segment_size=320 * a.frames, code_hop_size=320)
    for k, v in dict(sampling_rate=16000, n_fft=1024, num_mels=80, hop_size=256, win_size=1024, fmin=0, fmax=8000, fmax_for_loss=None).items():
        h.setdefault(k, v)
    trainer = gan_train.GanTrainer(h, DEV).init(seed=0)
    rows = []

    # ---- 1. the optimiser: alternating blocks, every block shown ----
    gen = torch.Generator(device=DEV).manual_seed(0)
    for name, leaves in (("optim_d", trainer.msd.parameters() + trainer.mpd.parameters()), ("optim_g", trainer.generator.parameters())):
        n = sum(p.numel() for p in leaves)
        grads = [torch.randn(p.shape, device=DEV, generator=gen) for p in leaves]
        kw = dict(lr=2e-4, betas=(0.8, 0.99))

        def make(ctor):
            ps = [p.detach().clone().requires_grad_(True) for p in leaves]
            for q, g in zip(ps, grads):
                q.grad = g
            return ctor(ps).step
        variants = [("nn.AdamW", make(lambda ps: nn.AdamW(ps, **kw))), ("torch default", make(lambda ps: torch.optim.AdamW(ps, **kw))),
                    ("torch foreach=True", make(lambda ps: torch.optim.AdamW(ps, foreach=True, **kw))),
                    ("torch fused=True", make(lambda ps: torch.optim.AdamW(ps, fused=True, **kw)))]
        for _, fn in variants:
            timed(fn, 5)
        blocks = {v: [] for v, _ in variants}
        for _ in range(a.blocks):
            for v, fn in variants:
                blocks[v].append(timed(fn, a.steps))
        for v, fn in variants:
            ms = sorted(blocks[v])[len(blocks[v]) // 2]
            rows.append(row(f"{name} ({n / 1e6:.1f} M floats, {len(leaves)} leaves): {v}", ms, 28e-6 * n,
                            {"blocks_us": [round(1e3 * x, 1) for x in blocks[v]], "kernels": kernel_count(fn)}))
        del variants, grads
        torch.cuda.empty_cache()

    # ---- 2. the batch: one gather launch against crops on the host and four uploads ----
    rs = np.random.RandomState(0)
    items = []
    for u in range(4 * a.batch):
        T = int(rs.randint(a.frames // 2, 12 * a.frames))
        items.append(dict(name=f"u{u}", gt=rs.uniform(-1, 1, 320 * T).astype(np.float32), code=rs.randint(0, 100, T).astype(np.int64),
                          f0=rs.uniform(-2, 2, T).astype(np.float32), spkr=int(rs.randint(0, 200))))
    sampler = gan_train.SegmentSampler(h, items, seed=0, device=DEV)
    tables = [sampler.draw(i % len(sampler)) for i in range(64)]

    def ours(i):
        return sampler.gather(tables[i % 64])

    def host(i):
        crops = [gan_train.crop_host(items[u], s, 320, h["segment_size"]) for u, s in tables[i % 64]]
        return {"y": torch.from_numpy(np.stack([c[0] for c in crops])[:, None]).to(DEV), "code": torch.from_numpy(np.stack([c[1] for c in crops])).to(DEV),
                "f0": torch.from_numpy(np.stack([c[2] for c in crops])[:, None]).to(DEV),
                "spkr": torch.from_numpy(np.array([[items[u]["spkr"]] for u, _ in tables[i % 64]], np.int64)).to(DEV)}
    assert all(torch.equal(x, y) for x, y in zip(ours(0).values(), host(0).values()))

    def wall(fn, iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(iters):
            fn(i)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / iters
    mb = 1e-6 * a.batch * (4 * h["segment_size"] * 2 + a.frames * (4 + 8 + 4 + 4))
    wall(ours, 20), wall(host, 20)
    blocks = {"gather launch (host table by value)": [], "host crops + four uploads": []}
    for _ in range(a.blocks):
        blocks["gather launch (host table by value)"].append(wall(ours, 200))
        blocks["host crops + four uploads"].append(wall(host, 200))
    for what, b in blocks.items():
        rows.append(row(f"batch {a.batch} x {h['segment_size']}: {what}, wall per batch", sorted(b)[len(b) // 2], mb,
                        {"blocks_us": [round(1e3 * x, 1) for x in b]}))
    rows.append(row("gather, back-to-back calls between two device events", timed(lambda: ours(0), 200), mb))

    # ---- 3. the whole alternation: GanTrainer.step against the same lines in eager torch (the generator of main() below, the
    # period side of mpd_bench, the scale side of msd_bench, torch.optim.AdamW), from the same weights on the same batch ----
    import gan_loss_ref as GL
    import gen_train_ref as GT
    import mpd_cases as MP
    import msd_cases as MS
    import dissc_amd
    from oracle import generator_ref as G
    F = torch.nn.functional
    batch = sampler.batch(0)
    y, T = batch["y"], h["segment_size"]
    PG = {k: t.to(DEV).requires_grad_(True) for k, t in trainer.generator.state_dict().items()}
    PP = {k: t.to(DEV).requires_grad_(True) for k, t in trainer.mpd.state_dict().items()}
    E = MS.torch_msd(trainer.msd.state_dict(), torch.float32).to(DEV)  # spectral_norm / weight_norm Conv1d modules, train() mode
    pools = [torch.nn.AvgPool1d(4, 2, padding=2), torch.nn.AvgPool1d(4, 2, padding=2)]
    kw = dict(lr=float(h["learning_rate"]), betas=(h["adam_b1"], h["adam_b2"]))
    eg, ed = torch.optim.AdamW(list(PG.values()), **kw), torch.optim.AdamW(list(E.parameters()) + list(PP.values()), **kw)
    basis = torch.from_numpy(dissc_amd.mel.mel_filterbank(16000, 1024, 80)).float().to(DEV)
    window = torch.hann_window(1024, device=DEV)
    y_mel = torch_mel(y[:, 0], basis, window)  # the reference's loader hands the target's mel over with the batch

    def eager_mpd(wav, grads):
        scores, fmaps = [], []
        for i, period in enumerate(MP.PERIODS):
            x = wav
            if T % period:
                x = F.pad(x, (0, period - T % period), "reflect")
            x = x.view(x.shape[0], 1, -1, period)
            fm = []
            for j, (name, _, _, k) in enumerate(MP.LAYERS):
                pre = f"discriminators.{i}.{name}"
                v, g, bb = (PP[pre + sfx] if grads else PP[pre + sfx].detach() for sfx in (".weight_v", ".weight_g", ".bias"))
                x = F.conv2d(x, torch._weight_norm(v, g, 0), bb, stride=(3, 1) if j < 4 else 1, padding=((k - 1) // 2, 0))
                if j < 5:
                    x = F.leaky_relu(x, 0.1)
                fm.append(x)
            scores.append(torch.flatten(x, 1, -1))
            fmaps.append(fm)
        return scores, fmaps

    def eager_disc_s(d, x):
        fmap = []
        for conv in d.convs:
            x = F.leaky_relu(conv(x), 0.1)
            fmap.append(x)
        x = d.conv_post(x)
        fmap.append(x)
        return torch.flatten(x, 1, -1), fmap

    def eager_msd(yr, yg):
        s_r, s_g, f_r, f_g = [], [], [], []
        for i, d in enumerate(E.discriminators):
            if i:
                yr, yg = pools[i - 1](yr), pools[i - 1](yg)
            a_, b_ = eager_disc_s(d, yr), eager_disc_s(d, yg)
            s_r.append(a_[0]), f_r.append(a_[1]), s_g.append(b_[0]), f_g.append(b_[1])
        return s_r, s_g, f_r, f_g

    def eager_step(d_grads_in_g_step):
        """the reference's lines (sr/train.py:142-191); d_grads_in_g_step True is the reference as written (the discriminators'
        parameters keep requires_grad in the generator's half, their gradients are computed and dropped), False detaches them
        there, which is what GanTrainer's param_grads=False does"""
        w = {}
        for k, t in PG.items():
            if k.endswith(".weight_g"):
                w[k[:-2]] = torch._weight_norm(PG[k[:-2] + "_v"], t, 0)
            elif not k.endswith(".weight_v"):
                w[k] = t
        y_hat = GT._forward(w, h, G.embed_concat(w, batch["code"], batch["f0"], batch["spkr"]), None, None)
        ed.zero_grad()
        yd = y_hat.detach()
        loss_f = GL.literal_discriminator_loss(eager_mpd(y, True)[0], eager_mpd(yd, True)[0])[0]
        s_r, s_g, _, _ = eager_msd(y, yd)
        loss_d = GL.literal_discriminator_loss(s_r, s_g)[0] + loss_f
        loss_d.backward()
        ed.step()
        eg.zero_grad()
        loss_mel = F.l1_loss(y_mel, torch_mel(y_hat[:, 0], basis, window)) * 45
        for q in E.parameters():
            q.requires_grad_(d_grads_in_g_step)
        (_, ff_r), (sf_g, ff_g) = eager_mpd(y, d_grads_in_g_step), eager_mpd(y_hat, d_grads_in_g_step)
        _, ss_g, fs_r, fs_g = eager_msd(y, y_hat)
        loss_g = GL.literal_generator_loss(ss_g)[0] + GL.literal_generator_loss(sf_g)[0] + GL.literal_feature_loss(fs_r, fs_g) + \
            GL.literal_feature_loss(ff_r, ff_g) + loss_mel
        loss_g.backward()
        for q in E.parameters():
            q.requires_grad_(True)
        eg.step()
        return loss_d.detach(), loss_g.detach()

    # the first step of each from one state: the same losses
    first = trainer.step(batch)
    e_d, e_g = eager_step(False)
    same = {"what": "first step from the same weights", "ours_loss_disc_all": float(first["loss_disc_all"]), "eager_loss_disc_all": float(e_d),
            "ours_loss_gen_all": float(first["loss_gen_all"]), "eager_loss_gen_all": float(e_g)}
    print(json.dumps(same), flush=True)
    variants = [("GanTrainer.step", lambda i=0: trainer.step(batch)),
                ("eager torch, discriminators detached in the generator's half", lambda i=0: eager_step(False)),
                ("eager torch, the reference as written (discriminator gradients computed in both halves)", lambda i=0: eager_step(True))]
    if a.precision == "split_bf16":  # the split step against the fp32 step of this session, by turns, from the same weights
        split = gan_train.GanTrainer(h, DEV, precision="split_bf16").init(seed=0)
        s_first = split.step(batch)
        print(json.dumps({"what": "first step from the same weights, split_bf16", **{k: float(v) for k, v in s_first.items()}}), flush=True)
        variants = [variants[0], ('GanTrainer(precision="split_bf16").step', lambda i=0: split.step(batch))]
    for _, fn in variants:
        wall(fn, 3)
    blocks = {v: [] for v, _ in variants}
    for _ in range(a.blocks):
        for v, fn in variants:
            blocks[v].append(wall(fn, a.steps))
    for v, fn in variants:
        rows.append(row(f"whole alternation, wall per step: {v}", sorted(blocks[v])[len(blocks[v]) // 2], 0.0,
                        {"blocks_ms": [round(x, 2) for x in blocks[v]], "kernels": kernel_count(fn)}))
    opt = lambda i=0: (trainer.optim_d.step(), trainer.optim_g.step())
    rows.append(row("  of GanTrainer.step: optim_d.step() + optim_g.step()", timed(opt, a.steps), 28e-6 * sum(p.numel() for o in (trainer.optim_d, trainer.optim_g) for p in o.params)))
    if a.markdown:
        print("\n| what | us | MB | GB/s | blocks | kernels |\n|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['what']} | {r['us']} | {r['MB']} | {r['GBps']} | {r.get('blocks_us', r.get('blocks_ms', ''))} | {r.get('kernels', '')} |")
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=28)
    ap.add_argument("--launches", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--markdown", action="store_true")
    ap.add_argument("--mpd", action="store_true", help="time the period half of the GAN step (nn.MultiPeriodDiscriminator and the losses)")
    ap.add_argument("--msd", action="store_true", help="time the scale half of the GAN step (nn.SpectralNorm, nn.MultiScaleDiscriminator)")
    ap.add_argument("--gan", action="store_true", help="time what the GAN trainer adds: nn.AdamW, the segment gather, GanTrainer.step")
    ap.add_argument("--blocks", type=int, default=3, help="--gan: alternating blocks per variant")
    ap.add_argument("--precision", default="fp32", choices=("fp32", "split_bf16"),
                    help="--gan: split_bf16 times GanTrainer(precision=\"split_bf16\").step against the fp32 step in alternating blocks")
    a = ap.parse_args(argv)
    import __graft_entry__ as ge
    ge.build()
    if a.mpd:
        return mpd_bench(a)
    if a.msd:
        return msd_bench(a)
    if a.gan:
        return gan_bench(a)
    import dissc_amd
    import gen_train_ref as GT
    import synthdata as synth
    from dissc_amd import nn
    from dissc_amd._lib import check, lib
    from oracle import generator_ref as G
    F = torch.nn.functional
    h = synth.VCTK_CONFIG
    B, T = a.batch, a.frames
    sd = synth.synth_generator_state_dict(h, seed=0)
    gen = nn.CodeGenerator(h).to(DEV)
    gen.load_state_dict(sd)
    wn = gen.wn
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    rows = []

    # ---- weight norm over the 97 tensors ----
    v_flat, g_flat, b_flat = gen.v_flat.detach(), gen.g_flat.detach(), gen.bias_flat.detach()
    gws = [torch.randn(r, c, device=DEV) for r, c in wn.shapes]
    gbs = [torch.randn(n, device=DEV) for n in wn.bias_sizes]
    buf = torch.empty(wn.total + wn.bias_total, device=DEV)
    gv = torch.empty(wn.total, device=DEV)
    # straight through the C ABI with the pointer arrays built once: the Python wrappers check ~200 tensors per call, which at
    # these times would be what is measured
    inv, gg, gbf = torch.empty(wn.total_rows, device=DEV), torch.empty(wn.total_rows, device=DEV), torch.zeros(wn.bias_total, device=DEV)
    pw = (ctypes.c_void_p * wn.n)(*[t.data_ptr() for t in gws])
    pb = (ctypes.c_void_p * wn.n)(*[t.data_ptr() for t in gbs])
    bias_out = ctypes.c_void_p(buf.data_ptr() + 4 * wn.total)
    fwd = lambda: check(lib.dissc_wnorm_forward(wn._h, p(v_flat), p(g_flat), p(buf), p(inv), p(b_flat), bias_out, wn.bias_total, None))
    bwd = lambda: check(lib.dissc_wnorm_backward(wn._h, p(v_flat), p(g_flat), pw, p(gv), p(gg), pb, wn._bias_n, p(gbf), None))
    tv = [t.to(DEV).requires_grad_(True) for k, t in sd.items() if k.endswith(".weight_v")]
    tg = [t.to(DEV).requires_grad_(True) for k, t in sd.items() if k.endswith(".weight_g")]
    tgw = [w.view(v.shape) for w, v in zip(gws, tv)]
    assert [tuple(t.shape) for t in tv] == [s for _, s, _ in gen.layers]

    def torch_fwd():
        return [torch._weight_norm(v, g, 0) for v, g in zip(tv, tg)]

    def torch_both():
        torch.autograd.grad(torch_fwd(), tv + tg, tgw)

    for fn in (fwd, bwd, torch_fwd, torch_both):
        timed(fn, 3)
    mb = 4e-6 * wn.total
    n_t = max(20, a.launches // 10)
    t_f, t_b = timed(fwd, a.launches), timed(bwd, a.launches)
    t_tf, t_tb = timed(torch_fwd, n_t), timed(torch_both, n_t)
    rows.append(row("wnorm forward, 97 tensors, one launch", t_f, 2 * mb))
    rows.append(row("wnorm backward, 97 tensors, one launch", t_b, 3 * mb))
    rows.append(row("torch._weight_norm loop, forward", t_tf, 2 * mb))
    rows.append(row("torch._weight_norm loop, forward + autograd backward", t_tb, 5 * mb))
    verdict = {"what": "wnorm bar: forward + backward not slower than the torch loop", "ours_us": round(1e3 * (t_f + t_b), 1),
               "torch_us": round(1e3 * t_tb, 1), "holds": bool(t_f + t_b <= t_tb)}
    print(json.dumps(verdict), flush=True)

    # ---- embeddings ----
    code, f0, spkr, _ = synth.synth_generator_inputs(B, T, seed=1, n_spk=200)
    code_d, f0_d, spkr_d = torch.from_numpy(code).to(DEV), torch.from_numpy(f0).to(DEV).reshape(B, T).contiguous(), \
        torch.from_numpy(spkr).to(DEV).reshape(-1).contiguous()
    E, C, ld = 128, 257, (T + 3) // 4 * 4
    lens = torch.full((B,), T, dtype=torch.int32, device=DEV)
    x, gx = torch.zeros(B, C, ld, device=DEV), torch.randn(B, C, ld, device=DEV)
    gd, gs = torch.empty(100, E, device=DEV), torch.empty(200, E, device=DEV)
    dw, sw = gen.dict_weight.detach(), gen.spkr_weight.detach()
    e_f = lambda: check(lib.dissc_embed_concat_fwd(p(code_d), p(f0_d), p(spkr_d), p(dw), p(sw), p(lens), B, T, E, 100, 200, p(x), ld, None))
    e_b = lambda: check(lib.dissc_embed_concat_bwd(p(gx), p(code_d), 1, p(spkr_d), p(lens), B, T, E, 100, 200, ld, p(gd), p(gs), None))
    timed(e_f, 3), timed(e_b, 3)
    act = 4e-6 * B * C * T
    rows.append(row("embed_concat forward", timed(e_f, a.launches), act + 4e-6 * (B * T * 2 + 300 * E)))
    rows.append(row("embed_concat gradient (dense, 300 table rows)", timed(e_b, a.launches), act + 4e-6 * 300 * E))

    # ---- MRF mean (five stages) and tanh ----
    t_mf = t_mb = mrf_mb = 0.0
    L, ch = T, 512
    for u in h["upsample_rates"]:
        L, ch = L * u, ch // 2
        rs3 = [torch.randn(B, ch, L, device=DEV) for _ in range(3)]
        y, ln = torch.empty(B, ch, L, device=DEV), torch.full((B,), L, dtype=torch.int32, device=DEV)
        ptrs = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in rs3])
        m_f = lambda: check(lib.dissc_mrf_mean_fwd(ptrs, 3, p(y), p(ln), B, ch, L, L, None))
        m_b = lambda: check(lib.dissc_mrf_mean_bwd(p(rs3[0]), 3, p(y), p(ln), B, ch, L, L, None))
        timed(m_f, 3), timed(m_b, 3)
        t_mf += timed(m_f, a.launches)
        t_mb += timed(m_b, a.launches)
        mrf_mb += 4e-6 * B * ch * L
    rows.append(row("MRF mean forward, five stages (nk = 3)", t_mf, 4 * mrf_mb))
    rows.append(row("MRF mean backward, five stages", t_mb, 2 * mrf_mb))
    xw, yw, lw = torch.randn(B, 1, L, device=DEV), torch.empty(B, 1, L, device=DEV), torch.full((B,), L, dtype=torch.int32, device=DEV)
    t_f_ = lambda: check(lib.dissc_tanh_fwd(p(xw), p(yw), p(lw), B, 1, L, L, L, None))
    gxw = torch.empty_like(xw)
    t_b_ = lambda: check(lib.dissc_tanh_bwd(p(yw), p(xw), p(gxw), p(lw), B, 1, L, L, L, None))
    timed(t_f_, 3), timed(t_b_, 3)
    rows.append(row("tanh forward, [32, 1, 8960]", timed(t_f_, a.launches), 2 * 4e-6 * B * L))
    rows.append(row("tanh backward", timed(t_b_, a.launches), 3 * 4e-6 * B * L))

    # ---- one step: forward + 45 x mel L1 + backward, ours and eager torch ----
    ms = dissc_amd.MelSpectrogram().to(DEV)
    target = (0.3 * torch.randn(B, 320 * T)).to(DEV)
    code_t, f0_t, spkr_t = torch.from_numpy(code), torch.from_numpy(f0), torch.from_numpy(spkr)

    def ours_step():
        gen.zero_grad()
        (45 * ms.l1_loss(target, gen(code=code_t, f0=f0_t, spkr=spkr_t))).backward()

    P = {k: t.to(DEV).requires_grad_(True) for k, t in sd.items()}
    basis = torch.from_numpy(dissc_amd.mel.mel_filterbank(16000, 1024, 80)).float().to(DEV)
    window = torch.hann_window(1024, device=DEV)
    target_mel = torch_mel(target, basis, window)
    cd, fd, sdv = code_t.to(DEV), f0_t.to(DEV), spkr_t.to(DEV)

    def torch_step():
        for t in P.values():
            t.grad = None
        w = {}
        for k, t in P.items():
            if k.endswith(".weight_g"):
                w[k[:-2]] = torch._weight_norm(P[k[:-2] + "_v"], t, 0)
            elif not k.endswith(".weight_v"):
                w[k] = t
        wav = GT._forward(w, h, G.embed_concat(w, cd, fd, sdv), None, None)
        (45 * F.l1_loss(target_mel, torch_mel(wav[:, 0], basis, window))).backward()
        return wav

    ours_step(), torch_step()
    rel = float((gen(code=code_t, f0=f0_t, spkr=spkr_t).detach() - torch_step().detach()).norm() / torch_step().detach().norm())
    timed(ours_step, 3), timed(torch_step, 3)
    t_o, t_t = timed(ours_step, a.steps), timed(torch_step, a.steps)
    step = {"what": "step: forward + 45 x mel L1 + backward", "batch": B, "frames": T, "ours_ms": round(t_o, 3), "torch_ms": round(t_t, 3),
            "wav_rel_diff": float(f"{rel:.2e}"), "ours_kernels": kernel_count(ours_step), "torch_kernels": kernel_count(torch_step)}
    print(json.dumps(step), flush=True)
    if a.markdown:
        print("\n| kernel | us | MB moved | GB/s |\n|---|---|---|---|")
        for r in rows:
            print(f"| {r['what']} | {r['us']} | {r['MB']} | {r['GBps']} |")
        print(f"\nweight norm, forward + backward: ours {verdict['ours_us']} us, torch loop {verdict['torch_us']} us "
              f"({'holds' if verdict['holds'] else 'MISSED'})")
        print(f"step at B = {B}, T = {T}: ours {step['ours_ms']} ms ({step['ours_kernels']} kernels), eager torch {step['torch_ms']} ms "
              f"({step['torch_kernels']} kernels); wav relative difference {step['wav_rel_diff']}")
    return rows, verdict, step


if __name__ == "__main__":
    main()
