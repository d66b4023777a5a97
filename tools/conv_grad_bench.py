"""Time of the differentiable Conv1d layer (dissc_amd.nn, csrc/conv_grad.hip) on every distinct stride-1 layer shape of the
generator at the trainer's batch, 32 segments of 28 frames (8 960 samples), against torch-ROCm's own conv1d autograd on
the same tensors in the same process:

    python tools/conv_grad_bench.py [--batch 32] [--frames 28] [--blocks 5] [--iters 10] [--only CIN,COUT,K] [--markdown]

Per shape: ms of the forward, the data gradient (conv^T + the leaky-ReLU mask) and the weight + bias gradient (partials +
their reduction), each through the C ABI alone, and torch's forward (leaky_relu + conv1d), and its data / weight + bias
gradients alone (aten.convolution_backward with one output mask each -- what conv1d's autograd node runs; torch's data
gradient leaves the mask to the leaky ReLU's own node, so its figure is a little short of ours).  Medians of alternating
blocks (ours, torch, ours, ...), each block `iters` calls between two device events.  TFLOP/s are of the EXECUTED matrix
work: padded rows / channel chunks for the direct convs, padded 32 x 32 tiles x tap groups for the weight gradient.  One
JSON line per shape; --markdown adds the table of profiles/conv_grad.md.

    python tools/conv_grad_bench.py --precision split_bf16 [--mpd] [--markdown]

adds, in the same alternating blocks, the three directions (and the repack) of the split-bf16 handle of each shape
(nn.conv1d(..., precision="split_bf16"), csrc/conv_grad_bf3.hip) next to the fp32 handle's and torch's, with every block's figure
kept in the JSON line ("*_ms_blocks"), the directions nn.conv1d_precision reports as split, and the split results' distance to
torch; --mpd adds 1024 -> 1024, k = 5 at the period discriminators' rows (2 x batch x p rows for p = 2, 3, 5, 7, 11): the tables of
profiles/conv1d_split_bf16.md.  The split TFLOP/s are of the same executed MACs (each as three bf16 MFMAs, not counted thrice).

    python tools/conv_grad_bench.py --transpose [--batch 32] [--frames 28] [--markdown]

The same for the differentiable ConvTranspose1d (nn.conv_transpose1d, csrc/conv_grad_t.hip) on the generator's five
upsamplers against torch's conv_transpose1d autograd (leaky_relu + conv_transpose1d; aten.convolution_backward, transposed,
one output mask each): the table of profiles/conv_transpose_grad.md.  Its TFLOP/s are of the direct form's MACs,
Cin Cout k per input position (the forward's phase groups execute some zero taps on top).

    python tools/conv_grad_bench.py --strided [--batch 32] [--samples 8960] [--periods 2,11] [--markdown]

The same for the strided Conv1d (nn.conv1d_strided, csrc/conv_grad_s.hip) on the four strided layers of DiscriminatorP at the
trainer's shape, 32 segments of 8 960 samples folded to 32 p rows of ceil(8 960 / p) columns, against torch's leaky_relu +
conv1d(stride=3) autograd on the rows' valid part: the table of profiles/conv_strided_grad.md.  TFLOP/s of the direct form's
MACs, Cin Cout k per OUTPUT position (Cin = 1 executes 8 channels in the forward and 32 in the gradients).

    python tools/conv_grad_bench.py --grouped [--batch 64] [--samples 8960] [--scales 3] [--iters 50] [--markdown]

The same for the grouped Conv1d (nn.conv1d_grouped, csrc/conv_grad_g.hip) on the six grouped layers of DiscriminatorS at the
trainer's rows, 64 rows (32 segments x the real and the generated waveform) of 8 960 samples and of the two pooled scales
(4 481, 2 241), against torch's leaky_relu + conv1d(stride, groups) autograd, and for the pool (nn.mean_pool) against
F.avg_pool1d: the tables of profiles/conv_grouped_grad.md.  TFLOP/s of the direct form's MACs, (Cin / groups) Cout k per OUTPUT
position; GB/s of the bytes that have to move (x, y and, for the data gradient, gy, x and gx) for convs.0 and the pool.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def rup(x, m):
    return (x + m - 1) // m * m


def executed_flops(cin, cout, k, positions):
    """(forward, data gradient, weight gradient) as the kernels execute them"""
    def direct(m, c):
        return 2.0 * rup(m, 32 if m >= 32 else 16) * rup(c, 16) * k * positions
    cib = 32
    while cib > 1 and cib // 2 >= cin:
        cib //= 2
    ng = -(-k // (32 // cib))
    return direct(cout, cin), direct(cin, cout), 2.0 * rup(cout, 32) * 32 * -(-cin // 32) * ng * positions


def bench_layer(a, kind, cin, cout, k, p_, L, groups=1):
    """one layer through its nn layer kind (nn.CONV1D: p_ = dilation; nn.CONV_TRANSPOSE1D, nn.CONV1D_STRIDED, nn.CONV1D_GROUPED:
    p_ = stride) and through torch"""
    from dissc_amd import nn
    from dissc_amd._lib import check, current_stream_ptr
    F = torch.nn.functional
    dev = torch.device("cuda:0")
    tr, sd = kind is nn.CONV_TRANSPOSE1D, kind in (nn.CONV1D_STRIDED, nn.CONV1D_GROUPED)
    cig = cin // groups
    s, d = (p_, 1) if tr or sd else (1, p_)
    B, slope = a.batch, 0.1
    rs = np.random.RandomState(0)
    ld = rup(L, 4)
    ldo, nout = kind.ldo(p_, ld), kind.nout(p_, L)  # the row of y / gy, and the outputs of L inputs
    x = torch.from_numpy(rs.standard_normal((B, cin, ld)).astype(np.float32)).to(dev)
    gy = torch.from_numpy(rs.standard_normal((B, cout, ldo)).astype(np.float32)).to(dev)
    w = torch.from_numpy((rs.uniform(-1, 1, (cin, cout, k) if tr else (cout, cig, k)) / np.sqrt(cig * k / (s if tr else 1))).astype(np.float32)).to(dev)
    b = torch.from_numpy(rs.uniform(-1, 1, cout).astype(np.float32)).to(dev)
    if kind is nn.CONV1D and ld != L:  # (the MPD rows: torch runs on whole rows, so the columns the layer never reads are zero)
        x[:, :, L:], gy[:, :, L:] = 0.0, 0.0
    lengths = torch.full((B,), L, dtype=torch.int32, device=dev)
    y, gx, gw, gb = torch.zeros_like(gy), torch.empty_like(x), torch.empty_like(w), torch.empty_like(b)
    h = nn._handle(kind, cin, cout, k, p_, dev, groups)
    split = kind is nn.CONV1D and getattr(a, "precision", "fp32") == "split_bf16"
    hs = nn._handle(kind, cin, cout, k, p_, dev, prec=1) if split else None  # (a handle of its own: both stay packed)
    st = current_stream_ptr(dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    nws = int(kind.workspace_bytes(h, B, ld))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    check(kind.set_weights(h, p(w), p(b), st), "set_weights")
    pad = (k - s) // 2 if tr else (k - 1) * d // 2
    add = () if tr or sd else (None,)
    # torch runs the strided layer on the rows' valid part: ceil(L / s) outputs of L inputs
    xt, gyt = (x[:, :, :L].contiguous(), gy[:, :, :nout].contiguous()) if sd else (x, gy)

    def ours_bwd(gx_, gw_, gb_):
        check(kind.backward(h, p(x), p(gy), p(lengths), B, ld, ldo, ld, slope, gx_, gw_, gb_, p(ws), nws, st), "backward")

    xa = F.leaky_relu(xt, slope)
    conv_bwd = torch.ops.aten.convolution_backward

    def torch_bwd(mask):
        return conv_bwd(gyt, xa, w, [cout], [s], [pad], [d], tr, [0], groups, mask)

    def torch_fwd():
        xl = F.leaky_relu(xt, slope)
        return F.conv_transpose1d(xl, w, b, stride=s, padding=pad) if tr else F.conv1d(xl, w, b, stride=s, padding=pad, dilation=d, groups=groups)

    cases = {
        "fwd": lambda: check(kind.forward(h, p(x), *add, p(y), p(lengths), B, ld, ldo, ld, slope, st), "forward"),
        "torch_fwd": torch_fwd,
        "dgrad": lambda: ours_bwd(p(gx), None, None),
        "torch_dgrad": lambda: torch_bwd([True, False, False]),
        "wgrad": lambda: ours_bwd(None, p(gw), p(gb)),
        "torch_wgrad": lambda: torch_bwd([False, True, True]),
        "repack": lambda: check(kind.set_weights(h, p(w), p(b), st), "set_weights"),
    }
    if split:
        ys, gxs, gws, gbs = torch.zeros_like(gy), torch.empty_like(x), torch.empty_like(w), torch.empty_like(b)
        check(kind.set_weights(hs, p(w), p(b), st), "set_weights")
        s_bwd = lambda gx_, gw_, gb_: check(kind.backward(hs, p(x), p(gy), p(lengths), B, ld, ldo, ld, slope, gx_, gw_, gb_, p(ws), nws, st),
                                            "backward")
        cases.update({
            "split_fwd": lambda: check(kind.forward(hs, p(x), None, p(ys), p(lengths), B, ld, ldo, ld, slope, st), "forward"),
            "split_dgrad": lambda: s_bwd(p(gxs), None, None),
            "split_wgrad": lambda: s_bwd(None, p(gws), p(gbs)),
            "split_repack": lambda: check(kind.set_weights(hs, p(w), p(b), st), "set_weights"),
        })
        cases["split_fwd"](), cases["split_dgrad"](), cases["split_wgrad"]()
    # agreement first (fp32 both sides)
    cases["fwd"](), cases["dgrad"](), cases["wgrad"]()
    tg = torch_bwd([True, True, True])
    rel = lambda u, v: float((u - v).norm() / v.norm())
    valid = (torch.arange(ld, device=dev) < L).float()
    if sd:
        assert not gx[:, :, L:].any() and not y[:, :, nout:].any()
        agree = {"y": rel(y[:, :, :nout], torch_fwd()), "gx": rel(gx[:, :, :L], tg[0] * torch.where(xt > 0, 1.0, slope)),
                 "gw": rel(gw, tg[1]), "gb": rel(gb, tg[2])}
    else:
        agree = {"y": rel(y[:, :, :s * L], torch_fwd()[:, :, :s * L]) if ld == L else None,
                 "gx": rel(gx, tg[0] * torch.where(x > 0, 1.0, slope) * valid), "gw": rel(gw, tg[1]), "gb": rel(gb, tg[2])}
    for fn in cases.values():
        timed(fn, 2)
    times = {n: [] for n in cases}
    for _ in range(a.blocks):
        for n, fn in cases.items():  # alternating
            times[n].append(timed(fn, a.iters))
    P, pairs = nn._partials(kind, B, ld, cin, cout, k, p_, groups)
    out = {"transpose": True} if tr else ({"strided": True} if sd else {})
    if kind.grouped:
        out = {"grouped": True, "groups": groups}
    out.update({"cin": cin, "cout": cout, "k": k, "stride" if tr or sd else "dilation": p_, "L": L, "batch": B, "partials": P,
                "pairs_per_partial": pairs, "workspace_mb": round(nws / 2**20, 2),
                "rel_diff_to_torch": {n: None if v is None else float(f"{v:.2e}") for n, v in agree.items()}})
    for n, v in times.items():
        out[n + "_ms"] = round(float(np.median(v)), 4)
        out[n + "_ms_spread"] = [round(float(min(v)), 4), round(float(max(v)), 4)]
        if split:
            out[n + "_ms_blocks"] = [round(float(t), 4) for t in v]
    if split:
        out["split"] = dict(zip(("fwd", "dgrad", "wgrad"), nn.conv1d_precision(cin, cout, k, p_)))
        out["split_rel_diff_to_torch"] = {"gx": float(f"{rel(gxs, tg[0] * torch.where(x > 0, 1.0, slope) * valid):.2e}"),
                                          "gw": float(f"{rel(gws, tg[1]):.2e}"), "gb": float(f"{rel(gbs, tg[2]):.2e}")}
    # the transposed layer: the direct form's MACs, Cin Cout k per input position
    flops = [2.0 * cig * cout * k * B * (nout if sd else L)] * 3 if tr or sd else executed_flops(cin, cout, k, B * L)
    for n, fl in zip(("fwd", "dgrad", "wgrad"), flops):
        out[n + "_tflops"] = round(fl / (out[n + "_ms"] * 1e-3) / 1e12, 2)
        if split:
            out["split_" + n + "_tflops"] = round(fl / (out["split_" + n + "_ms"] * 1e-3) / 1e12, 2)
    print(json.dumps(out), flush=True)
    return out


def main_transpose(a):
    import conv_transpose_grad_ref as RT
    from dissc_amd import nn
    rows, L = [], a.frames
    for cin, cout, k, s in RT.ups_from_config():
        if not a.only or [cin, cout, k] == [int(v) for v in a.only.split(",")]:
            rows.append(bench_layer(a, nn.CONV_TRANSPOSE1D, cin, cout, k, s, L))
        L *= s
    if a.markdown:
        print("| layer | L in | fwd ms (torch) | dgrad ms (torch) | wgrad ms (torch) | TFLOP/s fwd / dgrad / wgrad | P | repack ms |")
        print("|---|---|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['cin']} -> {r['cout']}, k = {r['k']}, s = {r['stride']} | {r['L']} | {r['fwd_ms']:.3f} ({r['torch_fwd_ms']:.3f}) | "
                  f"{r['dgrad_ms']:.3f} ({r['torch_dgrad_ms']:.3f}) | {r['wgrad_ms']:.3f} ({r['torch_wgrad_ms']:.3f}) | "
                  f"{r['fwd_tflops']} / {r['dgrad_tflops']} / {r['wgrad_tflops']} | {r['partials']} | {r['repack_ms']:.3f} |")
        tot = lambda n: sum(r[n] for r in rows)
        print(f"\nsum over the five upsamplers, ours (torch): fwd {tot('fwd_ms'):.2f} ({tot('torch_fwd_ms'):.2f}), "
              f"dgrad {tot('dgrad_ms'):.2f} ({tot('torch_dgrad_ms'):.2f}), wgrad {tot('wgrad_ms'):.2f} ({tot('torch_wgrad_ms'):.2f}) ms")
    return rows


def main_strided(a):
    import conv_strided_ref as RS
    from dissc_amd import nn
    rows, batch = [], a.batch
    for period in (int(v) for v in a.periods.split(",")):
        L, a.batch = -(-a.samples // period), batch * period  # the fold: every utterance is `period` rows
        for cin, cout, k, s in RS.DISC_P:
            if not a.only or [cin, cout, k] == [int(v) for v in a.only.split(",")]:
                rows.append(dict(bench_layer(a, nn.CONV1D_STRIDED, cin, cout, k, s, L), period=period))
            L = -(-L // s)
    a.batch = batch
    if a.markdown:
        print("| period | layer | rows x L in | fwd ms (torch) | dgrad ms (torch) | wgrad ms (torch) | TFLOP/s fwd / dgrad / wgrad | P | repack ms |")
        print("|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['period']} | {r['cin']} -> {r['cout']}, k = {r['k']}, s = {r['stride']} | {r['batch']} x {r['L']} | "
                  f"{r['fwd_ms']:.3f} ({r['torch_fwd_ms']:.3f}) | {r['dgrad_ms']:.3f} ({r['torch_dgrad_ms']:.3f}) | "
                  f"{r['wgrad_ms']:.3f} ({r['torch_wgrad_ms']:.3f}) | {r['fwd_tflops']} / {r['dgrad_tflops']} / {r['wgrad_tflops']} | "
                  f"{r['partials']} | {r['repack_ms']:.3f} |")
        tot = lambda n: sum(r[n] for r in rows)
        print(f"\nsum over the listed layers, ours (torch): fwd {tot('fwd_ms'):.2f} ({tot('torch_fwd_ms'):.2f}), "
              f"dgrad {tot('dgrad_ms'):.2f} ({tot('torch_dgrad_ms'):.2f}), wgrad {tot('wgrad_ms'):.2f} ({tot('torch_wgrad_ms'):.2f}) ms")
        slower = [(r["period"], r["cin"], r["cout"], n) for r in rows for n in ("fwd", "dgrad", "wgrad") if r[n + "_ms"] > r["torch_" + n + "_ms"]]
        print("slower than torch:", slower if slower else "none")
    return rows


def bench_pool(a, T):
    """nn.mean_pool's two kernels through the C ABI against F.avg_pool1d(4, 2, padding=2) and its autograd"""
    from dissc_amd import nn
    from dissc_amd._lib import check, current_stream_ptr, lib
    F = torch.nn.functional
    dev = torch.device("cuda:0")
    B, no = a.batch, T // 2 + 1
    ldo = rup(no, 4)
    rs = np.random.RandomState(1)
    x = torch.from_numpy(rs.standard_normal((B, 1, T)).astype(np.float32)).to(dev)
    g = torch.from_numpy(rs.standard_normal((B, 1, ldo)).astype(np.float32)).to(dev)
    out, gx = torch.zeros_like(g), torch.empty_like(x)
    st = current_stream_ptr(dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    xr = x.clone().requires_grad_(True)
    yr = F.avg_pool1d(xr, 4, 2, padding=2)
    gr = g[:, :, :no].contiguous()
    cases = {
        "fwd": lambda: check(lib.dissc_mean_pool_fwd(p(x), p(out), None, B, 1, T, T, ldo, st), "dissc_mean_pool_fwd"),
        "torch_fwd": lambda: F.avg_pool1d(x, 4, 2, padding=2),
        "bwd": lambda: check(lib.dissc_mean_pool_bwd(p(g), p(gx), None, B, 1, T, T, ldo, st), "dissc_mean_pool_bwd"),
        "torch_bwd": lambda: torch.autograd.grad(yr, xr, gr, retain_graph=True),
    }
    cases["fwd"](), cases["bwd"]()
    agree = {"out": float((out[:, :, :no] - cases["torch_fwd"]()).abs().max()), "gx": float((gx - cases["torch_bwd"]()[0]).abs().max())}
    for fn in cases.values():
        timed(fn, 2)
    times = {n: [] for n in cases}
    for _ in range(a.blocks):
        for n, fn in cases.items():
            times[n].append(timed(fn, a.iters))
    r = {"pool": True, "T": T, "batch": B, "max_abs_diff_to_torch": agree}
    for n, v in times.items():
        r[n + "_ms"] = round(float(np.median(v)), 4)
    nbytes = 4.0 * B * (T + no)
    r["fwd_gbs"], r["bwd_gbs"] = (round(nbytes / (r[n] * 1e-3) / 1e9, 1) for n in ("fwd_ms", "bwd_ms"))
    print(json.dumps(r), flush=True)
    return r


def main_grouped(a):
    import conv_grouped_ref as RG
    from dissc_amd import nn
    rows, pools, T = [], [], a.samples
    for scale in range(a.scales):
        L = T
        for i, (cin, cout, k, s, g) in enumerate(RG.DISC_S):
            if not a.only or [cin, cout, k] == [int(v) for v in a.only.split(",")]:
                r = dict(bench_layer(a, nn.CONV1D_GROUPED, cin, cout, k, s, L, g), scale=scale, layer=f"convs.{i}")
                if i == 0:  # bandwidth bound: x and y forward; gy, x and gx in the data gradient
                    r["fwd_gbs"] = round(4.0 * a.batch * L * (cin + cout) / (r["fwd_ms"] * 1e-3) / 1e9, 1)
                    r["dgrad_gbs"] = round(4.0 * a.batch * L * (2 * cin + cout) / (r["dgrad_ms"] * 1e-3) / 1e9, 1)
                rows.append(r)
            L = -(-L // s)
        if scale + 1 < a.scales:
            pools.append(bench_pool(a, T))
            T = T // 2 + 1
    if a.markdown:
        print("| scale | layer | rows x L in | fwd ms (torch) | dgrad ms (torch) | wgrad ms (torch) | TFLOP/s fwd / dgrad / wgrad | P | repack ms |")
        print("|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['scale']} | {r['layer']}: {r['cin']} -> {r['cout']}, k = {r['k']}, s = {r['stride']}, g = {r['groups']} | "
                  f"{r['batch']} x {r['L']} | {r['fwd_ms']:.3f} ({r['torch_fwd_ms']:.3f}) | {r['dgrad_ms']:.3f} ({r['torch_dgrad_ms']:.3f}) | "
                  f"{r['wgrad_ms']:.3f} ({r['torch_wgrad_ms']:.3f}) | {r['fwd_tflops']} / {r['dgrad_tflops']} / {r['wgrad_tflops']} | "
                  f"{r['partials']} | {r['repack_ms']:.3f} |")
        for r in rows:
            if "fwd_gbs" in r:
                print(f"\nscale {r['scale']} convs.0: forward {r['fwd_gbs']} GB/s, data gradient {r['dgrad_gbs']} GB/s")
        for r in pools:
            print(f"\npool {r['batch']} x {r['T']}: fwd {r['fwd_ms']:.4f} ms ({r['torch_fwd_ms']:.4f} torch), {r['fwd_gbs']} GB/s; "
                  f"bwd {r['bwd_ms']:.4f} ms ({r['torch_bwd_ms']:.4f} torch), {r['bwd_gbs']} GB/s")
        tot = lambda n: sum(r[n] for r in rows)
        print(f"\nsum over the listed layers, ours (torch): fwd {tot('fwd_ms'):.2f} ({tot('torch_fwd_ms'):.2f}), "
              f"dgrad {tot('dgrad_ms'):.2f} ({tot('torch_dgrad_ms'):.2f}), wgrad {tot('wgrad_ms'):.2f} ({tot('torch_wgrad_ms'):.2f}) ms")
        slower = [(r["scale"], r["layer"], n) for r in rows for n in ("fwd", "dgrad", "wgrad") if r[n + "_ms"] > r["torch_" + n + "_ms"]]
        print("slower than torch:", slower if slower else "none")
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=28)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", default=None, help="CIN,COUT,K: that shape only")
    ap.add_argument("--markdown", action="store_true")
    ap.add_argument("--transpose", action="store_true", help="the five ConvTranspose1d upsamplers instead")
    ap.add_argument("--strided", action="store_true", help="the four strided layers of DiscriminatorP instead")
    ap.add_argument("--grouped", action="store_true", help="the six grouped layers of DiscriminatorS and the pool instead")
    ap.add_argument("--scales", type=int, default=3, help="--grouped: the scales (each pooled from the one before)")
    ap.add_argument("--samples", type=int, default=8960, help="--strided, --grouped: samples per segment")
    ap.add_argument("--periods", default="2,11", help="--strided: the periods to fold to")
    ap.add_argument("--precision", default="fp32", choices=("fp32", "split_bf16"), help="split_bf16: the split handle's columns too")
    ap.add_argument("--mpd", action="store_true", help="also 1024 -> 1024, k = 5 at the period discriminators' rows")
    a = ap.parse_args(argv)
    if a.transpose:
        return main_transpose(a)
    if a.strided:
        return main_strided(a)
    if a.grouped:
        return main_grouped(a)
    import conv_grad_ref as R
    from dissc_amd import nn
    seen, rows = set(), []
    for cin, cout, k, d, L in R.generator_layer_shapes(a.frames):
        if (cin, cout, k) in seen or d not in (1, 3) or (cin == cout and d != 3):
            continue  # one dilation per shape (3 for the ResBlock convs): it moves no work
        if a.only and [cin, cout, k] != [int(v) for v in a.only.split(",")]:
            continue
        seen.add((cin, cout, k))
        rows.append(bench_layer(a, nn.CONV1D, cin, cout, k, d, L))
    mpd_rows = []
    if a.mpd:  # convs.4 of DiscriminatorP: 2 x batch x p rows (y and y_hat as one batch) of the fold's columns behind four stride-3 layers
        batch = a.batch
        for period in (2, 3, 5, 7, 11):
            L = -(-a.samples // period)
            for _ in range(4):
                L = -(-L // 3)
            a.batch = 2 * batch * period
            mpd_rows.append(dict(bench_layer(a, nn.CONV1D, 1024, 1024, 5, 1, L), period=period))
        a.batch = batch
    if a.markdown and a.precision == "split_bf16":
        print("| layer | rows x L | fwd ms fp32 / split (torch) | dgrad ms fp32 / split (torch) | wgrad ms fp32 / split (torch) | "
              "split TFLOP/s fwd / dgrad / wgrad | split directions | repack ms fp32 / split |")
        print("|---|---|---|---|---|---|---|---|")
        for r in rows + mpd_rows:
            tri = lambda n: f"{r[n + '_ms']:.3f} / {r['split_' + n + '_ms']:.3f} ({r['torch_' + n + '_ms']:.3f})"
            print(f"| {r['cin']} -> {r['cout']}, k = {r['k']}{' (MPD p = %d)' % r['period'] if 'period' in r else ''} | {r['batch']} x {r['L']} | "
                  f"{tri('fwd')} | {tri('dgrad')} | {tri('wgrad')} | {r['split_fwd_tflops']} / {r['split_dgrad_tflops']} / "
                  f"{r['split_wgrad_tflops']} | {'/'.join(n for n, v in r['split'].items() if v) or 'none'} | "
                  f"{r['repack_ms']:.3f} / {r['split_repack_ms']:.3f} |")
        mult = lambda r: 6 if r["cin"] == r["cout"] else 1  # a ResBlock has six convs of its shape
        for n in ("fwd", "dgrad", "wgrad") if rows else ():
            nb = len(rows[0][n + "_ms_blocks"])
            per = lambda key: [round(sum(r[key + "_ms_blocks"][i] * mult(r) for r in rows), 3) for i in range(nb)]
            print(f"\nsum over the generator's 92 stride-1 layers, {n}, per block: fp32 {per(n)} split {per('split_' + n)} torch {per('torch_' + n)} ms")
        slower = [(r["cin"], r["cout"], r["k"], r.get("period"), n) for r in rows + mpd_rows for n in ("fwd", "dgrad", "wgrad")
                  if r["split"][n] and r["split_" + n + "_ms"] > r[n + "_ms"]]
        print("split slower than fp32:", slower if slower else "none")
    elif a.markdown:
        print("| layer | L | fwd ms (torch) | dgrad ms (torch) | wgrad ms (torch) | TFLOP/s fwd / dgrad / wgrad | P | repack ms |")
        print("|---|---|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['cin']} -> {r['cout']}, k = {r['k']} | {r['L']} | {r['fwd_ms']:.3f} ({r['torch_fwd_ms']:.3f}) | "
                  f"{r['dgrad_ms']:.3f} ({r['torch_dgrad_ms']:.3f}) | {r['wgrad_ms']:.3f} ({r['torch_wgrad_ms']:.3f}) | "
                  f"{r['fwd_tflops']} / {r['dgrad_tflops']} / {r['wgrad_tflops']} | {r['partials']} | {r['repack_ms']:.3f} |")
        tot = lambda n: sum(r[n] * (6 if r["cin"] == r["cout"] else 1) for r in rows)  # a ResBlock has six convs of its shape
        print(f"\nsum over the generator's 92 stride-1 layers, ours (torch): "
              f"fwd {tot('fwd_ms'):.2f} ({tot('torch_fwd_ms'):.2f}), dgrad {tot('dgrad_ms'):.2f} ({tot('torch_dgrad_ms'):.2f}), "
              f"wgrad {tot('wgrad_ms'):.2f} ({tot('torch_wgrad_ms'):.2f}) ms")
    return rows


if __name__ == "__main__":
    main()
