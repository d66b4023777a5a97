"""Time of the mel kernels on the headline batch (32 utterances of 10 s) against torch-ROCm's own composition of the same
figure (torch.stft + matmul + log + l1_loss) in the same process:

    python tools/mel_bench.py [--batch 32] [--seconds 10] [--blocks 7] [--iters 20]
    python tools/mel_bench.py --backward [--config CONFIG.json]   # the gradient, on 32 x 10 s and on the trainer's batch

Medians of alternating blocks (ours, torch, ours, ...), each block `iters` calls between two device events.  Reports the
executed TFLOP/s of `forward` and `l1` and, with --generator_ms (the generator forward of the same batch, bench.py's
figure), their share of it.  One JSON line at the end; the numbers of record are in profiles/mel.md.

--backward: `l1_loss` forward + backward against the composition's (`.backward()` through torch.stft + matmul + log +
l1_loss), and `dissc_mel_backward` alone against the composition's backward alone (forward graph built outside the
timed region is not possible with autograd, so torch's figure there is forward + backward minus its forward), on the
headline batch and on the trainer's own batch: batch_size x segment_size of the vocoder config (--config; without it the
VCTK config's values, restated in VCTK below), whose mel parameters both sides use.  `backward_linear` is the first
knock-out (no mel recompute, no log factor); --batch / --seconds / --train_batch give shapes whose tiles fill the 256 CUs
exactly (32 x 8.192 s, 256 x 8 960) to separate the tail.  One JSON line per shape.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def executed_flops(ms, frames):
    """MFMA work per frame as the kernel executes it: the kept bin blocks x (cos + sin) x the window's k range, plus the mel GEMM"""
    import mel_ref
    fb = mel_ref.mel_filterbank(ms.sampling_rate, ms.n_fft, ms.num_mels, ms.fmin, ms.fmax)
    used = np.nonzero(fb.any(axis=0))[0]
    nblk = (used.max() - used.min() + 1 + 31) // 32
    w_lo = (ms.n_fft - ms.win_size) // 2
    k = 8 * ((w_lo + ms.win_size + 7) // 8 - w_lo // 8)
    nmt = (ms.num_mels + 31) // 32
    return frames * (2.0 * (2 * 32 * nblk) * k + 2.0 * (32 * nmt) * (32 * nblk))


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


# the reference's VCTK vocoder config (sr/configs/VCTK/hubert100_lut.json), what --backward uses without --config
VCTK = {"batch_size": 64, "segment_size": 8960, "sampling_rate": 16000, "n_fft": 1024, "num_mels": 80, "hop_size": 256,
        "win_size": 1024, "fmin": 0, "fmax": 8000, "fmax_for_loss": None}


def backward_bench(a, cfg, batch, n, label):
    """every mel parameter comes from the config, through the MelSpectrogram made from it"""
    import mel_ref
    from dissc_amd import MelSpectrogram
    F = torch.nn.functional
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    x = torch.from_numpy((0.3 * rs.standard_normal((batch, n))).astype(np.float32)).to(dev)
    y = torch.from_numpy((0.3 * rs.standard_normal((batch, n))).astype(np.float32)).to(dev).requires_grad_(True)
    ms = MelSpectrogram.from_config(cfg).to(dev)
    basis = torch.from_numpy(mel_ref.mel_filterbank(ms.sampling_rate, ms.n_fft, ms.num_mels, ms.fmin, ms.fmax)).float().to(dev)
    window = torch.hann_window(ms.win_size, device=dev)
    g = torch.from_numpy(rs.standard_normal((batch, ms.num_mels, n // ms.hop_size)).astype(np.float32)).to(dev)

    def torch_mel(s):
        s = F.pad(s[:, None], (ms.pad, ms.pad), mode="reflect")[:, 0]
        spec = torch.view_as_real(torch.stft(s, ms.n_fft, hop_length=ms.hop_size, win_length=ms.win_size, window=window,
                                             center=False, return_complex=True))
        return torch.log(torch.clamp(torch.matmul(basis, torch.sqrt(spec.pow(2).sum(-1) + 1e-9)), min=1e-5))

    with torch.no_grad():
        target = torch_mel(x)

    def ours_loss():
        y.grad = None
        ms.l1_loss(x, y).backward()

    def torch_loss():
        y.grad = None
        F.l1_loss(target, torch_mel(y)).backward()  # the trainer computes the target's mel without grad, once

    def torch_loss_both():
        y.grad = None
        F.l1_loss(torch_mel(x), torch_mel(y)).backward()

    def torch_vjp():
        y.grad = None
        torch_mel(y).backward(g)

    yd = y.detach()
    cases = {"l1_loss_fwd_bwd": ours_loss, "torch_l1_loss_fwd_bwd": torch_loss_both, "torch_l1_loss_fwd_bwd_target_cached": torch_loss,
             "backward": lambda: ms.backward(yd, g), "backward_linear": lambda: ms.backward(yd, g, linear=True),
             "torch_mel_fwd_bwd": torch_vjp, "torch_mel_fwd": lambda: torch_mel(yd),
             "l1": lambda: ms.l1(x, yd), "forward": lambda: ms.forward(yd)}
    ours_loss()
    mine = y.grad.clone()
    torch_loss()
    theirs = y.grad.clone()
    agree = float((mine - theirs).abs().max() / theirs.abs().max())  # includes cells whose fp32 sign(lb - la) differs
    torch_vjp()
    agree_vjp = float((ms.backward(yd, g) - y.grad).abs().max() / y.grad.abs().max())  # a fixed cotangent: no signs to differ
    for fn in cases.values():
        timed(fn, 3)
    times = {k: [] for k in cases}
    for _ in range(a.blocks):
        for k, fn in cases.items():  # alternating
            times[k].append(timed(fn, a.iters))
    out = {"shape": label, "batch": batch, "samples": n, "l1_grad_max_rel_diff_to_torch": agree,
           "vjp_max_rel_diff_to_torch": agree_vjp}
    for k, v in times.items():
        out[k + "_ms"] = round(float(np.median(v)), 4)
        out[k + "_ms_spread"] = [round(float(min(v)), 4), round(float(max(v)), 4)]
    out["torch_mel_bwd_ms"] = round(out["torch_mel_fwd_bwd_ms"] - out["torch_mel_fwd_ms"], 4)
    print(json.dumps(out))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--generator_ms", type=float, default=None)
    ap.add_argument("--backward", action="store_true")
    ap.add_argument("--config", default=None, help="vocoder config (json): batch_size, segment_size and the mel parameters")
    ap.add_argument("--train_batch", type=int, default=None, help="segments in the trainer's batch instead of the config's")
    a = ap.parse_args(argv)
    if a.backward:
        cfg = json.load(open(a.config)) if a.config else VCTK
        n = int(a.seconds * cfg["sampling_rate"])
        return [backward_bench(a, cfg, a.batch, n, "headline"),
                backward_bench(a, cfg, a.train_batch or int(cfg["batch_size"]), int(cfg["segment_size"]), "trainer")]
    import mel_ref
    from dissc_amd import MelSpectrogram
    dev = torch.device("cuda:0")
    n = int(a.seconds * 16000)
    rs = np.random.RandomState(0)
    x = torch.from_numpy((0.3 * rs.standard_normal((a.batch, n))).astype(np.float32)).to(dev)
    y = torch.from_numpy((0.3 * rs.standard_normal((a.batch, n))).astype(np.float32)).to(dev)
    ms = MelSpectrogram().to(dev)
    basis = torch.from_numpy(mel_ref.mel_filterbank(16000, 1024, 80)).float().to(dev)
    window = torch.hann_window(1024, device=dev)

    def torch_mel(s):
        s = torch.nn.functional.pad(s[:, None], (384, 384), mode="reflect")[:, 0]
        spec = torch.view_as_real(torch.stft(s, 1024, hop_length=256, win_length=1024, window=window, center=False,
                                             return_complex=True))
        return torch.log(torch.clamp(torch.matmul(basis, torch.sqrt(spec.pow(2).sum(-1) + 1e-9)), min=1e-5))

    cases = {"forward": lambda: ms.forward(x), "l1": lambda: ms.l1(x, y),
             "torch_forward": lambda: torch_mel(x), "torch_l1": lambda: torch.nn.functional.l1_loss(torch_mel(x), torch_mel(y))}
    ours, theirs = float(ms.l1(x, y)["mean"].mean()), float(cases["torch_l1"]())
    for fn in cases.values():
        timed(fn, 3)
    times = {k: [] for k in cases}
    for _ in range(a.blocks):
        for k, fn in cases.items():  # alternating
            times[k].append(timed(fn, a.iters))
    frames = a.batch * (n // 256)
    out = {"batch": a.batch, "seconds": a.seconds, "frames": frames, "l1_ours": ours, "l1_torch": theirs}
    for k, v in times.items():
        out[k + "_ms"] = round(float(np.median(v)), 4)
        out[k + "_ms_spread"] = [round(float(min(v)), 4), round(float(max(v)), 4)]
    out["forward_tflops"] = round(executed_flops(ms, frames) / (out["forward_ms"] * 1e-3) / 1e12, 2)
    out["l1_tflops"] = round(2 * executed_flops(ms, frames) / (out["l1_ms"] * 1e-3) / 1e12, 2)
    if a.generator_ms:
        out["l1_share_of_generator"] = round(out["l1_ms"] / a.generator_ms, 4)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
