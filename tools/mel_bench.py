"""Time of the mel kernels on the headline batch (32 utterances of 10 s) against torch-ROCm's own composition of the same
figure (torch.stft + matmul + log + l1_loss) in the same process:

    python tools/mel_bench.py [--batch 32] [--seconds 10] [--blocks 7] [--iters 20]

Medians of alternating blocks (ours, torch, ours, ...), each block `iters` calls between two device events.  Reports the
executed TFLOP/s of `forward` and `l1` and, with --generator_ms (the generator forward of the same batch, bench.py's
figure), their share of it.  One JSON line at the end; the numbers of record are in profiles/mel.md.
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--generator_ms", type=float, default=None)
    a = ap.parse_args(argv)
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
