#!/usr/bin/env python
"""Per-launch gate of the one-launch F(2,3) pairs of the 64-channel stage (respair64_f23_kernel) against the two conv_wino
launches they replace, through dissc_pair_bench (B = 32, C = 64, k = 3, L = 40 000):

    python tools/pair64_gate.py [--blocks 10] [--iters 100] [--ko]

Mode 2 (two conv_wino launches) and mode 3 (the new form) live in a process of their own each and take turns, one block of
`iters` launches each, `blocks` times per shape: d = 1 / 3 with EPI_RES, d = 5 with EPI_MRF_SET (the k = 3 chain is the stage's
first: its last pair sets the MRF accumulator).  A shape passes when the new median is below the old form's median by more than
the spread (max - min) of the old form's own blocks.  --ko: after the table, one block of the new form per knock-out
(kernel_dbg 1: no tap loops, 2: no T epilogue, 4: no output epilogue, 7: skeleton).  Exit status 1 if a shape does not pass.
A worker that does not answer within --block-timeout seconds, or ends, ends the run; nothing more is started after that."""
import argparse
import ctypes
import os
import select
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (3, 1), (5, 2)]  # (dilation, epilogue)


def worker():
    sys.path.insert(0, ROOT)
    from dissc_amd._lib import lib, check
    ms = ctypes.c_float()
    for line in sys.stdin:
        mode, d, epi, iters, dbg = (int(v) for v in line.split())
        check(lib.dissc_set_option(b"kernel_dbg", dbg), "kernel_dbg")
        check(lib.dissc_pair_bench(32, 64, 3, d, 40000, epi, iters, mode, ctypes.byref(ms)), "dissc_pair_bench")
        print(f"{ms.value * 1e3:.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--ko", action="store_true")
    ap.add_argument("--block-timeout", type=float, default=120.0)
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker()
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker"], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                              text=True) for _ in range(2)]

    def block(side, mode, d, epi, dbg=0):
        p = procs[side]
        p.stdin.write(f"{mode} {d} {epi} {a.iters} {dbg}\n")
        p.stdin.flush()
        if not select.select([p.stdout], [], [], a.block_timeout)[0]:
            raise RuntimeError(f"the worker of mode {mode} gave no answer in {a.block_timeout} s")
        line = p.stdout.readline()
        if not line:
            raise RuntimeError(f"the worker of mode {mode} ended (exit status {p.wait()})")
        return float(line)

    failed = 0
    try:
        for d, epi in SHAPES:
            us = ([], [])
            for _ in range(a.blocks):
                us[0].append(block(0, 2, d, epi))
                us[1].append(block(1, 3, d, epi))
            med = [sorted(v)[len(v) // 2] for v in us]
            spread = max(us[0]) - min(us[0])
            ok = med[1] < med[0] - spread
            failed += not ok
            print(f"GATE C=64 k=3 d={d} epi={epi}: two conv_wino launches median {med[0]:7.1f} us (min {min(us[0]):.1f} max {max(us[0]):.1f}) | "
                  f"one F(2,3) launch median {med[1]:7.1f} us (min {min(us[1]):.1f} max {max(us[1]):.1f}) | "
                  f"{100 * (med[1] / med[0] - 1):+.2f} % | {'passes' if ok else 'DOES NOT PASS'}", flush=True)
        if a.ko:
            for d, epi in SHAPES:
                t = {dbg: block(1, 3, d, epi, dbg) for dbg in (0, 1, 2, 4, 7)}
                print(f"KO   C=64 k=3 d={d} epi={epi}: full {t[0]:.1f} us | no tap loops {t[1]:.1f} | no T epilogue {t[2]:.1f} | "
                      f"no output epilogue {t[4]:.1f} | skeleton {t[7]:.1f}", flush=True)
    finally:
        for p in procs:
            p.stdin.close()
        for p in procs:  # (after a failure nothing more is started: a worker that does not leave by itself is killed)
            try:
                p.wait(timeout=60)
            except subprocess.TimeoutExpired:
                p.kill()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
