#!/usr/bin/env python
"""Per-launch gate of the one-launch register-only pairs of the 64-channel stage (k = 3: respair64_f23_kernel, k = 7 / 11:
respair64_tc6_kernel) against the two transform-domain launches they replace, through dissc_pair_bench (B = 32, C = 64,
L = 40 000):

    python tools/pair64_gate.py [--k 3|7|11] [--blocks 10] [--iters 100] [--ko]

The old form (k = 3: mode 2, two conv_wino launches; k = 7 / 11: mode 4, the two launches in the forms the plan gives the shape)
and mode 3 (the new form; for k = 7 / 11 under "pair_tc6_c64" = 3) live in a process of their own each and take turns, one block
of `iters` launches each, `blocks` times per shape: d = 1 / 3 with EPI_RES, d = 5 with the MRF epilogue of the chain's last pair
(k = 3 is the stage's first chain: EPI_MRF_SET; k = 7 its second: EPI_MRF_ADD; k = 11 its last: EPI_MRF_DIV).  A shape passes
when the new median is below the old form's median by more than the spread (max - min) of the old form's own blocks; the last line
sums the three shapes the same way.  --ko: after the table, one block of the new form per knock-out (kernel_dbg 1: no tap loops,
2: no T epilogue, 4: no output epilogue, 7: skeleton; six points also 8: every step loads the first step's weights).  Exit
status 1 if a shape does not pass.
A worker that does not answer within --block-timeout seconds, or ends, ends the run; nothing more is started after that."""
import argparse
import ctypes
import os
import select
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAST_EPI = {3: 2, 7: 3, 11: 4}  # the MRF epilogue of the d = 5 pair of the k chain


def worker():
    sys.path.insert(0, ROOT)
    from dissc_amd._lib import lib, check
    ms = ctypes.c_float()
    check(lib.dissc_set_option(b"pair_tc6_c64", 3), "pair_tc6_c64")  # (mode 3 at k = 7 / 11; no other mode or k reads it)
    for line in sys.stdin:
        mode, k, d, epi, iters, dbg = (int(v) for v in line.split())
        check(lib.dissc_set_option(b"kernel_dbg", dbg), "kernel_dbg")
        check(lib.dissc_pair_bench(32, 64, k, d, 40000, epi, iters, mode, ctypes.byref(ms)), "dissc_pair_bench")
        print(f"{ms.value * 1e3:.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=3, choices=(3, 7, 11))
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--ko", action="store_true")
    ap.add_argument("--block-timeout", type=float, default=120.0)
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker()
    k, old_mode = a.k, 2 if a.k == 3 else 4
    shapes = [(1, 1), (3, 1), (5, LAST_EPI[k])]  # (dilation, epilogue)
    names = ("two conv_wino launches", "one F(2,3) launch") if k == 3 else ("two transform-domain launches", "one six-point launch")
    kos = (0, 1, 2, 4, 7) if k == 3 else (0, 1, 2, 4, 7, 8)
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker"], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                              text=True) for _ in range(2)]

    def block(side, mode, d, epi, dbg=0):
        p = procs[side]
        p.stdin.write(f"{mode} {k} {d} {epi} {a.iters} {dbg}\n")
        p.stdin.flush()
        if not select.select([p.stdout], [], [], a.block_timeout)[0]:
            raise RuntimeError(f"the worker of mode {mode} gave no answer in {a.block_timeout} s")
        line = p.stdout.readline()
        if not line:
            raise RuntimeError(f"the worker of mode {mode} ended (exit status {p.wait()})")
        return float(line)

    failed = 0
    total = [0.0, 0.0, 0.0]  # old medians, new medians, old spreads
    try:
        for d, epi in shapes:
            us = ([], [])
            for _ in range(a.blocks):
                us[0].append(block(0, old_mode, d, epi))
                us[1].append(block(1, 3, d, epi))
            med = [sorted(v)[len(v) // 2] for v in us]
            spread = max(us[0]) - min(us[0])
            ok = med[1] < med[0] - spread
            failed += not ok
            total = [total[0] + med[0], total[1] + med[1], total[2] + spread]
            print(f"GATE C=64 k={k} d={d} epi={epi}: {names[0]} median {med[0]:7.1f} us (min {min(us[0]):.1f} max {max(us[0]):.1f}) | "
                  f"{names[1]} median {med[1]:7.1f} us (min {min(us[1]):.1f} max {max(us[1]):.1f}) | "
                  f"{100 * (med[1] / med[0] - 1):+.2f} % | {'passes' if ok else 'DOES NOT PASS'}", flush=True)
        print(f"SUM  C=64 k={k}: old {total[0]:.1f} us, new {total[1]:.1f} us, old spreads {total[2]:.1f} us | "
              f"{'passes' if total[1] < total[0] - total[2] else 'DOES NOT PASS'}", flush=True)
        if a.ko:
            for d, epi in shapes:
                t = {dbg: block(1, 3, d, epi, dbg) for dbg in kos}
                print(f"KO   C=64 k={k} d={d} epi={epi}: full {t[0]:.1f} us | no tap loops {t[1]:.1f} | no T epilogue {t[2]:.1f} | "
                      f"no output epilogue {t[4]:.1f} | skeleton {t[7]:.1f}" + (f" | one weight step {t[8]:.1f}" if 8 in t else ""),
                      flush=True)
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
