#!/usr/bin/env python
"""Per-launch gate of the one-launch F(2,3) chains of the k = 3 ResBlocks (reschain32_f23_kernel, reschain16_f23_kernel) against
the three one-launch pairs they replace, through dissc_chain_bench (B = 32; C = 32 x L = 80 000 and C = 16 x L = 160 000;
EPI_MRF_SET, the epilogue of a stage's first chain):

    python tools/chain_gate.py [--stage 32|16] [--blocks 10] [--iters 100] [--ko]

Mode 0 (three launches) and mode 1 (the chain) live in a process of their own each and take turns, one block of `iters` launches
each, `blocks` times per stage.  A stage passes when EVERY block of the chain is below EVERY block of the three launches.  --ko:
after the table, one block of the chain per knock-out (kernel_dbg 1: no tap loops, 2: no T / x_k epilogues, 4: no output epilogue,
7: skeleton).  Exit status 1 if a stage does not pass.
A worker that does not answer within --block-timeout seconds, or ends, ends the run; nothing more is started after that."""
import argparse
import ctypes
import os
import select
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGES = {32: 80000, 16: 160000}
EPI_MRF_SET = 2


def worker():
    sys.path.insert(0, ROOT)
    from dissc_amd._lib import lib, check
    ms = ctypes.c_float()
    for line in sys.stdin:
        mode, C, iters, dbg = (int(v) for v in line.split())
        check(lib.dissc_set_option(b"kernel_dbg", dbg), "kernel_dbg")
        check(lib.dissc_chain_bench(32, C, STAGES[C], EPI_MRF_SET, iters, mode, ctypes.byref(ms)), "dissc_chain_bench")
        print(f"{ms.value * 1e3:.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stage", type=int, default=0, choices=(0, 16, 32))
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

    def block(mode, C, dbg=0):
        p = procs[mode]
        p.stdin.write(f"{mode} {C} {a.iters} {dbg}\n")
        p.stdin.flush()
        if not select.select([p.stdout], [], [], a.block_timeout)[0]:
            raise RuntimeError(f"the worker of mode {mode} gave no answer in {a.block_timeout} s")
        line = p.stdout.readline()
        if not line:
            raise RuntimeError(f"the worker of mode {mode} ended (exit status {p.wait()})")
        return float(line)

    failed = 0
    try:
        for C in ([a.stage] if a.stage else [32, 16]):
            us = ([], [])
            for _ in range(a.blocks):
                us[0].append(block(0, C))
                us[1].append(block(1, C))
            med = [sorted(v)[len(v) // 2] for v in us]
            ok = max(us[1]) < min(us[0])
            failed += not ok
            print(f"GATE C={C} L={STAGES[C]}: three launches median {med[0]:7.1f} us (min {min(us[0]):.1f} max {max(us[0]):.1f}) | "
                  f"one chain launch median {med[1]:7.1f} us (min {min(us[1]):.1f} max {max(us[1]):.1f}) | "
                  f"{100 * (med[1] / med[0] - 1):+.2f} % | {'passes' if ok else 'DOES NOT PASS'}", flush=True)
            if a.ko:
                t = {dbg: block(1, C, dbg) for dbg in (0, 1, 2, 4, 7)}
                print(f"KO   C={C}: full {t[0]:.1f} us | no tap loops {t[1]:.1f} | no T / x_k epilogues {t[2]:.1f} | "
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
