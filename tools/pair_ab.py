#!/usr/bin/env python
"""Per-launch A/B of two builds of the library on the default-path residual pairs, through dissc_pair_bench (B = 32,
L = 80 000 * 32 / C):

    python tools/pair_ab.py PARENT.so NEW.so [--blocks 10] [--iters 100]

Each library lives in a process of its own (DISSC_HIP_LIB); the two take turns, one block of `iters` launches each (after
dissc_pair_bench's own 2-launch warm-up), `blocks` times per case.  A case holds when the new median is no higher than the
parent's slowest block of the same run -- the parent's own measured spread, no fixed percentage.  Exit status 1 if a case misses.
A worker that does not answer within --block-timeout seconds, or ends, ends the run; nothing more is started after that."""
import argparse
import ctypes
import os
import select
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (mode, C, k): six points at C = 32, F(2,3) at C = 16 k = 11 (mode 3 under the default masks); the direct pairs (mode 1)
CASES = [(3, 32, 7), (3, 32, 11), (3, 16, 11), (1, 16, 7), (1, 32, 3), (1, 16, 3)]


def worker():
    sys.path.insert(0, ROOT)
    from dissc_amd._lib import lib, check
    ms = ctypes.c_float()
    for line in sys.stdin:
        mode, C, k, d, epi, iters = (int(v) for v in line.split())
        check(lib.dissc_pair_bench(32, C, k, d, 80000 * 32 // C, epi, iters, mode, ctypes.byref(ms)), "dissc_pair_bench")
        print(f"{ms.value * 1e3:.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--block-timeout", type=float, default=120.0, help="seconds a worker may take over one block (the first includes start-up)")
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker()
    assert len(a.libs) == 2, "two libraries: parent, new"
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker"], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                              text=True, env=dict(os.environ, DISSC_HIP_LIB=os.path.abspath(p))) for p in a.libs]
    missed = 0
    try:
        for mode, C, k in CASES:
            for d in (1, 3, 5):
                epi = 3 if d == 5 else 1
                us = ([], [])
                for _ in range(a.blocks):
                    for side, p in enumerate(procs):
                        p.stdin.write(f"{mode} {C} {k} {d} {epi} {a.iters}\n")
                        p.stdin.flush()
                        if not select.select([p.stdout], [], [], a.block_timeout)[0]:
                            raise RuntimeError(f"the worker of {a.libs[side]} gave no answer in {a.block_timeout} s")
                        line = p.stdout.readline()
                        if not line:
                            raise RuntimeError(f"the worker of {a.libs[side]} ended (exit status {p.wait()})")
                        us[side].append(float(line))
                med = [sorted(v)[len(v) // 2] for v in us]
                ok = med[1] <= max(us[0])
                missed += not ok
                print(f"AB mode={mode} C={C} k={k} d={d} epi={epi}: parent median {med[0]:7.1f} us (min {min(us[0]):.1f} max {max(us[0]):.1f}) | "
                      f"new median {med[1]:7.1f} us (min {min(us[1]):.1f} max {max(us[1]):.1f}) | {100 * (med[1] / med[0] - 1):+.2f} % | "
                      f"{'holds' if ok else 'MISSES'}", flush=True)
    finally:
        for p in procs:
            p.stdin.close()
        for p in procs:  # (after a failure nothing more is started: a worker that does not leave by itself is killed)
            try:
                p.wait(timeout=60)
            except subprocess.TimeoutExpired:
                p.kill()
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
