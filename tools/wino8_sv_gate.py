#!/usr/bin/env python
"""Per-launch gate of conv_wino8.hip's shared-transform form (option "wino8_sv"): the 18 launches of the 256- and 128-channel
stages that the default plan puts on the 128 x 64 tile (all as F(5,4)), at B = 32 x 10 s, through dissc_conv_bench.  The two
forms alternate in blocks inside this one process (a warm-up call, then a timed one per block); per launch the median, min and
max of the blocks of either form, and the sums over the 18.
    timeout -k 10 300 python tools/wino8_sv_gate.py [blocks, default 5] [iterations per block, default 20]
One process, one GPU step: run it under a time limit of its own, as above (about 25 s at the defaults), and chain it to the steps
around it with &&."""
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dissc_amd import _lib  # noqa: E402

L = _lib.lib
NBLK = int(sys.argv[1]) if len(sys.argv) > 1 else 5
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
F54 = 12  # dissc_conv_bench flags: the eight-point kernel as F(5,4)
# A hand copy of the default plan's 18 launches on the (4, 2, 2) tile (gen_plan.hip: wino8_mask / wino8_r4_mask; the rows
# conv_wino8_kernel<.., 4, 2, 2, 4, ..> of profiles/r15/gen_per_layer.md): check it against that table when a mask changes.
# (C, L, k, d, epilogue, launches of that kind per forward): conv1 stores (0), conv2 adds the residual (1), the last conv2 of a
# ResBlock takes its MRF mode (k = 7: add, 3; k = 11: add and divide, 4)
LAUNCHES = [(256, 2500, 7, 1, 0, 1), (256, 2500, 7, 1, 1, 2), (256, 2500, 7, 5, 0, 1), (256, 2500, 7, 1, 3, 1), (256, 2500, 11, 5, 0, 1),
            (128, 10000, 7, 1, 0, 1), (128, 10000, 7, 3, 0, 1), (128, 10000, 7, 5, 0, 1), (128, 10000, 7, 1, 1, 2), (128, 10000, 7, 1, 3, 1),
            (128, 10000, 11, 1, 0, 1), (128, 10000, 11, 3, 0, 1), (128, 10000, 11, 5, 0, 1), (128, 10000, 11, 1, 1, 2), (128, 10000, 11, 1, 4, 1)]
assert sum(n for *_, n in LAUNCHES) == 18
ms = ctypes.c_float()


def bench(C, Ls, k, d, epi, iters):
    _lib.check(L.dissc_conv_bench(32, C, C, k, d, Ls, epi, iters, F54, ctypes.byref(ms)), "dissc_conv_bench")
    return ms.value * 1e3


tot = {0: 0.0, 1: 0.0}
slower = []
for C, Ls, k, d, epi, n in LAUNCHES:
    t = {0: [], 1: []}
    for blk in range(NBLK):
        for sv in (0, 1):
            _lib.set_option("wino8_sv", sv)
            assert _lib.wino8_form(C, k, d, 4, 32, Ls) == sv, (C, k, d, sv)
            bench(C, Ls, k, d, epi, 3)  # warm-up
            t[sv].append(bench(C, Ls, k, d, epi, ITERS))
    _lib.set_option("wino8_sv", 1)
    med = {sv: statistics.median(t[sv]) for sv in (0, 1)}
    for sv in (0, 1):
        tot[sv] += n * med[sv]
    if med[1] > med[0]:
        slower.append((C, k, d, epi))
    print(f"C={C} L={Ls} k={k} d={d} epi={epi} x{n} (us):  private {med[0]:6.1f} [{min(t[0]):6.1f} .. {max(t[0]):6.1f}]   "
          f"shared {med[1]:6.1f} [{min(t[1]):6.1f} .. {max(t[1]):6.1f}]   {100 * (med[1] / med[0] - 1):+5.1f} %", flush=True)
print(f"sum over the 18 launches (medians): private {tot[0]:.0f} us, shared {tot[1]:.0f} us, saving {tot[0] - tot[1]:.0f} us "
      f"({100 * (1 - tot[1] / tot[0]):.1f} %)")
print("shared slower than private on:", slower or "none")
