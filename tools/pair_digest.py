#!/usr/bin/env python
"""One sha256 per case of dissc_respair1d's output, for comparing two builds of the library bit for bit (run once per build in
separate processes, DISSC_HIP_LIB naming the other build, and diff the two outputs):
  mode 1 (the direct pairs) for C in {16, 32}, k in {3, 7, 11}, d in {1, 3, 5};
  mode 3 (the register-only pairs) under pair_tc6 = 3 and 0 for every shape with an instance in the default build;
each in the epilogue modes 1-4, on the ragged lengths of tests/test_gpu_pairs_f23.py with NaN beyond every utterance.  The digest
covers the whole output buffer, the untouched samples beyond each utterance included."""
import ctypes
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dissc_amd._lib import lib, check  # noqa: E402

DEV = "cuda:0"
LENGTHS = [2000, 1, 7, 255, 467, 468, 469, 491, 492, 493, 499, 500, 501, 507, 508, 509, 1023, 1999, 12]
LD = 2000


def digest(mode, C, k, d, epi):
    g = torch.Generator().manual_seed(1000 * C + 10 * k + d)
    x = (torch.rand(len(LENGTHS), C, LD, generator=g) * 2 - 1).to(DEV)
    for i, n in enumerate(LENGTHS):
        x[i, :, n:] = float("nan")
    sc = 0.9 / (C * k) ** 0.5
    w1, w2 = ((torch.rand(C, C, k, generator=g) * 2 - 1) * sc for _ in range(2))
    b1, b2 = ((torch.rand(C, generator=g) * 2 - 1) * 0.1 for _ in range(2))
    y = torch.full_like(x, -7.0)
    acc = torch.rand(len(LENGTHS), C, LD, generator=g).to(DEV)
    ln = torch.tensor(LENGTHS, dtype=torch.int32, device=DEV)
    check(lib.dissc_respair1d(x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), y.data_ptr(), acc.data_ptr(),
                              ln.data_ptr(), len(LENGTHS), C, k, d, LD, max(LENGTHS), ctypes.c_float(0.1), epi, ctypes.c_float(3.0),
                              mode, None), f"dissc_respair1d mode {mode} C={C} k={k} d={d} epi={epi}")
    out = y if epi == 1 else acc
    return hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()


def main():
    cases = [(1, 3, C, k) for C in (16, 32) for k in (3, 7, 11)]          # (mode, pair_tc6 (mode 3 only), C, k)
    cases += [(3, 3, 32, 7), (3, 3, 32, 11), (3, 3, 16, 11), (3, 0, 32, 11), (3, 0, 16, 11)]
    assert lib.dissc_set_option(b"pair_f23", 3) == 0
    for mode, tc6, C, k in cases:
        assert lib.dissc_set_option(b"pair_tc6", tc6) == 0
        for d in (1, 3, 5):
            for epi in (1, 2, 3, 4):
                form = "direct" if mode == 1 else f"register-only pair_tc6={tc6}"
                print(f"{form} C={C} k={k} d={d} epi={epi} {digest(mode, C, k, d, epi)}", flush=True)


if __name__ == "__main__":
    main()
