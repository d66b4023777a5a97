#!/usr/bin/env python
"""ResBlock2 (HiFi-GAN V3-style configs): the one-launch block kernel (csrc/resblock2.hip) against its two direct conv launches.

    python tools/resblock2_bench.py [--blocks 7] [--iters 50] [--forward-iters 10]

Per launch: each of the six (C; k; d0, d1) instances at B = 32 x 10 s (80 000 * 32 / C columns) through dissc_resblock2_bench, the
two forms by turns, one block of `iters` launches each after a warm-up block, `blocks` times; every block is shown and the median
block reported.  The rule for the default "rb2_fused" mask: a (C, k) is in it when the one-launch median is below the two-launch
median by more than the spread (max - min) between blocks of the same form, the larger of the two forms' spreads.
Forward: the VCTK model with the three V3 blocks (tests/resblock2_cases.py) on 32 x 10 s, a handle created under "rb2_fused" = 0, one
under 63 and one under the library's default, by turns in the same way.  One process: the two forms live in one library."""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from dissc_amd import _lib  # noqa: E402

BLOCKS = [(3, 1, 2), (5, 2, 6), (7, 3, 12)]
BIT = {(32, 3): 1, (32, 5): 2, (32, 7): 4, (16, 3): 8, (16, 5): 16, (16, 7): 32}


def launch_us(C, k, d0, d1, mode, iters, epi=3):
    ms = ctypes.c_float()
    _lib.check(_lib.lib.dissc_resblock2_bench(32, C, k, d0, d1, 80000 * 32 // C, epi, iters, mode, ctypes.byref(ms)), "dissc_resblock2_bench")
    return ms.value * 1e3


def median(v):
    return sorted(v)[len(v) // 2]


def per_launch(blocks, iters):
    mask = 0
    for C in (32, 16):
        for k, d0, d1 in BLOCKS:
            us = ([], [])
            for mode in (0, 1):
                launch_us(C, k, d0, d1, mode, iters)  # warm-up block
            for _ in range(blocks):
                for mode in (0, 1):
                    us[mode].append(launch_us(C, k, d0, d1, mode, iters))
            med, spread = [median(v) for v in us], max(max(v) - min(v) for v in us)
            on = med[0] - med[1] > spread
            mask |= BIT[(C, k)] if on else 0
            print(f"RB2 C={C} k={k} d=({d0}, {d1}): two launches {' '.join(f'{v:.1f}' for v in us[0])} us, median {med[0]:.1f} | one launch "
                  f"{' '.join(f'{v:.1f}' for v in us[1])} us, median {med[1]:.1f} | {100 * (med[1] / med[0] - 1):+.1f} % | spread {spread:.1f} us | "
                  f"{'ON' if on else 'off'}", flush=True)
    print(f"RB2 rule's mask: rb2_fused = {mask}", flush=True)


def forward(blocks, iters):
    import dissc_amd
    import resblock2_cases as RB
    import synthdata as synth
    h = RB.vctk_config()
    sd = RB.state_dict(h, seed=0)
    gens = []
    was = _lib.get_option("rb2_fused")
    masks = [0, 63] + ([was] if was not in (0, 63) else [])
    for mask in masks:
        _lib.set_option("rb2_fused", mask)
        try:
            g = dissc_amd.CodeGenerator(h).to("cuda:0")
            g.load_state_dict(sd)
            gens.append(g.eval().remove_weight_norm().prepare())
        finally:
            _lib.set_option("rb2_fused", was)
    code, f0, spkr, _ = synth.synth_generator_inputs(32, 500, seed=1234)
    args = dict(code=torch.from_numpy(code).cuda(), f0=torch.from_numpy(f0).cuda(), spkr=torch.from_numpy(spkr).cuda())

    def block(g):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            y = g(**args)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters, y

    ys = [block(g)[1] for g in gens]  # warm-up block
    assert torch.equal(ys[0], ys[1]), "the two forms differ"
    assert all(torch.equal(ys[0], y) for y in ys), "the forms differ"
    ms = [[] for _ in gens]
    for _ in range(blocks):
        for i, g in enumerate(gens):
            ms[i].append(block(g)[0])
    for mask, v in zip(masks, ms):
        print(f"RB2 forward 32 x 10 s, rb2_fused = {mask:2d}{' (the default)' if mask == was else ''}: {' '.join(f'{t:.3f}' for t in v)} ms, "
              f"median {median(v):.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--forward-iters", type=int, default=10)
    a = ap.parse_args()
    per_launch(a.blocks, a.iters)
    forward(a.blocks, a.forward_iters)


if __name__ == "__main__":
    main()
