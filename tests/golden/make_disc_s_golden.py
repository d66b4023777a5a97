"""Writes tests/golden/disc_s.npz by running the REFERENCE's own DiscriminatorS (sr/models.py:285-307; this container only).

    python tests/golden/make_disc_s_golden.py

Imports the reference module unmodified from /root/reference (which does not exist on the GPU box -- only the .npz travels),
removes its weight norm, sets the folded weights drawn by tests/conv_grouped_ref.disc_s_weights(seed) and runs it in float64 on
a seeded waveform of 513 samples.  Stored: the score (9 values) and, of each of the eight maps AS THE REFERENCE RETURNS THEM
(leaky_relu of the first seven, conv_post's output as the eighth), the shape, the sum and the first 16 values.  Results only: no
weights, nothing of the reference's source.  tests/test_conv_grouped_cpu.py holds the project's restatement to it.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.environ.get("DISSC_GOLDEN_OUT", HERE)
sys.path.insert(0, os.path.dirname(HERE))  # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import conv_grouped_ref as R  # noqa: E402

SEEDS, T = (0, 1), 513


def wave(seed):
    return torch.from_numpy(np.random.RandomState(1000 + seed).uniform(-1, 1, (1, 1, T)))


def main():
    sys.path.insert(0, os.path.join(REF, "sr"))
    import models as ref_models  # reference sr/models.py
    out = {}
    for seed in SEEDS:
        d = ref_models.DiscriminatorS()
        w = R.disc_s_weights(seed, torch.float64)
        for name, conv in [(f"convs.{i}", c) for i, c in enumerate(d.convs)] + [("conv_post", d.conv_post)]:
            torch.nn.utils.remove_weight_norm(conv)
            assert tuple(conv.weight.shape) == tuple(w[name + ".weight"].shape), name
            conv.weight.data = w[name + ".weight"].clone()
            conv.bias.data = w[name + ".bias"].clone()
        d = d.double().eval()
        with torch.no_grad():
            score, fmap = d(wave(seed))
        out[f"s{seed}/score"] = score.numpy().reshape(-1)
        for j, m in enumerate(fmap):
            out[f"s{seed}/map{j}/shape"] = np.array(m.shape, dtype=np.int64)
            out[f"s{seed}/map{j}/sum"] = np.array([m.sum().item(), m.abs().sum().item()])
            out[f"s{seed}/map{j}/head"] = m.reshape(-1)[:16].numpy().copy()
    np.savez_compressed(os.path.join(OUT, "disc_s.npz"), **out)
    print({k: v.shape for k, v in out.items() if k.endswith("score")})


if __name__ == "__main__":
    main()
