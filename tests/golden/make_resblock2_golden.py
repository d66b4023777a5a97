#!/usr/bin/env python3
"""Generates tests/golden/gen_resblock2.npz from the REFERENCE implementation, in the style of make_golden.py.

    python tests/golden/make_resblock2_golden.py

Imports the reference's sr/models.py unmodified from /root/reference (which does not exist on the GPU machine) and builds its
CodeGenerator for the VCTK config with ``"resblock": "2"`` and the three HiFi-GAN V3 blocks (tests/resblock2_cases.py).  The
seeded state dict of that helper is loaded with strict ``load_state_dict`` (which pins our ResBlock2 key layout against the
reference's), and only data is stored: the reference's named_parameters() order, its waveforms at T = 1, 2, 7, 33, 99 and of the
ragged batch (one utterance per call: the reference never batches), and at T = 7 every block's output on the columns
resblock2_cases.edge_cols names.  Nothing of the reference's source is stored."""
import os
import sys
import warnings

import numpy as np
import torch

warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
OUT = os.environ.get("DISSC_GOLDEN_OUT", HERE)
os.makedirs(OUT, exist_ok=True)
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import resblock2_cases as RB  # noqa: E402
import synthdata as synth  # noqa: E402


def main():
    sys.path.insert(0, os.path.join(REF, "sr"))
    import models as ref_models  # reference sr/models.py
    import utils as ref_utils  # reference sr/utils.py
    h = ref_utils.AttrDict(RB.vctk_config())
    g = ref_models.CodeGenerator(h)
    out = {"param_order": np.array([k for k, _ in g.named_parameters()])}
    g.load_state_dict(RB.state_dict(h, seed=0), strict=True)
    g.eval()
    g.remove_weight_norm()

    def run(code, f0, spkr, want_taps):
        taps, hooks = {}, []
        if want_taps:
            for j, rb in enumerate(g.resblocks):
                hooks.append(rb.register_forward_hook(lambda m, i_, o, j=j: taps.__setitem__(f"rb{j}", o.clone())))
        with torch.no_grad():
            y = g(code=torch.from_numpy(code), f0=torch.from_numpy(f0), spkr=torch.from_numpy(spkr))
        for hk in hooks:
            hk.remove()
        return y, taps

    peak = 0.0
    for T in RB.GOLDEN_T:
        code, f0, spkr, _ = synth.synth_generator_inputs(1, T, seed=100 + T)
        y, taps = run(code, f0, spkr, want_taps=(T == 7))
        out[f"T{T}/wav"] = y.numpy()
        peak = max(peak, float(y.abs().max()))
        for k, v in taps.items():  # block outputs on their edge columns
            out[f"T{T}/{k}"] = v.numpy()[:, :, RB.edge_cols(v.shape[2])]
    code, f0, spkr, _ = synth.synth_generator_inputs(4, 40, seed=777)
    for b, n in enumerate(RB.RAGGED_LENGTHS):
        y, _ = run(code[b:b + 1, :n], f0[b:b + 1, :, :n], spkr[b:b + 1], False)
        out[f"ragged/wav{b}"] = y.numpy()
        peak = max(peak, float(y.abs().max()))
    out["ragged/lengths"] = np.array(RB.RAGGED_LENGTHS, dtype=np.int32)
    print(f"max |wav| = {peak:.4f} (gain {RB.RB2_GAIN})")
    assert peak < 0.99, "the reference's own waveform saturates tanh: lower resblock2_cases.RB2_GAIN"
    path = os.path.join(OUT, "gen_resblock2.npz")
    np.savez_compressed(path, **out)
    print("gen_resblock2.npz", len(out), "arrays,", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1 << 20


if __name__ == "__main__":
    main()
