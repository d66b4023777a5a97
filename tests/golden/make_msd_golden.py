"""Writes tests/golden/msd.npz by running the REFERENCE's own MultiScaleDiscriminator (sr/models.py:310-333).

    DISSC_REFERENCE=<checkout of the reference> python tests/golden/make_msd_golden.py

Imports the reference module unmodified (only the .npz travels with the repository), loads the state dict drawn by
tests/msd_cases.msd_state_dict(seed) -- unit-norm seeded weight_u / weight_v included --, keeps it in train() mode in float64 and
runs it TWICE on a seeded y, y_hat of 1 030 samples, B = 1: every forward runs two power iterations on discriminator 0, one in
d(y) and one in d(y_hat).  Stored after each forward: per scale the two scores and, of every map AS THE REFERENCE RETURNS IT
(leaky_relu of the first seven, conv_post's output as the eighth), the shape, the sum, the absolute sum and the first 16 values;
discriminator 0's weight_u and weight_v (whole in float32; their sum, absolute sum and first 16 values in float64) and
u . (W v) per layer.  Results only: no weights, nothing of the reference's source.
tests/test_msd_cpu.py holds the project's restatement to it.
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.environ.get("DISSC_GOLDEN_OUT", HERE)
sys.path.insert(0, os.path.dirname(HERE))  # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import msd_cases as M  # noqa: E402

SEED, T, FORWARDS = 0, 1030, 2


def waves():
    rs = np.random.RandomState(1000 + SEED)
    return tuple(torch.from_numpy(rs.uniform(-1, 1, (1, 1, T))) for _ in range(2))


def main():
    ref = os.environ.get("DISSC_REFERENCE")
    if not ref or not os.path.isdir(os.path.join(ref, "sr")):
        sys.exit("set DISSC_REFERENCE to a checkout of the reference (the directory that holds sr/models.py)")
    sys.path.insert(0, os.path.join(ref, "sr"))
    import models as ref_models  # reference sr/models.py
    d = ref_models.MultiScaleDiscriminator().double()
    d.load_state_dict({k: v.double() for k, v in M.msd_state_dict(SEED).items()}, strict=True)
    d.train()
    y, y_hat = waves()
    out = {}
    for f in range(FORWARDS):
        with torch.no_grad():
            y_d_rs, y_d_gs, fmap_rs, fmap_gs = d(y, y_hat)
        for i in range(3):
            for half, score, fmap in (("r", y_d_rs[i], fmap_rs[i]), ("g", y_d_gs[i], fmap_gs[i])):
                pre = f"f{f}/d{i}/{half}"
                out[pre + "/score"] = score.numpy().reshape(-1).copy()
                for j, m in enumerate(fmap):
                    out[f"{pre}/map{j}/shape"] = np.array(m.shape, dtype=np.int64)
                    out[f"{pre}/map{j}/sum"] = np.array([m.sum().item(), m.abs().sum().item()])
                    out[f"{pre}/map{j}/head"] = m.reshape(-1)[:16].numpy().copy()
        d0 = d.discriminators[0]
        for name, conv in [(f"convs.{j}", c) for j, c in enumerate(d0.convs)] + [("conv_post", d0.conv_post)]:
            w = conv.weight_orig.detach().reshape(conv.weight_orig.shape[0], -1)
            for what in ("weight_u", "weight_v"):  # whole in float32 (the file's size), a digest in float64
                t = getattr(conv, what).detach()
                out[f"f{f}/{name}/{what}"] = t.numpy().astype(np.float32)
                out[f"f{f}/{name}/{what}/sum"] = np.array([t.sum().item(), t.abs().sum().item()])
                out[f"f{f}/{name}/{what}/head"] = t[:16].numpy().copy()
            out[f"f{f}/{name}/sigma"] = np.array([torch.dot(conv.weight_u, torch.mv(w, conv.weight_v)).item()])
    # fixed member order and timestamps: the same bytes from every run
    path = os.path.join(OUT, "msd.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    print(path, os.path.getsize(path), "bytes;", {k: v for k, v in out.items() if k.endswith("sigma") and k.startswith("f1")})


if __name__ == "__main__":
    main()
