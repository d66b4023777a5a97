#!/usr/bin/env python
"""Per layer class: fp32 against split-bf16 encoder kernels, from two rocprofv3 --kernel-trace captures of
    DISSC_OPTIONS=multistream=0,hubert_split=0 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- \\
        python tools/encode_bench.py --iters 5 --precision {fp32,split_bf16}
(32 x 10 s: 57 launches per forward, in the order of hubert_forward_part).
    python tools/enc_split_table.py <fp32 dir> <split dir> [forwards averaged, default 5]
Prints a markdown table: fp32 us, split us, speed-up, executed bf16 TFLOP/s (3 products per algorithmic one), the matrix-pipe
floor (3 x GFLOP at 2.5 PFLOP/s dense bf16) and the HBM floor (algorithmic bytes at 6.3 TB/s achievable) of the split kernel."""
import csv
import glob
import sys

PER_FWD = 57
B, T = 32, 499
# frames after conv0..conv6 of 160 000 samples
LENS = [31999, 15999, 7999, 3999, 1999, 999, 499]


def conv(l, k):  # feature conv l (1-based): 512 -> 512, k taps, stride 2
    gflop = 2.0 * 512 * 512 * k * LENS[l] * B / 1e9
    gb = 4.0 * B * 512 * (LENS[l - 1] + LENS[l]) / 1e9 + 4.0 * 512 * 512 * k / 1e9
    return gflop, gb


def lin(K, M, res=False):
    gflop = 2.0 * K * M * T * B / 1e9
    gb = 4.0 * B * T * (K + M * (2 if res else 1)) / 1e9 + 4.0 * K * M / 1e9
    return gflop, gb


# dispatch index within a forward -> (class, (GFLOP, algorithmic GB))
IDX = {4: ("conv1", conv(1, 3)), 5: ("conv2", conv(2, 3)), 6: ("conv3", conv(3, 3)), 7: ("conv4", conv(4, 3)),
       8: ("conv5", conv(5, 2)), 9: ("conv6", conv(6, 2)), 11: ("proj", lin(512, 768))}
for i in range(6):
    o = 14 + 7 * i
    IDX[o] = ("qkv", lin(768, 2304))
    IDX[o + 2] = ("out_proj", lin(768, 768, True))
    IDX[o + 4] = ("fc1", lin(768, 3072))
    IDX[o + 5] = ("fc2", lin(3072, 768, True))


def per_index(d, nf):
    f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = sorted((r for r in csv.DictReader(open(f)) if "dissc::" in r["Kernel_Name"]),  # (not torch's fills and copies)
                  key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) % PER_FWD == 0, (len(rows), "launches: not a multiple of %d" % PER_FWD)
    rows = rows[-nf * PER_FWD:]
    us = [0.0] * PER_FWD
    names = [""] * PER_FWD
    for i, r in enumerate(rows):
        us[i % PER_FWD] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 / nf
        names[i % PER_FWD] = r["Kernel_Name"]
    return us, names


def main():
    nf = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    (u0, n0), (u1, n1) = per_index(sys.argv[1], nf), per_index(sys.argv[2], nf)
    order, acc = [], {}
    for i in sorted(IDX):
        cls, (gf, gb) = IDX[i]
        if cls not in acc:
            order.append(cls)
            acc[cls] = [0, 0.0, 0.0, 0.0, 0.0, n0[i], n1[i]]
        a = acc[cls]
        a[0] += 1
        a[1] += u0[i]
        a[2] += u1[i]
        a[3] += gf
        a[4] += gb
    print("| class | launches | fp32 us | split us | speed-up | executed bf16 TFLOP/s | matrix-pipe floor us | HBM floor us | binds |"
          " fp32 kernel | split kernel |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for cls in order:
        n, a0, a1, gf, gb, k0, k1 = acc[cls]
        mp, hbm = 3 * gf / 2500.0 * 1e3, gb / 6.3 * 1e3
        print("| %s | %d | %.0f | %.0f | %.2f | %.0f | %.0f | %.0f | %s | %s | %s |" % (
            cls, n, a0, a1, a0 / a1, 3 * gf / a1 * 1e3, mp, hbm, "matrix pipe" if mp >= hbm else "HBM",
            k0.split("(")[0][:48], k1.split("(")[0][:48]))
    rest0 = sum(u for i, u in enumerate(u0) if i not in IDX)
    rest1 = sum(u for i, u in enumerate(u1) if i not in IDX)
    print("\nsum of kernel times per forward: fp32 %.2f ms, split %.2f ms; layers fp32 in both modes: %.2f / %.2f ms"
          % (sum(u0) / 1e3, sum(u1) / 1e3, rest0 / 1e3, rest1 / 1e3))


if __name__ == "__main__":
    main()
