#!/usr/bin/env python
"""Compare the device assembly of two builds of ONE source kernel by kernel, for a change that removes or adds template instances
(where the whole-file hash of profiles/r12/device_asm.md cannot be equal):
  hipcc <build flags> --cuda-device-only -S <source> -o parent.s     (on the parent)     ... -o this.s     (on this tree)
  tools/device_asm_kernels.py parent.s this.s [symbol prefix, default _ZN5dissc]
Per kernel symbol the function text (label to .Lfunc_end) and the .amdhsa_kernel descriptor, with what depends on a function's
ordinal in the file taken out (the BB<ordinal>_ of local labels, and the comments, whose column moves with the ordinal's digits).
Prints the kernels removed, added and differing and one sha256 over the surviving texts of either file; exit status 1 if a
surviving kernel differs."""
import hashlib
import re
import sys


def kernels(path, prefix):
    txt = open(path).read()
    body = {m.group(1): m.group(2) for m in re.finditer(r"^(%s\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(prefix), txt, re.S | re.M)}
    desc = {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", txt, re.S)}
    return {k: norm(v) + desc.get(k, "") for k, v in body.items() if k in desc}


def norm(body):
    return re.sub(r"[ \t]*;[^\n]*", "", re.sub(r"BB\d+_", "BB_", body))


def main():
    prefix = sys.argv[3] if len(sys.argv) > 3 else "_ZN5dissc"
    a, b = kernels(sys.argv[1], prefix), kernels(sys.argv[2], prefix)
    both = sorted(set(a) & set(b))
    print(f"{len(a)} kernels in {sys.argv[1]}, {len(b)} in {sys.argv[2]}")
    for title, names in (("removed", sorted(set(a) - set(b))), ("added", sorted(set(b) - set(a))),
                         ("differing", [k for k in both if a[k] != b[k]])):
        print(f"{title}: {len(names)}")
        for n in names:
            print("  ", n)
    for path, ks in ((sys.argv[1], a), (sys.argv[2], b)):
        print(f"sha256 over the {len(both)} surviving kernels of {path}:", hashlib.sha256("".join(k + ks[k] for k in both).encode()).hexdigest()[:16])
    return 1 if any(a[k] != b[k] for k in both) else 0


if __name__ == "__main__":
    sys.exit(main())
