#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two builds of kernels.hip, kernel by kernel.

A refactor of inlined device code should leave the machine code of the kernels as it was.  Produce the assembly of both
commits with the flags of mitsuba2_amd/csrc/Makefile plus `--cuda-device-only -S`:

    hipcc --offload-arch=gfx950 -std=c++17 -O3 -fPIC -fvisibility=hidden -ffp-contract=off -fno-fast-math \
          -fno-slp-vectorize -I include --cuda-device-only -S -o kernels.s mitsuba2_amd/csrc/kernels.hip

    python scripts/isa_compare.py before.s after.s [--allow SUBSTRING ...]

A kernel is its text from its label to `.end_amdhsa_kernel` (instructions and the .amdhsa_ descriptor) plus its entry in the
`amdhsa.kernels` metadata.  Local labels carry the number of the function inside the file (.LBB12_3); that number is dropped, so
that a kernel which merely moved compares equal.  Nothing else is normalised.  Exit status 0: same set of kernels, and every
kernel whose mangled name contains none of the --allow substrings is identical.
"""
import argparse
import re
import sys

LABEL = re.compile(r"\.L(BB|func_begin|func_end|tmp)\d+")
FIGURES = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def kernels(path):
    lines = open(path).read().split("\n")
    names = [l.split()[1] for l in lines if l.startswith("\t.amdhsa_kernel ")]
    start = {l.split(":")[0]: i for i, l in enumerate(lines) if l.startswith("_Z") and ":" in l}
    meta_at = lines.index("amdhsa.kernels:")
    meta = {}
    for entry in ("\n" + "\n".join(lines[meta_at + 1:])).split("\n  - ."):       # (the first entry has no line before it)
        m = re.search(r"^\s+\.name:\s+(\S+)$", entry, re.M)
        if m:
            meta[m.group(1)] = entry.split("\namdhsa.")[0]
    out = {}
    for n in names:
        end = lines.index("\t.end_amdhsa_kernel", start[n])
        text = "\n".join(LABEL.sub(lambda m: ".L" + m.group(1), l) for l in lines[start[n]:end + 1])
        figures = tuple(int(re.search(re.escape(k) + r":\s+(\d+)", meta[n]).group(1)) for k in FIGURES)
        out[n] = (text, meta[n], figures)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--allow", nargs="*", default=[], help="kernels whose name contains one of these may differ")
    args = ap.parse_args()
    a, b = kernels(args.before), kernels(args.after)
    bad = sorted(set(a) ^ set(b))
    for n in bad:
        print(f"only in {'before' if n in a else 'after'}: {n}")
    print(f"{'kernel':<100} same  vgpr        sgpr        scratch     lds")
    n_same = 0
    for n in sorted(set(a) & set(b)):
        same = a[n][:2] == b[n][:2]
        n_same += same
        if not same and not any(s in n for s in args.allow):
            bad.append(n)
        cols = "  ".join(f"{x:>4} {y:>5}" for x, y in zip(a[n][2], b[n][2]))
        print(f"{n:<100} {'yes' if same else 'NO ':<4}  {cols}")
        if not same:
            la, lb = a[n][0].split("\n"), b[n][0].split("\n")
            first = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
            print(f"    {len(la)} / {len(lb)} lines; first difference at line {first}:")
            print(f"    - {la[first].strip() if first < len(la) else '<end>'}\n    + {lb[first].strip() if first < len(lb) else '<end>'}")
    print(f"{len(a)} / {len(b)} kernels, {n_same} identical, {len(bad)} not accepted")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
