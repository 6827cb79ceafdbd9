#!/usr/bin/env python3
"""Did a source change alter the device code?  Compares two device assembly listings kernel by kernel.

Make the listings with the flags of csrc/Makefile plus `--cuda-device-only -S`:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC [-DMPN_EXPERIMENTS] --cuda-device-only -S -c conv_igemm.hip -o new.s
    python tools/isa_diff.py old.s new.s [more pairs: old2.s new2.s ...]

A kernel is everything the compiler prints for one `.amdhsa_kernel` symbol: the instruction text, the `.amdhsa_*` descriptor and the
`.set` / "Kernel info" resource lines.  Two kernels are identical when that text is equal line for line.  The only thing put aside is
the function's ordinal inside compiler-local labels (.LBB<n>_<k>, .LJTI<n>_<k>, .LCPI<n>_<k>, .Lfunc_begin<n>, .Lfunc_end<n>) and in
the loop comments that quote them ("Header=BB<n>_<k>", "Parent Loop BB<n>_<k>", "Child Loop BB<n>_<k>"): it counts the functions
printed before this one and changes for every kernel behind a removed instantiation.  A kernel that differs is reported with its size
and register figures on both sides and with every `.amdhsa_*` / `.set` line that changed.
Exit status 1 if a kernel differs or exists in one listing only."""
import re
import shutil
import subprocess
import sys

BEGIN = re.compile(r"^\s*\.globl\s+(\S+)\s*; -- Begin function")
ORDINAL = re.compile(r"(\.L(?:BB|JTI|CPI|func_begin|func_end)|(?:Header=|Parent Loop |Child Loop )BB)\d+")
RESOURCE = re.compile(r"^\s*(\.amdhsa_|\.set )")
INFO = re.compile(r"^; (codeLenInByte|TotalNumSgprs|NumVgprs|NumAgprs|ScratchSize|LDSByteSize|Occupancy)")


def kernels(path):
    """symbol -> list of lines, for every function of the listing that carries a kernel descriptor"""
    out, name, body, tail = {}, None, [], False
    def close():
        if name and any(l.lstrip().startswith(".amdhsa_kernel") for l in body):
            out[name] = body
    with open(path) as f:
        for line in f:
            line = line.rstrip("\n")
            m = BEGIN.match(line)
            if m or (tail and not line.startswith(";")):      # next function, or the end of this one's "Kernel info" comment
                close()
                name, body, tail = (m.group(1), [], False) if m else (None, [], False)
            if name is None:
                continue
            body.append(ORDINAL.sub(r"\1", line))
            if ".AMDGPU.csdata" in line:
                tail = True
    close()
    return out


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not names:
        return {n: n for n in names}
    res = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: (d.replace("(anonymous namespace)::", "") or n) for n, d in zip(names, res)}


def compare(a_path, b_path):
    a, b = kernels(a_path), kernels(b_path)
    pretty = demangle(sorted(set(a) | set(b)))
    same = [n for n in a if n in b and a[n] == b[n]]
    diff = [n for n in a if n in b and a[n] != b[n]]
    only_a, only_b = [n for n in a if n not in b], [n for n in b if n not in a]
    print("== %s  vs  %s" % (a_path, b_path))
    print("   %d kernels / %d kernels: %d identical, %d differing, %d only in the first, %d only in the second"
          % (len(a), len(b), len(same), len(diff), len(only_a), len(only_b)))
    for n in same:
        print("   identical   %s" % pretty[n])
    for n in diff:
        print("   DIFFERS     %s" % pretty[n])
        for side, k in (("first ", a[n]), ("second", b[n])):
            print("               %s %5d lines; %s" % (side, len(k), ", ".join(l[2:].split(" bytes")[0] for l in k if INFO.match(l))))
        ra, rb = [l.strip() for l in a[n] if RESOURCE.match(l)], [l.strip() for l in b[n] if RESOURCE.match(l)]
        for x, y in (zip(ra, rb) if len(ra) == len(rb) else []):
            if x != y:
                print("               %s  |  %s" % (x, y))
    for n in only_a:
        print("   only first  %s" % pretty[n])
    for n in only_b:
        print("   only second %s" % pretty[n])
    return not (diff or only_a or only_b)


def main():
    args = sys.argv[1:]
    if len(args) < 2 or len(args) % 2:
        sys.exit(__doc__)
    ok = True
    for i in range(0, len(args), 2):
        ok = compare(args[i], args[i + 1]) and ok
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
