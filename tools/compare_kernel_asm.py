#!/usr/bin/env python3
"""Compare the kernels of two device-assembly files of one source, e.g.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S x.hip -o x.s

    tools/compare_kernel_asm.py parent.s branch.s [--subset]

Per kernel (an .amdhsa_kernel block): the descriptor block (registers,
scratch, LDS, ...) and the function's text from its label to its end label
must be equal, after normalising what moves when other kernels come or go:
the function index in local labels (.LBB<n>_, .Lfunc_end<n>, and the like)
and the per-compilation __hip_cuid_ symbol.  --subset: the second file may
lack kernels of the first (they are listed); otherwise the sets must match.
Exit status 0 when everything present in both is equal and the sets agree."""
import re
import subprocess
import sys


def kernels(path):
    """{mangled name: (normalised body lines, descriptor lines)}"""
    lines = open(path).read().split("\n")
    out = {}
    for i, ln in enumerate(lines):
        m = re.match(r"\s+\.amdhsa_kernel\s+(\S+)", ln)
        if not m:
            continue
        name = m.group(1)
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        desc = [l.strip() for l in lines[i + 1:end]]
        start = max(j for j in range(i) if lines[j].startswith(name + ":"))
        stop = next(j for j in range(start, i) if lines[j].lstrip().startswith(".section"))
        out[name] = ([norm(l) for l in lines[start + 1:stop]], desc)
    return out


def norm(line):
    line = re.sub(r"\.L([A-Za-z_]+?)\d+(_|\b)", r".L\1\2", line)     # .LBB12_3 -> .LBB_3, .Lfunc_end12 -> .Lfunc_end
    line = re.sub(r"\bBB\d+_(\d)", r"BB_\1", line)                   # the same index in loop comments
    line = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", line)
    return re.sub(r"\s+", " ", line).strip()                          # (comment columns move with the index's width)


def demangle(names):
    names = sorted(names)
    if not names:
        return {}
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True)
            return dict(zip(names, r.stdout.split("\n")))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    subset = "--subset" in sys.argv
    if len(args) != 2:
        sys.exit(__doc__)
    a, b = kernels(args[0]), kernels(args[1])
    dm = demangle(set(a) | set(b))
    bad = 0
    for n in sorted(set(b) - set(a)):
        print("only in %s: %s" % (args[1], dm[n]))
        bad += 1
    gone = sorted(set(a) - set(b), key=lambda n: dm[n])
    for n in gone:
        print("only in %s: %s" % (args[0], dm[n]))
    if gone and not subset:
        bad += len(gone)
    same = 0
    for n in sorted(set(a) & set(b)):
        if a[n][1] != b[n][1]:
            print("descriptor differs: %s" % dm[n])
            bad += 1
        elif a[n][0] != b[n][0]:
            k = next((i for i, (x, y) in enumerate(zip(a[n][0], b[n][0])) if x != y), min(len(a[n][0]), len(b[n][0])))
            print("text differs at line %d of the function: %s" % (k, dm[n]))
            bad += 1
        else:
            same += 1
    print("%d kernels in %s, %d in %s: %d in both and equal, %d missing from the second, %d problems"
          % (len(a), args[0], len(b), args[1], same, len(gone), bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
