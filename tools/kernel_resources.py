"""Kernel resource figures of two builds side by side, from hipcc's
-Rpass-analysis=kernel-resource-usage remarks (stderr of a compile):

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off --cuda-device-only \
        -Rpass-analysis=kernel-resource-usage -c drep_amd/csrc/linkage.hip -o /dev/null 2> branch.txt
  (the same on the parent commit's sources 2> parent.txt)
  python tools/kernel_resources.py parent.txt branch.txt > profiles/linkage_ward_resources.txt

One line per kernel (demangled, template arguments kept): SGPRs, VGPRs, AGPRs,
scratch bytes per lane, LDS bytes per block, occupancy -- parent | branch --
and "same", "DIFFERS" or "new".  Exit status 1 when a kernel both builds have
differs."""
import re
import subprocess
import sys

FIELDS = (("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("LDS Size [bytes/block]", "lds"), ("Occupancy [waves/SIMD]", "occ"))


def parse(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        for key, short in FIELDS:
            m = re.search(r"remark:\s+" + re.escape(key) + r": (\d+)", line)
            if m and cur is not None:
                cur[short] = int(m.group(1))
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    d = r.stdout.splitlines() if r.returncode == 0 else list(names)
    # the kernel and its template arguments, without the parameter list
    return {n: re.sub(r"^void ", "", re.sub(r"\(.*$", "", x)) for n, x in zip(names, d)}


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    names = sorted(set(a) | set(b))
    dm = demangle(names)
    fmt = lambda r: " ".join("%s=%d" % (s, r.get(s, -1)) for _, s in FIELDS)
    differs = 0
    for n in sorted(names, key=lambda x: dm[x]):
        if n in a and n in b:
            same = a[n] == b[n]
            differs += not same
            print("%-60s %s | %s   %s" % (dm[n], fmt(a[n]), fmt(b[n]), "same" if same else "DIFFERS"))
        elif n in b:
            print("%-60s %s | %s   new" % (dm[n], "-", fmt(b[n])))
        else:
            print("%-60s %s | -   removed" % (dm[n], fmt(a[n])))
    print("# %d kernels in both builds, %d differ" % (len(set(a) & set(b)), differs))
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main())
