"""Per-phase VALU budget of the sketch hash kernel's hot loop, from the ISA
(not product code).  Compiles drep_amd/csrc/sketch.hip for gfx950 with line
tables (-gline-tables-only: the same code, plus .loc directives), walks the
k_sketch_hash21<64,2> body and attributes every instruction of the unrolled
hash blocks to the source function its .loc names -- the k-mer cut and
canonical select, the table addressing, MurmurHash3's body, fmix64, the
prefilter -- or to the loop (code-word sliding, validity, branches).  The
rare admit branch (murmur_fin, the exact test, the staging) is listed apart.
usage: [EXTRA=<hipcc flags of an A/B build>] python tools/isa_phases.py > profiles/r05_sketch_isa_phases.json"""
import collections
import json
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "drep_amd/csrc/sketch.hip")
HDR = os.path.join(ROOT, "drep_amd/csrc/prefilter.h")      # fmix64's tail and the prefilter (host + device)
CANON = os.path.join(ROOT, "drep_amd/csrc/canon.h")         # the strand choice and the tail cut (host + device)
CANON_BASE = 100000                                         # canon.h line n is carried as -(CANON_BASE + n)


PREFILTER = "prefilter (sum, one high word, compare)"


def func_ranges(lines, hlines, clines):
    """(first, last) source lines of the functions and regions the phases name
    (sketch.hip; negative line numbers: prefilter.h, below -CANON_BASE: canon.h)."""
    def find(pat, start=0):
        for i in range(start, len(lines)):
            if re.search(pat, lines[i]):
                return i + 1
        raise KeyError(pat)

    def body(pat):                       # a function: from its header to the closing brace at column 0
        a = find(pat)
        b = next(i + 1 for i in range(a, len(lines)) if lines[i].startswith("}"))
        return a, b
    r = {}
    r["k-mer cut + canonical select"] = [(find(r"auto canon = \["), find(r"auto canon = \[")),
                                         (-(CANON_BASE + len(clines)), -(CANON_BASE + 1))]
    r["table addressing + LDS reads"] = body(r"MEnt fetch_ent\(")
    r["Murmur body (tables combined)"] = body(r"void murmur21_ent\(")
    r["Murmur helpers (rotl, *5+c, add64, mad64)"] = None   # several functions, below
    def hbody(pat):                      # a function of prefilter.h, as negated line numbers
        a = next(i + 1 for i in range(len(hlines)) if re.search(pat, hlines[i]))
        b = next(i + 1 for i in range(a, len(hlines)) if hlines[i].startswith("}"))
        return -b, -a
    r["fmix64 to the last multiply"] = hbody(r"uint64_t fmix64_q\(")
    r[PREFILTER] = [hbody(p) for p in (r"uint32_t prefilter_hi\(", r"uint32_t mulhi32\(")]
    r["admit branch (rare)"] = (find(r"if \(__builtin_expect\(hit, 0\)\)"), find(r"// slide one code word") - 1)
    helpers = [body(p) for p in (r"uint64_t rotl64_ab\(", r"uint64_t x5_plus\(", r"uint64_t add64\(",
                                 r"uint64_t mad64\(")]
    r["Murmur helpers (rotl, *5+c, add64, mad64)"] = helpers
    r["murmur_fin (admit branch)"] = [hbody(r"uint64_t murmur_fin\("), hbody(r"uint64_t fmix_mul\(")]
    return r


def main():
    lines = open(SRC).read().split("\n")
    ranges = func_ranges(lines, open(HDR).read().split("\n"), open(CANON).read().split("\n"))
    hit_lines = [i + 1 for i, l in enumerate(lines) if "pf[b] = prefilter_hi" in l or "hit |= pf[b]" in l]

    def phase_of(line):
        if line in hit_lines:
            return PREFILTER
        for name, rg in ranges.items():
            for a, b in (rg if isinstance(rg, list) else [rg]):
                if a <= line <= b:
                    return name
        return "loop: code words, validity, control"
    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, "sk.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-gline-tables-only",
                        "--cuda-device-only", "-S", "-o", asm, SRC, "-I" + os.path.join(ROOT, "drep_amd/csrc")] +
                       os.environ.get("EXTRA", "").split(), check=True, stderr=subprocess.DEVNULL)
        s = open(asm).read()
    fileno = hdrno = canno = None
    for m in re.finditer(r'^\s*\.file\s+(\d+)\s+"[^"]*"\s+"([^"]*)"', s, re.M):
        if m.group(2).endswith("sketch.hip"):
            fileno = m.group(1)
        if m.group(2).endswith("prefilter.h"):
            hdrno = m.group(1)
        if m.group(2).endswith("canon.h"):
            canno = m.group(1)
    m = re.search(r"^(_ZN7drephip\d+k_sketch_hash21ILi64ELi2E\S*):", s, re.M)
    body = s[m.start():s.index(".Lfunc_end", m.start())]
    # blocks between labels; the hot ones hold the hash (2 k-mers' mad_u64 chains)
    blocks, cur, loc = [], None, 0
    for ln in body.split("\n"):
        t = ln.strip()
        if re.match(r"^\.LBB\S+:", ln):
            cur = []
            blocks.append(cur)
            continue
        lm = re.match(r"\.loc\s+(\d+)\s+(\d+)", t)
        if lm:
            n = int(lm.group(2))
            loc = n if lm.group(1) == fileno else -n if lm.group(1) == hdrno else -(CANON_BASE + n) if lm.group(1) == canno else 0
            continue
        if cur is None or not ln.startswith("\t") or t.startswith((".", ";")) or not t:
            continue
        cur.append((t.split()[0], loc))
    hot = [b for b in blocks if sum(1 for op, _ in b if op == "v_mad_u64_u32") >= 8]
    kmers = 2 * len(hot)
    per = collections.defaultdict(collections.Counter)
    for b in hot:
        for op, line in b:
            if op.startswith("v_"):
                per[phase_of(line)][op] += 1
    total = sum(sum(c.values()) for c in per.values())
    out = {"kernel": "k_sketch_hash21<64,2>", "source": "drep_amd/csrc/sketch.hip", "hot_blocks": len(hot),
           "kmers_in_hot_blocks": kmers, "valu_per_kmer": round(total / kmers, 3), "phases": {}}
    for name, c in sorted(per.items(), key=lambda kv: -sum(kv[1].values())):
        n = sum(c.values())
        out["phases"][name] = {"valu_per_kmer": round(n / kmers, 3), "share": round(n / total, 3),
                               "mix_per_kmer": {k: round(v / kmers, 3) for k, v in c.most_common()}}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
