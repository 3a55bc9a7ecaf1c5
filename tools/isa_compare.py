"""Kernel-by-kernel comparison of two sets of gfx950 assembly listings (hipcc --cuda-device-only -S of the same .hip files
at two commits): per mangled kernel name, the instruction text with labels, comments and symbol names stripped, and the
register / scratch / LDS figures of the kernel's metadata.  A plain comparison: it says which kernels changed, nothing more.

    python tools/isa_compare.py PARENT_DIR NEW_DIR file1.s [file2.s ...]

--by-text: for a change that renames kernels or moves them between files.  The files named are looked for in both
directories (one that exists on one side only is fine) and the kernels of each side are taken together:
  1. a new kernel is paired with a parent kernel of equal normalised text and equal metadata (as multisets);
  2. of the rest, kernels pair whose metadata, instruction count and sequence of mnemonics are equal: "operands" pairs, the
     same instructions on other registers, offsets or immediates -- both names are printed;
  3. what is left on either side is listed.
Exit status 0 only if nothing is left.

    python tools/isa_compare.py --by-text PARENT_DIR NEW_DIR file1.s [file2.s ...]
"""
import hashlib
import os
import re
import sys
from collections import defaultdict

FIELDS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def listing(path):
    """{mangled name: (normalised instruction lines, {metadata field: value})}"""
    text = open(path).read()
    meta = {}
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {f: int(re.search(re.escape(f) + r":\s+(\d+)", block).group(1)) for f in FIELDS}
    out = {}
    for name in meta:
        m = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end" % re.escape(name), text, re.S | re.M)
        lines = []
        for ln in m.group(1).split("\n"):
            ln = ln.split(";")[0].split("//")[0].strip()
            if not ln or ln.endswith(":") or ln.startswith("."):
                continue
            ln = re.sub(r"\.?L?[A-Za-z_$][\w$.]*@(rel32@(lo|hi)|gotpcrel32@(lo|hi))\+?\d*", "SYM", ln)  # symbol references
            ln = re.sub(r"\.LBB\d+_\d+", "LBB", ln)                                                    # branch targets
            lines.append(ln)
        out[name] = (lines, meta[name])
    return out


def sha1(lines):
    return hashlib.sha1("\n".join(lines).encode()).hexdigest()


def kernels(path):
    """{mangled name: (sha1 of the normalised instruction text, number of instructions, {metadata field: value})}"""
    return {name: (sha1(lines), len(lines), meta) for name, (lines, meta) in listing(path).items()}


def by_text(parent_dir, new_dir, files):
    def side(d):
        """[(file, name, lines, metadata figures)] of every kernel of the files that exist under d"""
        out = []
        for f in files:
            if os.path.exists("%s/%s" % (d, f)):
                out += [(f, name, lines, [meta[k] for k in FIELDS]) for name, (lines, meta) in sorted(listing("%s/%s" % (d, f)).items())]
        return out

    def pair(left, right, key):
        """pairs of left and right entries with equal key, each entry used once; and what stays of either"""
        pool = defaultdict(list)
        for e in left:
            pool[key(e)].append(e)
        pairs, rest_r = [], []
        for e in right:
            same = pool.get(key(e))
            if same:
                pairs.append((same.pop(0), e))
            else:
                rest_r.append(e)
        return pairs, [e for es in pool.values() for e in es], rest_r

    a, b = side(parent_dir), side(new_dir)
    print("%d kernels in the parent's files, %d in the new ones" % (len(a), len(b)))
    print("%-10s kernel  [vgpr sgpr scratch lds | instructions]  <- parent kernel" % "text")
    same, a, b = pair(a, b, lambda e: (sha1(e[2]), tuple(e[3])))
    ops, a, b = pair(a, b, lambda e: (tuple(e[3]), len(e[2]), tuple(ln.split()[0] for ln in e[2])))
    for word, pairs in (("identical", same), ("operands", ops)):
        for (fa, na, la, ma), (fb, nb, lb, mb) in pairs:
            print("%-10s %s:%s  %s | %d  <- %s:%s" % (word, fb, nb, mb, len(lb), fa, na))
    for word, rest in (("PARENT ONLY", a), ("NEW ONLY", b)):
        for f, name, lines, m in rest:
            print("%-10s %s:%s  %s | %d" % (word, f, name, m, len(lines)))
    print("%d pairs identical, %d pairs differ in operands only, %d parent and %d new kernels unpaired" % (len(same), len(ops), len(a), len(b)))
    return 0 if not a and not b else 1


def main():
    if sys.argv[1] == "--by-text":
        return by_text(sys.argv[2], sys.argv[3], sys.argv[4:])
    parent_dir, new_dir, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    print("%-12s %-9s %s" % ("file", "text", "kernel  [vgpr sgpr scratch lds | instructions]  (parent -> new where they differ)"))
    n_same = n_diff = 0
    ok = True
    for f in files:
        a, b = kernels("%s/%s" % (parent_dir, f)), kernels("%s/%s" % (new_dir, f))
        if set(a) != set(b):
            ok = False
            print("%-12s SYMBOLS   only in parent: %s; only in new: %s" % (f, sorted(set(a) - set(b)), sorted(set(b) - set(a))))
        for name in sorted(set(a) & set(b)):
            (ha, na, ma), (hb, nb, mb) = a[name], b[name]
            fa, fb = [ma[k] for k in FIELDS], [mb[k] for k in FIELDS]
            same = ha == hb and fa == fb
            n_same += same
            n_diff += not same
            if not same and (mb[".vgpr_count"] > ma[".vgpr_count"] or mb[".private_segment_fixed_size"] > ma[".private_segment_fixed_size"]):
                ok = False
            fig = "%s | %d" % (fa, na) if same else "%s | %d -> %s | %d" % (fa, na, fb, nb)
            print("%-12s %-9s %s  %s" % (f, "identical" if same else "DIFFERS", name, fig))
    print("%d kernels identical, %d differ; symbols equal and no VGPR / scratch growth: %s" % (n_same, n_diff, "yes" if ok else "NO"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
