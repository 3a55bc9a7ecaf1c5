"""Kernel-by-kernel comparison of two sets of gfx950 assembly listings (hipcc --cuda-device-only -S of the same .hip files
at two commits): per mangled kernel name, the instruction text with labels, comments and symbol names stripped, and the
register / scratch / LDS figures of the kernel's metadata.  A plain comparison: it says which kernels changed, nothing more.

    python tools/isa_compare.py PARENT_DIR NEW_DIR file1.s [file2.s ...]
"""
import hashlib
import re
import sys

FIELDS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def kernels(path):
    """{mangled name: (sha1 of the normalised instruction text, number of instructions, {metadata field: value})}"""
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
        out[name] = (hashlib.sha1("\n".join(lines).encode()).hexdigest(), len(lines), meta[name])
    return out


def main():
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
