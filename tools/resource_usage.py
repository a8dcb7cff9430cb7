#!/usr/bin/env python3
"""Registers, scratch and LDS of template kernels from gfx950 device assembly (hipcc ... --cuda-device-only -S),
the instantiations with one template argument at value A beside their siblings with it at value B.

usage: tools/resource_usage.py FILE.s [FILE.s ...] --arg INDEX --a A --b B
       tools/resource_usage.py PARENT.s [PARENT.s ...] --against NEW.s [NEW.s ...]

Per pair one line: the other template arguments, then SGPRs, VGPRs, scratch bytes, static LDS bytes and waves
per SIMD of the A instantiation and of its B sibling (the "; Kernel info:" block the compiler writes after
each kernel).  The last line counts the A instantiations with scratch whose B sibling has none; exit status 1
if there is one.  (The marches' LDS is dynamic -- sized by the host per launch -- so the static figure is 0.)

--against: two builds of the same files instead, each kernel of PARENT.s beside the kernel of the same name and
template arguments in NEW.s.  The last line counts the kernels with fewer, as many and more waves per SIMD than
their parent; exit status 1 if a kernel has no partner, one has fewer waves, or one uses scratch.
"""
import argparse
import re
import sys

NAME = re.compile(r"^_ZN2vr\d+([a-z0-9_]+?)I((?:L[bi]\d+E)+)E")
FIELDS = ("TotalNumSgprs", "NumVgprs", "ScratchSize", "LDSByteSize", "Occupancy")


def kernels(path):
    """{(kernel, template arguments): {field: value}} of the file's template kernels."""
    out, cur = {}, None
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            n = NAME.match(m.group(1))
            cur = (n.group(1), tuple(int(a) for a in re.findall(r"L[bi](\d+)E", n.group(2)))) if n else None
            if cur:
                out.setdefault(cur, {})
            continue
        m = re.match(r"^; (\w+):\s*(\d+)", ln)
        if cur and m and m.group(1) in FIELDS and m.group(1) not in out[cur]:
            out[cur][m.group(1)] = int(m.group(2))
    return {k: v for k, v in out.items() if len(v) == len(FIELDS)}


def against(parents, news):
    lower = equal = higher = bad = 0
    row = "%5d %5d %7d %3d %10d"
    for pa, pb in zip(parents, news):
        A, B = kernels(pa), kernels(pb)
        print("%s | %s" % (pa, pb))
        print("kernel <template arguments> | parent: SGPRs VGPRs scratch LDS waves/SIMD | new: the same | waves")
        for k in sorted(A):
            a, b = A[k], B.get(k)
            name = "%s<%s>" % (k[0], ", ".join(map(str, k[1])))
            if b is None:
                print("%-40s | %s | (no partner)" % (name, row % tuple(a[f] for f in FIELDS)))
                bad += 1
                continue
            d = b["Occupancy"] - a["Occupancy"]
            lower, equal, higher = lower + (d < 0), equal + (d == 0), higher + (d > 0)
            bad += b["ScratchSize"] > 0
            print("%-40s | %s | %s | %s" % (name, row % tuple(a[f] for f in FIELDS), row % tuple(b[f] for f in FIELDS),
                                           "lower" if d < 0 else "higher" if d > 0 else "equal"))
        bad += len(set(B) - set(A))
        print()
    print("%d kernels: %d with fewer waves per SIMD than their parent, %d with as many, %d with more; "
          "%d without a partner or with scratch" % (lower + equal + higher, lower, equal, higher, bad))
    return 1 if lower or bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("files", nargs="+")
    ap.add_argument("--against", nargs="+", help="the same files of another build, in the same order")
    ap.add_argument("--arg", type=int, help="index of the template argument that differs")
    ap.add_argument("--a", type=int)
    ap.add_argument("--b", type=int)
    o = ap.parse_args()
    if o.against:
        if len(o.against) != len(o.files):
            ap.error("--against takes as many files as there are ahead of it (%d)" % len(o.files))
        return against(o.files, o.against)
    if o.arg is None or o.a is None or o.b is None:
        ap.error("give --arg, --a and --b, or --against")
    worse = total = 0
    for path in o.files:
        K = kernels(path)
        names = sorted({k[0] for k in K})
        for name in names:
            rows = sorted((k for k in K if k[0] == name and len(k[1]) > o.arg and k[1][o.arg] == o.a), reverse=True)
            if not rows:
                continue
            print("%s, template argument %d = %d beside = %d" % (name, o.arg, o.a, o.b))
            print("other arguments | SGPRs VGPRs scratch LDS waves/SIMD | SGPRs VGPRs scratch LDS waves/SIMD")
            for k in rows:
                sib = (name, k[1][:o.arg] + (o.b,) + k[1][o.arg + 1:])
                a, b = K[k], K.get(sib)
                rest = " ".join(str(v) for i, v in enumerate(k[1]) if i != o.arg)
                fa = "%5d %5d %7d %3d %10d" % tuple(a[f] for f in FIELDS)
                fb = "%5d %5d %7d %3d %10d" % tuple(b[f] for f in FIELDS) if b else "(no sibling)"
                print("%-15s | %s | %s" % (rest, fa, fb))
                total += 1
                if b and a["ScratchSize"] > 0 and b["ScratchSize"] == 0:
                    worse += 1
            print()
    print("%d instantiations with argument %d = %d; %d use scratch where the sibling with %d uses none"
          % (total, o.arg, o.a, worse, o.b))
    return 1 if worse else 0


if __name__ == "__main__":
    sys.exit(main())
