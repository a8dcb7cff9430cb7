#!/usr/bin/env python3
"""Registers, scratch and LDS of template kernels from gfx950 device assembly (hipcc ... --cuda-device-only -S),
the instantiations with one template argument at value A beside their siblings with it at value B.

usage: tools/resource_usage.py FILE.s [FILE.s ...] --arg INDEX --a A --b B

Per pair one line: the other template arguments, then SGPRs, VGPRs, scratch bytes, static LDS bytes and waves
per SIMD of the A instantiation and of its B sibling (the "; Kernel info:" block the compiler writes after
each kernel).  The last line counts the A instantiations with scratch whose B sibling has none; exit status 1
if there is one.  (The marches' LDS is dynamic -- sized by the host per launch -- so the static figure is 0.)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("files", nargs="+")
    ap.add_argument("--arg", type=int, required=True, help="index of the template argument that differs")
    ap.add_argument("--a", type=int, required=True)
    ap.add_argument("--b", type=int, required=True)
    o = ap.parse_args()
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
