#!/usr/bin/env python3
"""Compare the kernels of two gfx950 device-assembly files (hipcc ... --cuda-device-only -S), kernel by kernel.

usage: tools/isa_compare.py A.s B.s [--trailing 0|1[,0|1...]]

A template kernel is paired by its template arguments (the kernels' names may differ: sdvr_march_kernel<...>
in A against dvr_march_kernel<..., true> in B), any other kernel by its name.  A boolean argument and an
integer one pair by value (bool SEP = true in A against int LAW = 1 in B); a kernel of B alone (LAW = 2) is
left out.  --trailing T: B's template
kernels carry the arguments T after A's -- only B's kernels that end in T take part, with T dropped.

Per pair one line: "identical", "identical up to labels and kernel-argument offsets" (with the offsets'
shifts), or "DIFFERENT" and the first differing lines.  Two things only are normalised: the function number n
of the .LBB<n>_<block> labels, and the literal offset of a scalar load whose base is the kernel-argument
pointer (the user SGPR pair the kernel descriptor assigns it).  The kernel descriptors (registers, LDS,
scratch) must be equal too, but for the size of the kernel arguments.  Exit status 1 if a pair differs or a
kernel of A has no partner.
"""
import argparse
import re
import sys

TEMPLATE = re.compile(r"^_ZN2vr\d+([a-z0-9_]+?)I((?:L[bi]\d+E)+)E")
PLAIN = re.compile(r"^_ZN2vr\d+([a-z0-9_]+?)E")
LBB = re.compile(r"\bL?BB\d+_")   # (.LBB<n>_<block>, and BB<n>_<block> in the loop comments)
SLOAD = re.compile(r"^(\s*s_load_dword(?:x\d+)?\s+\S+,\s*s\[(\d+):\d+\],\s*)(0x[0-9a-f]+|\d+)(.*)$")


def kernels(path):
    """{mangled name: (body lines, first SGPR of the kernel-argument pointer, descriptor lines)} of the file's
    kernels.  The body runs from the kernel's label to the section change ahead of its descriptor; the
    descriptor (.amdhsa_kernel ... .end_amdhsa_kernel: registers, LDS, scratch) is kept without the kernel's
    name and without .amdhsa_kernarg_size, the one entry an added argument has to change."""
    lines = open(path).read().split("\n")
    out = {}
    i = 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):", lines[i])
        if not m:
            i += 1
            continue
        name, j = m.group(1), i + 1
        while not lines[j].lstrip().startswith(".section"):
            j += 1
        body = lines[i + 1:j]
        while not lines[j].lstrip().startswith(".amdhsa_kernel"):
            j += 1
        if lines[j].split()[1] != name:   # (a device function, not a kernel)
            i = j
            continue
        # user SGPRs in the order the ABI fixes; the kernel-argument pointer follows those enabled before it
        at, desc = 0, []
        j += 1
        while not lines[j].lstrip().startswith(".end_amdhsa_kernel"):
            d = lines[j].split()
            if d[0] != ".amdhsa_kernarg_size":
                desc.append(" ".join(d))
            if len(d) == 2 and d[1] == "1":
                if d[0] == ".amdhsa_user_sgpr_private_segment_buffer":
                    at += 4
                elif d[0] in (".amdhsa_user_sgpr_dispatch_ptr", ".amdhsa_user_sgpr_queue_ptr"):
                    at += 2
            j += 1
        out[name] = (body, at, desc)
        i = j
    return out


def key_of(name, trailing=None):
    """(display name, pairing key) of a mangled kernel name; None if --trailing leaves the kernel out."""
    m = TEMPLATE.match(name)
    if m:
        args = tuple(int(a) for a in re.findall(r"L[bi](\d+)E", m.group(2)))
        shown = "%s<%s>" % (m.group(1), ", ".join(map(str, args)))
        if trailing is not None:
            if args[len(args) - len(trailing):] != trailing:
                return None
            args = args[:len(args) - len(trailing)]
        return shown, args
    m = PLAIN.match(name)
    return (m.group(1) if m else name), name


def normalised(body, karg):
    out, offs = [], []
    for ln in body:
        if LBB.search(ln):   # (a label's comment is padded to a column: the padding follows the number's width)
            ln = re.sub(r"\s+;", " ;", LBB.sub("BB#_", ln))
        m = SLOAD.match(ln)
        if m and int(m.group(2)) == karg:
            offs.append(int(m.group(3), 0))
            ln = m.group(1) + "<karg>" + m.group(4)
        out.append(ln)
    return out, offs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--trailing", default=None)
    o = ap.parse_args()
    trailing = tuple(int(t) for t in o.trailing.split(",")) if o.trailing else None
    A, B = kernels(o.a), kernels(o.b)
    bk = {}
    for name in B:
        if trailing is None and name in A:   # (the same kernel in both files: paired by its name, below)
            continue
        k = key_of(name, trailing)
        if k is None:
            continue
        if k[1] in bk:
            sys.exit("ambiguous pairing: %s and %s" % (bk[k[1]][0], k[0]))
        bk[k[1]] = (k[0], name)
    counts = {"identical": 0, "labels": 0, "different": 0, "unpaired": 0}
    for name in sorted(A, key=lambda n: key_of(n)[0]):
        shown, key = key_of(name)
        if trailing is None and name in B:
            bk[key] = (shown, name)
        if key not in bk:
            print("%s: NO PARTNER in %s" % (shown, o.b))
            counts["unpaired"] += 1
            continue
        shown_b, name_b = bk[key]
        title = shown if shown == shown_b else "%s | %s" % (shown, shown_b)
        if A[name][2] != B[name_b][2]:
            counts["different"] += 1
            print("%s: DIFFERENT kernel descriptors:" % title)
            for x, y in zip(A[name][2], B[name_b][2]):
                if x != y:
                    print("    A: %s\n    B: %s" % (x, y))
            continue
        if A[name][0] == B[name_b][0]:
            print("%s: identical (%d lines)" % (title, len(A[name][0])))
            counts["identical"] += 1
            continue
        (na, oa), (nb, ob) = normalised(*A[name][:2]), normalised(*B[name_b][:2])
        if na == nb:
            shifts = sorted({y - x for x, y in zip(oa, ob)})
            print("%s: identical up to labels and kernel-argument offsets (%d lines; offsets shifted by %s)"
                  % (title, len(na), ", ".join("%+d" % s for s in shifts) or "none"))
            counts["labels"] += 1
            continue
        counts["different"] += 1
        at = next((i for i, (x, y) in enumerate(zip(na, nb)) if x != y), min(len(na), len(nb)))
        print("%s: DIFFERENT (%d against %d lines), first at line %d:" % (title, len(na), len(nb), at + 1))
        for i in range(at, min(at + 4, max(len(na), len(nb)))):
            print("    A: %s" % (na[i] if i < len(na) else "<end>"))
            print("    B: %s" % (nb[i] if i < len(nb) else "<end>"))
    print("%d kernels of %s against %s: %d identical, %d identical up to labels and kernel-argument offsets, "
          "%d different, %d without a partner" % (len(A), o.a, o.b, counts["identical"], counts["labels"],
                                                  counts["different"], counts["unpaired"]))
    return 1 if counts["different"] or counts["unpaired"] else 0


if __name__ == "__main__":
    sys.exit(main())
