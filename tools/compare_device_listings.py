#!/usr/bin/env python3
"""Are two device listings of the HIP library the same code?

A change that touches host code only must leave the device code as it was.  Make the listing of both trees, in csrc/ of each:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value --cuda-device-only -S -o X.s sdvpcm_hip.hip

(the developer build: with -DSDV_DEV_AIDS) and give both to this script.  It compares text.  The lines that carry the compilation unit's
__hip_cuid_<hash> symbol differ after any edit and are dropped.  First the listings are compared line for line; if they differ - moving a launch can
change the order in which template kernels are emitted - they are compared function by function: the text of every symbol (from its label to its
.Lfunc_end), the .amdhsa_kernel descriptors and the metadata entries, by name.  Exit status 0: the same; 1: not."""
import re
import sys


def lines_of(path):
    return [l.rstrip("\n") for l in open(path, errors="replace") if "__hip_cuid_" not in l]


def pieces(lines):
    """name -> text, for functions, kernel descriptors and metadata entries"""
    out = {}
    i, n = 0, len(lines)
    while i < n:
        l = lines[i]
        m = re.match(r"^([A-Za-z_$.][\w$.]*):", l)
        if m and not l.startswith(".L") and i > 0:
            name, j = m.group(1), i + 1
            while j < n and not lines[j].startswith(".Lfunc_end"):
                if re.match(r"^[A-Za-z_$][\w$.]*:", lines[j]):
                    break
                j += 1
            if j < n and lines[j].startswith(".Lfunc_end"):
                out["function " + name] = "\n".join(lines[i:j])
                i = j
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", l)
        if m:
            j = i
            while j < n and ".end_amdhsa_kernel" not in lines[j]:
                j += 1
            out["descriptor " + m.group(1)] = "\n".join(lines[i:j + 1])
            i = j
        m = re.match(r"^  - \.(?:agpr_count|args):", l)
        if m:
            j = i + 1
            while j < n and not lines[j].startswith("  - .") and not lines[j].startswith("amdhsa.") and not lines[j].startswith("..."):
                j += 1
            body = "\n".join(lines[i:j])
            nm = re.search(r"^\s+\.name:\s+(\S+)", body, re.M)
            out["metadata " + (nm.group(1) if nm else str(i))] = body
            i = j - 1
        i += 1
    return out


def main(a, b):
    la, lb = lines_of(a), lines_of(b)
    kernels = sum(1 for l in la if re.match(r"^\s*\.amdhsa_kernel\s", l))
    if la == lb:
        print("identical line for line (%d lines, %d kernels; __hip_cuid_ lines dropped)" % (len(la), kernels))
        return 0
    pa, pb = pieces(la), pieces(lb)
    bad = sorted(k for k in set(pa) | set(pb) if pa.get(k) != pb.get(k))
    if not bad and pa:
        print("not identical line for line, but every function, kernel descriptor and metadata entry is the same text (%d pieces, %d kernels): emitted in another order" % (len(pa), kernels))
        return 0
    for k in bad[:40]:
        print("differs: %s%s" % (k, "" if k in pa and k in pb else " (only in %s)" % (a if k in pa else b)))
    print("%d of %d pieces differ" % (len(bad), len(set(pa) | set(pb))))
    return 1


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
