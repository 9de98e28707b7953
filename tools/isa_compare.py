#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two builds of the same .hip files.

    hipcc <csrc/Makefile FLAGS> -x hip --cuda-device-only -S f.hip -o DIR/f.s

once per side, then `isa_compare.py BEFORE_DIR AFTER_DIR f.s ...`.  Prints a
markdown table, one row per kernel: registers, scratch, LDS, occupancy, code
length, and whether the instruction lines are the same (comments and
assembler directives dropped, basic-block labels renumbered per function).  Exit status 1 when a resource
figure of any kernel differs.
"""
import re
import sys

FIELDS = ("NumVgprs", "NumSgprs", "ScratchSize", "LDSByteSize", "Occupancy", "codeLenInByte")


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(\w+):\s*(;.*)?$", line)
        if name is None:
            if m and not m.group(1).startswith("."):
                name, body, stats = m.group(1), [], {}
            continue
        code = line.split(";", 1)[0].strip()
        if code and (not code.startswith(".") or code.startswith(".LBB")):  # instructions and block labels
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", code))
        for f in FIELDS:
            m = re.match(r"^; (?:Total)?%s(?::| =) (\d+)" % f, line)  # (some compilers print TotalNumSgprs)
            if m:
                stats[f] = int(m.group(1))
        if line.startswith("; COMPUTE_PGM_RSRC2:TIDIG_COMP_CNT"):
            out[name] = (tuple(stats.get(f) for f in FIELDS), body)
            name = None
    return out


def main():
    before, after, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    bad = False
    print("| file | kernel | " + " | ".join(FIELDS) + " | instructions |")
    print("|---|---|" + "---|" * (len(FIELDS) + 1))
    for f in files:
        a, b = kernels("%s/%s" % (before, f)), kernels("%s/%s" % (after, f))
        for k in sorted(set(a) | set(b)):
            if k not in a or k not in b:
                print("| %s | `%s` | %s |" % (f, k, "only before" if k in a else "only after"))
                continue
            (sa, ia), (sb, ib) = a[k], b[k]
            cols = [str(x) if x == y else "%s -> %s" % (x, y) for x, y in zip(sa, sb)]
            bad |= sa[:5] != sb[:5]
            print("| %s | `%s` | %s | %s |" % (f, k, " | ".join(cols), "same" if ia == ib else "differ"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
