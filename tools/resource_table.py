#!/usr/bin/env python3
"""Reduce the output of `make -C .../csrc resource-usage` to one line per kernel, or compare two such outputs.

    resource_table.py NEW.log                 one line per kernel: registers, spills, scratch, LDS, occupancy
    resource_table.py OLD.log NEW.log         kernels only in one of the two, and every kernel whose numbers differ
"""
import re
import subprocess
import sys

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]")


def table(path):
    out, name = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            name = val
            out[name] = {}
        elif name and key in FIELDS:
            out[name][key] = val
    names = list(out)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {p: out[n] for n, p in zip(names, plain)}


def row(name, v):
    return "%-110s sgpr %3s vgpr %3s agpr %3s scratch %4s occ %s spill s%s v%s lds %s" % (
        name, v["TotalSGPRs"], v["VGPRs"], v["AGPRs"], v["ScratchSize [bytes/lane]"], v["Occupancy [waves/SIMD]"],
        v["SGPRs Spill"], v["VGPRs Spill"], v["LDS Size [bytes/block]"])


def main():
    if len(sys.argv) == 2:
        for n, v in sorted(table(sys.argv[1]).items()):
            print(row(n, v))
        return 0
    old, new = table(sys.argv[1]), table(sys.argv[2])
    both = sorted(set(old) & set(new))
    moved = [n for n in both if old[n] != new[n]]
    print("kernels: %d before, %d after, %d in both, %d of those with different numbers" % (len(old), len(new), len(both), len(moved)))
    for n in moved:
        print("MOVED  - " + row(n, old[n]))
        print("       + " + row(n, new[n]))
    for n in sorted(set(old) - set(new)):
        print("only before: " + row(n, old[n]))
    for n in sorted(set(new) - set(old)):
        print("only after:  " + row(n, new[n]))
    return 1 if moved else 0


if __name__ == "__main__":
    sys.exit(main())
