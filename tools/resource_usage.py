#!/usr/bin/env python3
"""Kernel resource usage of one compilation, from the compiler's own remarks.

Compile a kernel file for the device alone with the flags of build.sh plus
``-Rpass-analysis=kernel-resource-usage`` and keep the compiler's stderr; this script turns that text into one
line per kernel (registers, spills, scratch, LDS, occupancy), or compares two such texts kernel by kernel:

    resource_usage.py remarks.txt                 # the table
    resource_usage.py before.txt after.txt       # kernels that differ, that left and that are new

Exit status 1 when a kernel both texts hold differs in any figure.
"""
import re
import subprocess
import sys

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Dynamic Stack", "Occupancy [waves/SIMD]",
          "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def parse(path):
    kernels, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(.+?): (\S+) \[-Rpass-analysis", line)
        if m and cur is not None and m.group(1).strip() in FIELDS:
            cur[m.group(1).strip()] = m.group(2)
    return kernels


def row(k):
    return "  ".join("%s=%s" % (f.split(" [")[0], k.get(f, "?")) for f in FIELDS)


def main(argv):
    if len(argv) == 2:
        ks = parse(argv[1])
        names = demangle(sorted(ks))
        for n in sorted(ks):
            print("%s\n    %s" % (names[n], row(ks[n])))
        return 0
    a, b = parse(argv[1]), parse(argv[2])
    names = demangle(sorted(set(a) | set(b)))
    differ = [n for n in sorted(a) if n in b and a[n] != b[n]]
    print("%d kernels before, %d after, %d in both, %d of those differ" % (len(a), len(b), len(set(a) & set(b)),
                                                                           len(differ)))
    for n in differ:
        print("DIFFERS %s\n    before %s\n    after  %s" % (names[n], row(a[n]), row(b[n])))
    for n in sorted(set(a) - set(b)):
        print("GONE    %s\n    %s" % (names[n], row(a[n])))
    for n in sorted(set(b) - set(a)):
        print("NEW     %s\n    %s" % (names[n], row(b[n])))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
