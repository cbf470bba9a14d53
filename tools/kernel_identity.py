#!/usr/bin/env python3
"""Per-function comparison of two device assembly files of one unit (hipcc ... --cuda-device-only -S with the unit's
build.sh flags): for every function symbol the instruction text between its label and .Lfunc_end (comments and
directives dropped, block labels renumbered) and its resource block. Prints one line per function: identical,
differs, added or lost, with VGPRs, AGPRs, SGPRs, LDS bytes, scratch bytes and occupancy of the second file.

usage: kernel_identity.py <unit name> <parent.s> <this.s>"""
import re
import subprocess
import sys

RES = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "LDSByteSize", "ScratchSize", "Occupancy")


def functions(path):
    out, name, body, res = {}, None, [], {}
    lines = open(path).read().split("\n")
    i = 0
    while i < len(lines):
        line = lines[i]
        m = re.match(r"^(_Z\w+|\w+):\s*(;.*)?$", line)
        if name is None and m and not line.startswith(".L"):
            name, body, res = m.group(1), [], {}
        elif name is not None:
            if line.startswith(".Lfunc_end"):
                # the resource block follows as comments
                j = i + 1
                while j < len(lines) and not re.match(r"^(_Z\w+|\w+):", lines[j]) and j < i + 80:
                    r = re.match(r"^\s*;\s*(\w+):\s*(\d+)", lines[j])
                    if r and r.group(1) in RES:
                        res[r.group(1)] = int(r.group(2))
                    j += 1
                labels = {}
                text = []
                for b in body:
                    b = re.sub(r";.*$", "", b).strip()
                    if not b or b.startswith(".") and not re.match(r"^\.LBB\d+_\d+:", b):
                        continue
                    b = re.sub(r"\.LBB\d+_\d+", lambda q: labels.setdefault(q.group(0), "L%d" % len(labels)), b)
                    text.append(b)
                out[name] = ("\n".join(text), res)
                name = None
            else:
                body.append(line)
        i += 1
    return out


def demangle(names):
    p = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    got = p.stdout.split("\n") if p.returncode == 0 else names
    return dict(zip(names, got))


def main():
    unit, old, new = sys.argv[1:4]
    fo, fn = functions(old), functions(new)
    names = sorted(set(fo) | set(fn))
    dm = demangle(names)
    count = dict(identical=0, differs=0, added=0, lost=0)
    for n in names:
        if n not in fo:
            what = "added"
        elif n not in fn:
            what = "lost"
        else:
            what = "identical" if fo[n] == fn[n] else "differs"
        count[what] += 1
        r = (fn.get(n) or fo[n])[1]
        short = re.sub(r"\(.*$", "", dm[n]).replace("void ", "")
        print("%-100s %-6s %-9s v%-4d a%-3d s%-4d lds%-7d scr%-5d occ%d" % (
            short, unit, what, r.get("NumVgprs", -1), r.get("NumAgprs", -1), r.get("TotalNumSgprs", -1),
            r.get("LDSByteSize", -1), r.get("ScratchSize", -1), r.get("Occupancy", -1)))
    print("# %s: %s" % (unit, ", ".join("%d %s" % (v, k) for k, v in count.items())))


if __name__ == "__main__":
    main()
