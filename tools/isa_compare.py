#!/usr/bin/env python3
"""Per-kernel resource use and instruction count of two device assembly files (hipcc
--cuda-device-only -S): the check that a change leaves an unrelated configuration's kernels alone.
    python tools/isa_compare.py old.s new.s
    python tools/isa_compare.py --exact old.s new.s
--exact compares each kernel's text as well (label to its .size directive, every early-exit
s_endpgm included, without the lines that carry the unit's __hip_cuid_ hash): one line per kernel, "identical" or its resource lines and a unified
diff of the instructions; the exit status is the number of kernels that differ.  Where the only
difference is v_bitop3_b32 with its first two sources commuted and the truth table adjusted
(0x78 = a ^ (b & c) against 0x6c = b ^ (a & c)), the count of such lines stands for the diff."""
import difflib
import re
import sys


def kernels(path):
    txt = open(path).read()
    meta = {}
    for blk in re.split(r"\n\s+- \.", txt.split("amdhsa.kernels:", 1)[1].split("amdhsa.target", 1)[0]):
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name:
            continue
        g = lambda k: (re.search(r"\.%s:\s+(\d+)" % k, blk) or [None, "?"])[1]
        meta[name.group(1)] = {k: g(k) for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count",
                                                  "sgpr_spill_count", "private_segment_fixed_size")}
    text = {}
    for name in meta:
        m = re.search(r"^%s:.*?\n(.*?)^\s*\.size\s+%s," % (re.escape(name), re.escape(name)), txt, re.S | re.M)
        body = m.group(1).splitlines() if m else []
        text[name] = [l for l in body if "__hip_cuid_" not in l]
        meta[name]["insts"] = sum(1 for l in body if l.strip() and not l.strip().startswith((".", ";", "//"))
                                  and not l.rstrip().endswith(":"))
    return meta, text


BITOP = re.compile(r"(v_bitop3_b32 \S+, )(\S+), (\S+)(, \S+ bitop3:)0x78")


def commuted(lines):
    return [BITOP.sub(r"\1\3, \2\g<4>0x6c", l) for l in lines]


exact = "--exact" in sys.argv
paths = [x for x in sys.argv[1:] if x != "--exact"]
(a, ta), (b, tb) = kernels(paths[0]), kernels(paths[1])
differ = 0
for k in sorted(set(a) | set(b)):
    short = re.sub(r"_Z\d+", "", k)[:60]
    if exact and a.get(k) == b.get(k) and ta.get(k) == tb.get(k):
        print(short, "identical (%s instructions)" % a[k]["insts"])
        continue
    differ += 1
    print(short, a.get(k), "\n" + " " * len(short), b.get(k), "" if a.get(k) == b.get(k) else "  <-- differs")
    if exact and commuted(ta.get(k, [])) == commuted(tb.get(k, [])):
        print("    %d v_bitop3_b32 lines with sources 0 and 1 commuted (0x78 <-> 0x6c), nothing else"
              % sum(x != y for x, y in zip(ta[k], tb[k])))
    elif exact:
        for l in difflib.unified_diff(ta.get(k, []), tb.get(k, []), "old", "new", n=0, lineterm=""):
            print("    " + l)
if exact:
    sys.exit(min(differ, 255))
