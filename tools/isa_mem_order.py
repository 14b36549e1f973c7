#!/usr/bin/env python3
"""Dev tool: a kernel's vector-memory instructions, the waits that name vmcnt and the barriers, in
program order with their source lines, from a hipcc -S -gline-tables-only listing -- to see whether
a group of loads goes out as one batch (no s_waitcnt with a vmcnt term between them).
    python tools/isa_mem_order.py LISTING.s KERNEL_SUBSTRING [FILE:LO-HI ...]
With FILE:LO-HI ranges only instructions from those source lines are shown (barriers always)."""
import re
import sys

path, ksub = sys.argv[1], sys.argv[2]
ranges = []
for r in sys.argv[3:]:
    f, lohi = r.split(":")
    lo, hi = lohi.split("-")
    ranges.append((f, int(lo), int(hi)))
pat = re.compile(r"\s+((?:global|flat|buffer)_(?:load|store|atomic)\w*|s_waitcnt\b.*vmcnt.*|s_barrier)\b")
files, cur, fn, n = {}, None, None, 0
for line in open(path):
    m = re.match(r"^(_Z\w+):", line)
    if m:
        fn = m.group(1)
    m = re.match(r'\s*\.file\s+(\d+)\s+"[^"]*"\s+"([^"]+)"', line)
    if m:
        files[m.group(1)] = m.group(2).split("/")[-1]
        continue
    m = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", line)
    if m:
        cur = (files.get(m.group(1), m.group(1)), int(m.group(2)))
        continue
    if not (fn and ksub in fn):
        continue
    if re.match(r"\s+[a-z]\w+", line):
        n += 1
    m = pat.match(line)
    if not m:
        continue
    ins = m.group(1).split(";")[0].strip()
    show = not ranges or ins == "s_barrier" or (cur and any(cur[0] == f and lo <= cur[1] <= hi for f, lo, hi in ranges))
    if show:
        print(f"{n:6d}  {ins:40s} {cur[0]}:{cur[1]}" if cur else f"{n:6d}  {ins}")
