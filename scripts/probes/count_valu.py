#!/usr/bin/env python3
"""Static count of vector ALU instructions (v_*) per kernel of an AMDGPU assembly file (hipcc -S --cuda-device-only)."""
import re
import sys

cur, cnt = None, {}
for line in open(sys.argv[1]):
    m = re.match(r"^(\w+):\s*; @", line)
    if m:
        cur = m.group(1)
        cnt[cur] = 0
        continue
    if line.strip().startswith("s_endpgm"):
        cur = None
    if cur and re.match(r"\s+v_", line):
        cnt[cur] += 1
for k, v in cnt.items():
    print("%-12s %d" % (k, v))
