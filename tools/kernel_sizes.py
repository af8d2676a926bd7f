#!/usr/bin/env python3
"""Code size, registers, LDS and occupancy of every kernel of a translation unit, from the compiler's own remarks in its assembly:
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o /tmp/x.s colorid_amd/csrc/cid_kmerset.hip && python3 tools/kernel_sizes.py /tmp/x.s
(round 6: a kernel unrolled into 60 KB of code ran 15 % slower than its rolled form of 12 KB — the instruction cache is 64 KB for two CUs)
A kernel's remarks follow its .amdhsa_kernel directive and end before the next function's label; each figure is looked up on its own,
inside that stretch, whatever order the compiler prints them in."""
import re, subprocess, sys
txt = open(sys.argv[1]).read()
FIGURES = (r"; codeLenInByte = (\d+)", r"; NumVgprs: (\d+)", r"; (?:Total)?NumSgprs: (\d+)", r"; ScratchSize: (\d+)", r"; Occupancy: (\d+)", r"; LDSByteSize: (\d+)")
marks = list(re.finditer(r"^\t\.amdhsa_kernel (\w+)$", txt, re.M))
rows = []
for m in marks:
    label = re.compile(r"^\w+:", re.M).search(txt, m.end())          # the next function, kernel or not
    part = txt[m.end():label.start() if label else len(txt)]
    code, vgpr, sgpr, scratch, occ, lds = (re.search(f, part).group(1) for f in FIGURES)
    rows.append((int(code), subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()[:90], vgpr, sgpr, scratch, occ, lds))
for code, name, vgpr, sgpr, scratch, occ, lds in sorted(rows, reverse=True):
    print(f"{code:7d} B  vgpr {vgpr:>3s} sgpr {sgpr:>3s} scratch {scratch:>4s} occ {occ} lds {lds:>6s}  {name}")
