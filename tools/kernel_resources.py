#!/usr/bin/env python3
"""Per-kernel register / scratch / LDS usage of the library (hipcc -Rpass-analysis=kernel-resource-usage over every unit, with the
library's own flags: wave_mamba_amd/build.py build_variant), one line each.

usage: python tools/kernel_resources.py [substring-of-demangled-name] [extra hipcc flags ...]
"""
import re, subprocess, sys, os
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
from wave_mamba_amd import build
flt = sys.argv[1] if len(sys.argv) > 1 else ""
err = "".join(build.build_variant(os.path.join(root, "build", "asm_resources"), asm=True, force=True,
                                  extra_flags=["-Rpass-analysis=kernel-resource-usage"] + sys.argv[2:]).values())
cur = None
rows = {}
for line in err.splitlines():
    m = re.search(r"remark: (?:\S+: )?\s*Function Name: (\S+)", line) or re.search(r"Function Name: (\S+)", line)
    if m:
        cur = m.group(1); rows[cur] = {}; continue
    m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/\w+\])?: (\d+)", line)
    if m and cur: rows[cur][m.group(1).strip()] = int(m.group(2))
names = list(rows)
dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
for n, d in zip(names, dem):
    if flt and flt not in d: continue
    r = rows[n]
    print(f"{d[:110]:110s} vgpr {r.get('VGPRs', -1):4d} agpr {r.get('AGPRs', -1):3d} sspill {r.get('SGPRs Spill', -1):3d} "
          f"vspill {r.get('VGPRs Spill', -1):3d} scratch {r.get('ScratchSize', -1):4d} occ {r.get('Occupancy', -1):2d} lds {r.get('LDS Size', -1)}")
