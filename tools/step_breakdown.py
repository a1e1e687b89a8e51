#!/usr/bin/env python3
"""Per-step kernel-time breakdown from a rocprofv3 --kernel-trace CSV of bench.py (steps delimited by the first
kernel that runs once per forward).  python tools/step_breakdown.py <bench_kernel_trace.csv> [nsteps]"""
import collections, csv, functools, math, sys
rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r['Start_Timestamp']))
idx = [i for i, r in enumerate(rows) if 'selscan_chunk_kernel' in r['Kernel_Name']]
rows = rows[:idx[0]] if idx else rows              # drop the op-boundary scan leg that follows the timed region
# a forward starts at the first kernel that runs once per forward.  Forwards in the trace: the greatest common divisor of the
# dispatch counts that at least two kernel names share (a kernel of the forward runs a multiple of it; copies and one-off preparation
# kernels have counts of their own).  (Until the level-1 analysis moved into conv_01's kernel the three Haar analysis launches
# delimited the steps.)
cnt = collections.Counter(r['Kernel_Name'] for r in rows)
once = functools.reduce(math.gcd, [c for c, k in collections.Counter(cnt.values()).items() if k >= 2 and c >= 5])
first = next(r['Kernel_Name'] for r in rows if cnt[r['Kernel_Name']] == once)
starts = [i for i, r in enumerate(rows) if r['Kernel_Name'] == first]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 3
# `bench.py --full --steps 5 --warmup 3 --timed-only`: 3 warm-up + 5 timed forwards; use timed steps 2..4 (the last one has no
# successor to delimit it)
s0, s1 = starts[3 + 1], starts[3 + 1 + n]
step = rows[s0:s1]
dur = lambda r: int(r['End_Timestamp']) - int(r['Start_Timestamp'])
agg = collections.defaultdict(lambda: [0, 0])
gaps = 0
for a, b in zip(step, step[1:]):
    g = int(b['Start_Timestamp']) - int(a['End_Timestamp'])
    if g > 0: gaps += g
for r in step:
    agg[r['Kernel_Name']][0] += 1; agg[r['Kernel_Name']][1] += dur(r)
tot = sum(v[1] for v in agg.values()); wmt = sum(v[1] for k, v in agg.items() if 'wm::' in k)
wall = (int(rows[s1]['Start_Timestamp']) - int(rows[s0]['Start_Timestamp'])) / n / 1e6
print(f"# per-step kernel time, mean of {n} timed steps of `rocprofv3 --kernel-trace -- python bench.py --full --steps 5 --warmup 3 --no-cpu-baseline --timed-only`")
print(f"# step wall {wall:.2f} ms; sum of kernel durations {tot / n / 1e6:.2f} ms/step in {len(step) / n:.0f} dispatches (kernels of the side "
      f"streams overlap the main stream's: the sum exceeds the wall, and a kernel sharing the GPU runs longer than alone); "
      f"wm:: kernels {wmt / n / 1e6:.2f} ms/step")
print("calls/step  ms/step  kernel")
for k, v in sorted(agg.items(), key=lambda kv: -kv[1][1])[:48]:
    print(f"{v[0] / n:9.1f} {v[1] / n / 1e6:8.3f}  {k[:130]}")
small = [(k, v) for k, v in agg.items() if v[1] / v[0] < 10000]
print(f"# dispatches shorter than 10 us: {sum(v[0] for _, v in small) / n:.0f} per step, {sum(v[1] for _, v in small) / n / 1e6:.3f} ms/step of kernel time")
