#!/usr/bin/env python3
"""The carry launch of wm_ss2d_core_fwd at the three UHD pyramid levels: stored-P summaries (wm_ss2d_core_carry_select(1))
against sum_dt summaries (0), alternating, `--reps` repetitions of `--calls` calls each.  Per level: the plan's chunk counts
and summary bytes per call, then ms per call as median [fastest .. slowest] of the repetitions - the whole core call (events
around the repetition, no per-launch events) and, from a second pass, the carry launch alone (the library's per-class events).
   python tools/bench_core_carry.py [--reps 7] [--calls 20] [--levels 1 2 3] [--dstate 16]"""
import argparse, ctypes, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wave_mamba_amd as wm

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--levels", type=int, nargs="*", default=[1, 2, 3])
ap.add_argument("--dstate", type=int, default=16)
args = ap.parse_args()
dev = "cuda:0"
lib = wm._lib.load()
print("lib:", wm._lib.LIB_PATH, "build", wm._lib.build_id(), "device", torch.cuda.get_device_name(0))


def fmt(v):
    return f"{statistics.median(v):.4f} [{min(v):.4f} .. {max(v):.4f}]"


for lvl in args.levels:
    H, W = 2176 >> lvl, 3840 >> lvl
    B, D, N, R = 1, 64, args.dstate, 2
    NP = 16 if N <= 16 else 32
    plan = (ctypes.c_int * 10)()
    assert lib.wm_ss2d_core_plan(B, D, H, W, N, R, plan) == 0
    row, col = plan[6], W * plan[2]
    entries = 2 * (row + col)                                    # chunk entries of the four directions
    h_mb = entries * B * D * NP * 4 / 1e6
    print(f"level {lvl} {H}x{W}: row_nchunks {row}, col_nchunks {col}, per {-(-row // 64)} / {-(-col // 64)}; per call H {h_mb:.2f} MB, "
          f"stored P {h_mb:.2f} MB, sum_dt {h_mb / NP:.2f} MB; the carry moves {3 * h_mb:.1f} MB (stored P: read P and H, write H_in) or "
          f"{(2 + 1 / NP) * h_mb:.1f} MB (sum_dt)")
    g = torch.Generator(device=dev); g.manual_seed(lvl)
    x = torch.randn(B, D, H, W, device=dev, generator=g)
    Wx = torch.randn(4, R + 2 * N, D, device=dev, generator=g) / 8
    Wdt = torch.randn(4, D, R, device=dev, generator=g) * 0.7
    bias = torch.randn(4, D, device=dev, generator=g) * 0.5 - 3.0
    A_logs = torch.log(torch.arange(1, N + 1, device=dev, dtype=torch.float32)).repeat(4 * D, 1)
    Ds = torch.ones(4 * D, device=dev)
    call = lambda: wm.ops.ss2d_core(x, Wx, Wdt, bias, A_logs, Ds)
    outs = {}
    for mode in (1, 0):
        assert lib.wm_ss2d_core_carry_select(mode) == 0
        for _ in range(3):
            outs[mode] = call()
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    whole, carry = {0: [], 1: []}, {0: [], 1: []}
    for rep in range(args.reps):
        for mode in (1, 0):
            assert lib.wm_ss2d_core_carry_select(mode) == 0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                call()
            e1.record(); torch.cuda.synchronize()
            whole[mode].append(e0.elapsed_time(e1) / args.calls)
    for rep in range(args.reps):
        for mode in (1, 0):
            assert lib.wm_ss2d_core_carry_select(mode) == 0
            wm.ops.prof_enable(("selscan_carry",))
            for _ in range(args.calls):
                call()
            torch.cuda.synchronize()
            n, ms = wm.ops.prof_collect()["selscan_carry"]; wm.ops.prof_enable(False)
            assert n == args.calls, n
            carry[mode].append(ms / n)
    lib.wm_ss2d_core_carry_select(0)
    for mode, name in ((1, "stored P"), (0, "sum_dt  ")):
        print(f"  {name}: core call {fmt(whole[mode])} ms   carry launch {fmt(carry[mode])} ms")
    print(f"  outputs torch.equal: {same};  carry: sum_dt slowest < stored-P fastest: {max(carry[0]) < min(carry[1])};  "
          f"core call: {max(whole[0]) < min(whole[1])}")
