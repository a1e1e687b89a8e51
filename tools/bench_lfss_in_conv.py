#!/usr/bin/env python3
"""SS2D's prologue at the UHD levels: wm_lfss_in_conv_fwd (one kernel, x never stored) against wm_lfss_in_fwd(z = NULL) +
wm_dwconv3x3_fwd(SiLU).  Per call: the median of `--reps` timings (HIP events over `--iters` back-to-back calls each), the two paths
alternating, both token layouts; GB/s on the algorithmic bytes (fused: 128 B of tokens in + 256 B of xc out per position; pair: 896).

usage: python tools/bench_lfss_in_conv.py [--reps 7] [--iters 20]"""
import argparse, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wave_mamba_amd as wm
from wave_mamba_amd import _lib
from wave_mamba_amd.ops import _ptr, _stream, check
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
args = ap.parse_args()
dev = "cuda:0"
lib = _lib.load()
C, D = 32, 64
g = torch.Generator(device=dev); g.manual_seed(0)
rn = lambda *s: torch.randn(*s, device=dev, generator=g)
ln1w, ln1b, Win, cw, cb = rn(C) * 0.1 + 1, rn(C) * 0.1, rn(2 * D, C) / 6, rn(D, 1, 3, 3) / 3, rn(D) * 0.1


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.iters


print(f"build {_lib.build_id()}, {torch.cuda.get_device_name(0)}; ms per call: median [min .. max] of {args.reps} x {args.iters} calls")
for lvl in (1, 2, 3):
    H, W = 2176 >> lvl, 3840 >> lvl
    L, B = H * W, 1
    rb = lib.wm_lfss_in_conv_band_rows(B, H, W)
    for nchw in (1, 0):
        tok = rn(B, C, L) if nchw else rn(B, L, C)
        x, xc, xf = (torch.empty(B, D, H, W, device=dev) for _ in range(3))
        st = _stream()
        def pair():
            check(lib.wm_lfss_in_fwd(_ptr(tok), nchw, _ptr(ln1w), _ptr(ln1b), 1e-5, _ptr(Win), _ptr(x), None, B, L, C, 0, st), "in")
            check(lib.wm_dwconv3x3_fwd(_ptr(x), _ptr(cw), _ptr(cb), _ptr(xc), B, D, H, W, 1, 0, st), "dwconv")
        def fused():
            check(lib.wm_lfss_in_conv_fwd(_ptr(tok), nchw, _ptr(ln1w), _ptr(ln1b), 1e-5, _ptr(Win), _ptr(cw), _ptr(cb), _ptr(xf), B, H, W, C, 0, st), "in_conv")
        for _ in range(3):
            pair(); fused()
        tp, tf = [], []
        for _ in range(args.reps):
            tp.append(timed(pair)); tf.append(timed(fused))
        same = torch.equal(xc, xf)
        mp, mf = statistics.median(tp), statistics.median(tf)
        print(f"level {lvl} {H}x{W} {'nchw  ' if nchw else 'tokens'} (band {rb:2d} rows): pair {mp:.3f} [{min(tp):.3f} .. {max(tp):.3f}] ms {896 * L / mp / 1e6:5.0f} GB/s | "
              f"fused {mf:.3f} [{min(tf):.3f} .. {max(tf):.3f}] ms {384 * L / mf / 1e6:5.0f} GB/s | fused slowest < pair fastest: {max(tf) < min(tp)} | "
              f"bit-identical: {same}")
