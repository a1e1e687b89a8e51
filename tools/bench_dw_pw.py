#!/usr/bin/env python3
"""HFE's two depth-wise-3x3 -> 1x1 sites at the UHD levels: wm_dwconv_conv1x1_fwd (one kernel, the plane between the two never
stored) against wm_dwconv3x3_fwd + wm_conv2d_fwd, library calls on preallocated buffers.
  ffn    FeedForward.project_out: dwconv3x3(GELU) + conv1x1(+ residual)               -> the fused call
  value  CMTAttention: dwconv3x3 over the 96 qkv channels + conv1x1(v, + residual)    -> dwconv3x3 over the 64 q | k channels + the
         fused call on channels 64..95
Per call: the median of `--reps` timings (HIP events over `--iters` back-to-back calls each), the two paths alternating; GB/s on the
algorithmic bytes per position (ffn: 640 -> 384; value: 1152 -> 896).  A level takes the fused path only if its slowest fused
repetition beats its fastest pair repetition.

usage: python tools/bench_dw_pw.py [--reps 7] [--iters 20]"""
import argparse, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wave_mamba_amd as wm
from wave_mamba_amd import _lib
from wave_mamba_amd.ops import _conv2d_wfrag, _ptr, _stream, check
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
args = ap.parse_args()
dev = "cuda:0"
lib = _lib.load()
C = 32
g = torch.Generator(device=dev); g.manual_seed(0)
rn = lambda *s: torch.randn(*s, device=dev, generator=g)
wd, bd, w, b = rn(3 * C, 1, 3, 3) / 3, rn(3 * C) * 0.1, rn(C, C, 1, 1) / C ** 0.5, rn(C) * 0.1
frag = _conv2d_wfrag(w, cache=False)


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
    st = _stream()
    pre, res = rn(B, 3 * C, H, W), rn(B, C, H, W)
    mid = torch.empty(B, 3 * C, H, W, device=dev)
    yp, yf = torch.empty(B, C, H, W, device=dev), torch.empty(B, C, H, W, device=dev)
    v_off = 2 * C * L * 4                                     # byte offset of channel 64 inside one image

    def dw(x, c0, n, y, act):
        check(lib.wm_dwconv3x3_fwd(x, _ptr(wd) + c0 * 36, _ptr(bd) + c0 * 4, y, B, n, H, W, act, 0, st), "dwconv3x3")

    def pw(x, y):
        check(lib.wm_conv2d_fwd(x, None, None, _ptr(frag), _ptr(b), None, _ptr(res), y, B, C, 0, 0, C, H, W, 1, st), "conv2d")

    def fu(x, xbs, c0, y, act):
        check(lib.wm_dwconv_conv1x1_fwd(x, xbs, _ptr(wd) + c0 * 36, _ptr(bd) + c0 * 4, act, _ptr(frag), _ptr(b), _ptr(res), y,
                                        B, C, C, H, W, st), "dwconv_conv1x1")
    forms = {
        "ffn  ": (lambda: (dw(_ptr(pre), 0, C, _ptr(mid), 2), pw(_ptr(mid), _ptr(yp))),
                  lambda: fu(_ptr(pre), C * L, 0, _ptr(yf), 2), 640, 384),
        "value": (lambda: (dw(_ptr(pre), 0, 3 * C, _ptr(mid), 0), pw(_ptr(mid) + v_off, _ptr(yp))),
                  lambda: (dw(_ptr(pre), 0, 2 * C, _ptr(mid), 0), fu(_ptr(pre) + v_off, 3 * C * L, 2 * C, _ptr(yf), 0)), 1152, 896),
    }
    for name, (pair, fused, bytes_pair, bytes_fused) in forms.items():
        for _ in range(3):
            pair(); fused()
        tp, tf = [], []
        for _ in range(args.reps):
            tp.append(timed(pair)); tf.append(timed(fused))
        same = torch.equal(yp, yf)
        mp, mf = statistics.median(tp), statistics.median(tf)
        print(f"level {lvl} {H}x{W} {name}: pair {mp:.3f} [{min(tp):.3f} .. {max(tp):.3f}] ms {bytes_pair * L / mp / 1e6:5.0f} GB/s | "
              f"fused {mf:.3f} [{min(tf):.3f} .. {max(tf):.3f}] ms {bytes_fused * L / mf / 1e6:5.0f} GB/s | "
              f"fused slowest < pair fastest: {max(tf) < min(tp)} | bit-identical: {same}")
