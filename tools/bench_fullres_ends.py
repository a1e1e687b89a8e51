#!/usr/bin/env python3
"""The two full-resolution 32-channel planes at the ends of the UHD forward, per call, library calls on preallocated buffers:
  head   UNet.conv_01 (3 -> 32, 3x3) + the level-1 Haar analysis        -> wm_conv2d_dwt_fwd (bands formed in the convolution's epilogue)
  tail   the level-1 Haar synthesis of (low, h_out_conv) + UNet.last (32 -> 3, 3x3, + image) -> wm_idwt_conv2d_fwd (the input tile
         formed from the bands by the convolution's producer waves)
First every call of the pairs on its own (conv_01, dwt, iwt, last), then pair against fused, alternating: the median of `--reps`
timings (HIP events over `--iters` back-to-back calls each) with [fastest .. slowest], and GB/s on the algorithmic bytes per
full-resolution position (head: 12 + 128 + 128 + 128 -> 12 + 128; tail: 128 + 128 + 128 + 12 + 12 -> 128 + 12 + 12).  A map takes the
fused path only if its slowest fused repetition beats its fastest pair repetition.  A library without a fused entry (the parent of
the change) reports that pair alone.

usage: python tools/bench_fullres_ends.py [--reps 7] [--iters 20] [--sizes 2176x3840,1088x1920]"""
import argparse, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wave_mamba_amd as wm
from wave_mamba_amd import _lib
from wave_mamba_amd.ops import _conv2d_wfrag, _ptr, _stream, check
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--sizes", default="2176x3840,1088x1920")
args = ap.parse_args()
dev = "cuda:0"
lib = _lib.load()
C = 32
g = torch.Generator(device=dev); g.manual_seed(0)
rn = lambda *s: torch.randn(*s, device=dev, generator=g)
w01, b01, wl, bl = rn(C, 3, 3, 3) / 27 ** 0.5, rn(C) * 0.1, rn(3, C, 3, 3) / (9 * C) ** 0.5, rn(3) * 0.1
f01, fl = _conv2d_wfrag(w01, cache=False), _conv2d_wfrag(wl, cache=False)
fused_head, fused_tail = "wm_conv2d_dwt_fwd" in _lib.SIGNATURES, "wm_idwt_conv2d_fwd" in _lib.SIGNATURES


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.iters


def series(fns):
    """`--reps` timings of each callable, the callables alternating -> one list per callable."""
    for _ in range(3):
        for fn in fns:
            fn()
    ts = [[] for _ in fns]
    for _ in range(args.reps):
        for t, fn in zip(ts, fns):
            t.append(timed(fn))
    return ts


def fmt(t, nbytes):
    m = statistics.median(t)
    return f"{m:.3f} [{min(t):.3f} .. {max(t):.3f}] ms {nbytes / m / 1e6:5.0f} GB/s"


print(f"build {_lib.build_id()}, {torch.cuda.get_device_name(0)}; ms per call: median [min .. max] of {args.reps} x {args.iters} calls")
for size in args.sizes.split(","):
    H, W = (int(v) for v in size.split("x"))
    B, L, st = 1, H * W, _stream()
    h, w = H // 2, W // 2
    img = torch.rand(B, 3, H, W, device=dev, generator=g)
    low, high = rn(B, C, h, w), rn(B, 3 * C, h, w)
    plane = torch.empty(B, C, H, W, device=dev)
    bands_p = [torch.empty(B, C, h, w, device=dev) for _ in range(4)]
    bands_f = [torch.empty(B, C, h, w, device=dev) for _ in range(4)]
    out, out_f = torch.empty(B, 3, H, W, device=dev), torch.empty(B, 3, H, W, device=dev)
    hp = [_ptr(low)] + [_ptr(high) + k * C * h * w * 4 for k in range(3)]

    def conv_01():
        check(lib.wm_conv2d_fwd(_ptr(img), None, None, _ptr(f01), _ptr(b01), None, None, _ptr(plane), B, 3, 0, 0, C, H, W, 3, st), "conv_01")

    def dwt():
        check(lib.wm_dwt2d_fwd(_ptr(plane), *[_ptr(t) for t in bands_p], B, C, H, W, 0, st), "dwt")

    def iwt():
        check(lib.wm_idwt2d_fwd(*hp, C * h * w, 3 * C * h * w, 3 * C * h * w, 3 * C * h * w, _ptr(plane), B, C, h, w, 0, st), "iwt")

    def last():
        check(lib.wm_conv2d_fwd(_ptr(plane), None, None, _ptr(fl), _ptr(bl), None, _ptr(img), _ptr(out), B, C, 0, 0, 3, H, W, 3, st), "last")

    def head_fused():
        check(lib.wm_conv2d_dwt_fwd(_ptr(img), _ptr(f01), _ptr(b01), *[_ptr(t) for t in bands_f], B, 3, C, H, W, 0, st), "conv2d_dwt")

    def tail_fused():
        check(lib.wm_idwt_conv2d_fwd(_ptr(low), _ptr(high), _ptr(fl), _ptr(bl), _ptr(img), _ptr(out_f), B, C, 3, H, W, 0, st), "idwt_conv2d")

    # the tail first (it leaves the synthesised plane in `plane`), then the head (conv_01 overwrites it)
    t_iwt, t_last = series([iwt, last])
    t_c01, t_dwt = series([conv_01, dwt])
    print(f"{H}x{W} conv_01: {fmt(t_c01, 140 * L)}")
    print(f"{H}x{W} dwt    : {fmt(t_dwt, 256 * L)}")
    print(f"{H}x{W} iwt    : {fmt(t_iwt, 256 * L)}")
    print(f"{H}x{W} last   : {fmt(t_last, 152 * L)}")
    if fused_head:
        tp, tf = series([lambda: (conv_01(), dwt()), head_fused])
        same = all(torch.equal(a, b) for a, b in zip(bands_p, bands_f))
        print(f"{H}x{W} head   : pair {fmt(tp, 396 * L)} | fused {fmt(tf, 140 * L)} | "
              f"fused slowest < pair fastest: {max(tf) < min(tp)} | bit-identical: {same}")
    if fused_tail:
        tp, tf = series([lambda: (iwt(), last()), tail_fused])
        print(f"{H}x{W} tail   : pair {fmt(tp, 408 * L)} | fused {fmt(tf, 152 * L)} | "
              f"fused slowest < pair fastest: {max(tf) < min(tp)} | bit-identical: {torch.equal(out, out_f)}")
