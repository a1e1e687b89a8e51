#!/usr/bin/env python3
"""The two heads of an HFE block at the UHD levels: wm_ln_conv1x1_dwconv_fwd (one kernel, the plane between the 1x1 and the depth-wise
3x3 never stored) against wm_conv2d_ln_fwd + wm_dwconv3x3_fwd, library calls on preallocated buffers.
  qkv         norm1 -> attn.qkv (32 -> 96) -> qkv_dwconv on the 64 q | k channels (the value third leaves as the 1x1 wrote it)
  project_in  norm2 -> ffn.project_in[0] (32 -> 32) -> project_in[1] (depth-wise 3x3, 32 channels)
Per call: the median of `--reps` timings (HIP events over `--iters` back-to-back calls each), the two paths alternating; GB/s on the
algorithmic bytes per position (qkv: 1024 -> 512; project_in: 512 -> 256).  A head takes the fused path at a level only if its slowest
fused repetition beats its fastest pair repetition.  --band-rows: further fused timings with the band height forced (the entry's own
choice is what the verdict is about).

usage: python tools/bench_hfe_heads.py [--reps 7] [--iters 20] [--band-rows 8,16,32]"""
import argparse, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wave_mamba_amd as wm
from wave_mamba_amd import _lib
from wave_mamba_amd.ops import _conv2d_wfrag, _ptr, _stream, check
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--band-rows", default="")
args = ap.parse_args()
forced = [int(r) for r in args.band_rows.split(",") if r]
dev = "cuda:0"
lib = _lib.load()
C, EPS = 32, 1e-6
g = torch.Generator(device=dev); g.manual_seed(0)
rn = lambda *s: torch.randn(*s, device=dev, generator=g)
lw, lb = 1.0 + 0.3 * rn(C), 0.2 * rn(C)


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
    x = rn(B, C, H, W)
    for name, cout, cdw, bytes_pair, bytes_fused in (("qkv       ", 96, 64, 1024, 512), ("project_in", 32, 32, 512, 256)):
        w, b, wd, bd = rn(cout, C, 1, 1) / C ** 0.5, rn(cout) * 0.1, rn(cdw, 1, 3, 3) / 3, rn(cdw) * 0.1
        frag = _conv2d_wfrag(w, cache=False)
        pre = torch.empty(B, cout, H, W, device=dev)
        yp, yf = torch.empty(B, cdw, H, W, device=dev), torch.empty(B, cout, H, W, device=dev)

        def pair():
            check(lib.wm_conv2d_ln_fwd(_ptr(x), _ptr(lw), _ptr(lb), EPS, _ptr(frag), _ptr(b), None, _ptr(pre), B, C, cout, H, W, st),
                  "conv2d_ln")
            check(lib.wm_dwconv3x3_fwd(_ptr(pre), _ptr(wd), _ptr(bd), _ptr(yp), B, cdw, H, W, 0, 0, st), "dwconv3x3")

        def fused(rows=0):
            check(lib.wm_ln_conv1x1_dwconv_fwd(_ptr(x), _ptr(lw), _ptr(lb), EPS, _ptr(frag), _ptr(b), _ptr(wd), _ptr(bd), _ptr(yf),
                                               B, C, cout, cdw, H, W, rows, st), "ln_conv1x1_dwconv")
        for _ in range(3):
            pair(); fused()
        tp, tf = [], []
        for _ in range(args.reps):
            tp.append(timed(pair)); tf.append(timed(fused))
        same = torch.equal(yp, yf[:, :cdw]) and torch.equal(pre[:, cdw:], yf[:, cdw:])
        mp, mf = statistics.median(tp), statistics.median(tf)
        print(f"level {lvl} {H}x{W} {name}: pair {mp:.3f} [{min(tp):.3f} .. {max(tp):.3f}] ms {bytes_pair * L / mp / 1e6:5.0f} GB/s | "
              f"fused {mf:.3f} [{min(tf):.3f} .. {max(tf):.3f}] ms {bytes_fused * L / mf / 1e6:5.0f} GB/s | "
              f"fused slowest < pair fastest: {max(tf) < min(tp)} | bit-identical: {same}", flush=True)
        for rows in forced:
            fused(rows)
            tr = [timed(lambda: fused(rows)) for _ in range(args.reps)]
            same = torch.equal(yp, yf[:, :cdw]) and torch.equal(pre[:, cdw:], yf[:, cdw:])
            print(f"    band height {rows:3d}: fused {statistics.median(tr):.3f} [{min(tr):.3f} .. {max(tr):.3f}] ms | bit-identical: {same}",
                  flush=True)
