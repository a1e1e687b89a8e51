#!/usr/bin/env python3
"""The close of an LFSSBlock at the UHD levels: wm_lfss_mid_rz_tok_fwd + wm_lfss_ffn_fwd (f = conv1(ln_2(tok1)) never stored) against
wm_lfss_mid_rz_fwd + wm_lfss_out_conv_fwd, library calls on preallocated buffers, NCHW output.  Per call of the pair: the median of
`--reps` timings (HIP events over `--iters` back-to-back calls each), old and new alternating, and the same for the closing kernels
alone (out_conv against ffn).  A level takes the new pair only if its slowest repetition beats the old pair's fastest.  --band-rows:
further timings of wm_lfss_ffn_fwd alone with the band height forced (the entry's own plan is what the verdict is about).

usage: python tools/bench_lfss_ffn.py [--reps 7] [--iters 20] [--band-rows 4,8,16,32]"""
import argparse, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wave_mamba_amd as wm
from wave_mamba_amd import _lib
from wave_mamba_amd.ops import _ptr, _stream, check
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--band-rows", default="")
args = ap.parse_args()
forced = [int(r) for r in args.band_rows.split(",") if r]
dev = "cuda:0"
lib = _lib.load()
C, D = 32, 64
g = torch.Generator(device=dev); g.manual_seed(0)
rn = lambda *s: torch.randn(*s, device=dev, generator=g)
ln1w, ln1b, Win = rn(C) * 0.1 + 1, rn(C) * 0.1, rn(2 * D, C) / 6
onw, onb, Wout, skip1 = rn(D) * 0.1 + 1, rn(D) * 0.1, rn(C, D) / 8, rn(C) * 0.1 + 1
ln2w, ln2b, W1, b1 = rn(C) * 0.1 + 1, rn(C) * 0.1, rn(D, C) / 6, rn(D) * 0.1
cw, cb, W3, b3, skip2 = rn(D, 1, 3, 3) / 3, rn(D) * 0.1, rn(C, C) / 6, rn(C) * 0.1, rn(C) * 0.1 + 1


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.iters


def row(ts):
    return f"{statistics.median(ts):.3f} [{min(ts):.3f} .. {max(ts):.3f}]"


print(f"build {_lib.build_id()}, {torch.cuda.get_device_name(0)}; ms per call: median [min .. max] of {args.reps} x {args.iters} calls")
for lvl in (1, 2, 3):
    H, W = 2176 >> lvl, 3840 >> lvl
    L, B = H * W, 1
    rb = lib.wm_lfss_ffn_band_rows(B, H, W)
    st = _stream()
    y4, tok = rn(4, B, D, L), rn(B, C, L)
    t_old, t_new, f = torch.empty(B, L, C, device=dev), torch.empty(B, L, C, device=dev), torch.empty(B, D, H, W, device=dev)
    o_old, o_new = torch.empty(B, C, H, W, device=dev), torch.empty(B, C, H, W, device=dev)
    head = (_ptr(y4), 4, B * D * L, _ptr(tok), 1, _ptr(ln1w), _ptr(ln1b), 1e-5, _ptr(Win), _ptr(onw), _ptr(onb), 1e-5, _ptr(Wout), _ptr(skip1))

    def mid_old():
        check(lib.wm_lfss_mid_rz_fwd(*head, _ptr(ln2w), _ptr(ln2b), 1e-5, _ptr(W1), _ptr(b1), _ptr(t_old), _ptr(f), B, L, C, 0, st), "mid_rz")

    def out_old():
        check(lib.wm_lfss_out_conv_fwd(_ptr(f), _ptr(cw), _ptr(cb), _ptr(t_old), _ptr(W3), _ptr(b3), _ptr(skip2), _ptr(o_old), 1, B, H, W, C, 0, st),
              "out_conv")

    def mid_new():
        check(lib.wm_lfss_mid_rz_tok_fwd(*head, _ptr(t_new), B, L, C, 0, st), "mid_rz_tok")

    def ffn(rows=0):
        check(lib.wm_lfss_ffn_fwd(_ptr(t_new), _ptr(ln2w), _ptr(ln2b), 1e-5, _ptr(W1), _ptr(b1), _ptr(cw), _ptr(cb), _ptr(W3), _ptr(b3),
                                  _ptr(skip2), _ptr(o_new), 1, B, H, W, C, 0, rows, st), "ffn")

    def old():
        mid_old(); out_old()

    def new():
        mid_new(); ffn()
    for _ in range(3):
        old(); new()
    t = {k: [] for k in ("old", "new", "mid_old", "mid_new", "out_old", "ffn")}
    for _ in range(args.reps):
        t["old"].append(timed(old)); t["new"].append(timed(new))
    for _ in range(args.reps):
        t["mid_old"].append(timed(mid_old)); t["mid_new"].append(timed(mid_new))
        t["out_old"].append(timed(out_old)); t["ffn"].append(timed(ffn))
    same = torch.equal(t_old, t_new) and torch.equal(o_old, o_new)
    print(f"level {lvl} {H}x{W} (band {rb:2d} rows): old pair {row(t['old'])} ms | new pair {row(t['new'])} ms | "
          f"new slowest < old fastest: {max(t['new']) < min(t['old'])} | bit-identical: {same}")
    print(f"    mid_rz {row(t['mid_old'])} -> mid_rz_tok {row(t['mid_new'])} ms | out_conv {row(t['out_old'])} -> ffn {row(t['ffn'])} ms "
          f"({256 * L / statistics.median(t['ffn']) / 1e6:5.0f} GB/s on 256 B per position)", flush=True)
    for rows in forced:
        o_new.fill_(float("nan"))
        ffn(rows)
        tr = [timed(lambda: ffn(rows)) for _ in range(args.reps)]
        print(f"    band height {rows:3d}: ffn {row(tr)} ms | bit-identical: {torch.equal(o_old, o_new)}", flush=True)
