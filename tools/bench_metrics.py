#!/usr/bin/env python3
"""Time of the Y-channel PSNR / SSIM kernels (ops.psnr_ssim_y, csrc/metrics.hip.h) on one UHD uint8 pair and on a batch of 8,
from device events after warm-up; bytes and fp64 FLOPs computed from the shape; the float64 CPU restatement
(metrics.psnr_ssim_y_cpu) timed on the same pair for context.  GPU only.

    python tools/bench_metrics.py [--iters 20] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wave_mamba_amd as wm                     # noqa: E402
from wave_mamba_amd import metrics              # noqa: E402

TW, TH, HALO, TAPS = 32, 24, 5, 11              # csrc/metrics.hip.h: MET_TW, MET_TH, MET_HALO, MET_TAPS


def work(n, h, w, crop):
    """(bytes read from the images once, fp64 FLOPs the kernels execute) for n pairs of h x w."""
    hc, wc = h - 2 * crop, w - 2 * crop
    tiles_y, tiles_x = -(-hc // TH), -(-wc // TW)
    row_px = tiles_y * (TH + 2 * HALO) * tiles_x * TW          # row filter runs over the halo rows too
    out_px = hc * wc
    flops = n * (row_px * (3 + 5 * 2 * TAPS)                   # three products, five 11-tap FMA chains
                 + out_px * (5 * 2 * TAPS + 17)                # five 11-tap column chains, the SSIM map
                 + out_px * 3)                                 # (Y1 - Y2)^2 accumulated
    return 2 * n * h * w * 3, flops


def time_gpu(a, b, iters):
    for _ in range(3):
        wm.ops.psnr_ssim_y(a, b)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        wm.ops.psnr_ssim_y(a, b)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics: needs a GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    h, w = 2160, 3840
    a = rng.integers(0, 256, (8, h, w, 3), dtype=np.uint8)
    b = np.clip(a.astype(np.int16) + rng.integers(-12, 13, a.shape, dtype=np.int16), 0, 255).astype(np.uint8)
    ga, gb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    res = {}
    for n in (1, 8):
        ms = time_gpu(ga[:n], gb[:n], args.iters)
        nbytes, flops = work(n, h, w, 1)
        res[f"uhd_x{n}"] = {"ms": round(ms, 4), "ms_per_image": round(ms / n, 4), "image_bytes": nbytes,
                            "fp64_flops": flops, "image_GBps": round(nbytes / ms / 1e6, 1),
                            "fp64_TFLOPs": round(flops / ms / 1e9, 2)}
    got = wm.ops.psnr_ssim_y(ga[:1], gb[:1]).cpu()[0].tolist()
    res["uhd_psnr_ssim"] = got
    if not args.no_cpu:
        t0 = time.perf_counter()
        ref = metrics.psnr_ssim_y_cpu(a[0], b[0], 1)
        res["cpu_restatement_s"] = round(time.perf_counter() - t0, 3)
        res["abs_diff_vs_cpu"] = [abs(got[0] - ref[0]), abs(got[1] - ref[1])]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
