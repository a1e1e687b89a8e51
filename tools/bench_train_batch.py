#!/usr/bin/env python3
"""Forming a training batch (B = 8, P = 512) from UHD-sized (2160 x 3840) uint8 image pairs, three ways, per mode class
(identity = mode 0, mirror = mode 4, transpose = mode 2):

    (a) hip    data.PairedPatchBatcher.form on a DeviceImageStore: one launch of csrc/patch_batch.hip.h (table update included;
               `hip_kernel_ms` is the launch alone on a table already written)
    (b) torch  the PyTorch spelling on the device from the same resident images: index the window, flip / rot90, flip the
               channels, permute, float, divide by 255, stack
    (c) host   the reference's way on the CPU, restated with numpy on whole float32 images (uint8 -> float32 / 255 of the whole
               image, crop, flip / rot90 + copy, BGR -> RGB, CHW), the samples of a batch on a pool of --workers threads
               (16: what a job on the pool is granted - never os.cpu_count()), then stack + upload

(a) and (b) are timed with device events after a warm-up, (c) with the wall clock around the batch (it ends in a synchronised
upload).  Each result is compared with cpu_twin.paired_patches bit for bit (`bit_equal_to_twin`; ATen divides by a scalar on the
device by multiplying with its reciprocal, so (b) may differ from uint8 / 255 in the last bit).  For (a) the achieved fraction
of the bytes-moved bound is reported: 2 B P^2 (3 bytes read + 12 written) at --hbm-gbs.  GPU only.  Writes one JSON line per mode class to stdout and, with --out, to that file.

    python tools/bench_train_batch.py [--iters 50] [--images 4] [--out profiles/train_batch/bench.jsonl]"""
import argparse
import concurrent.futures
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wave_mamba_amd as wm
from wave_mamba_amd import cpu_twin, data

H, W, B, P = 2160, 3840, 8, 512


def time_ms(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def wall_ms(fn, iters, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iters


def torch_sample(img, top, left, mode):
    a = img[top:top + P, left:left + P]
    k, flip = mode // 2, mode % 2                      # data_augmentation: rot90 k times, then flipud for the odd modes
    if k:
        a = torch.rot90(a, k, (0, 1))
    if flip:
        a = a.flip(0)
    return a.flip(-1).permute(2, 0, 1).float() / 255.0


def host_sample(img, top, left, mode):
    a = img.astype(np.float32) / 255.                  # imfrombytes(float32=True): the whole image
    a = a[top:top + P, left:left + P]
    k, flip = mode // 2, mode % 2
    if k:
        a = np.rot90(a, k)
    if flip:
        a = np.flipud(a)
    a = a.copy() if mode else a                        # random_augmentation's .copy() of the view
    return torch.from_numpy(np.ascontiguousarray(a[..., ::-1].transpose(2, 0, 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--images", type=int, default=4, help="UHD pairs in the store (49.8 MB each)")
    ap.add_argument("--workers", type=int, default=16, help="threads of the host restatement: the cores a job is granted")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM bandwidth the bound is stated against (MI355X: 8 TB/s peak)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    pairs = [(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
             for _ in range(args.images)]
    store = data.DeviceImageStore(dev)
    for p in pairs:
        store.add(*p)
    batcher = data.PairedPatchBatcher(store, gt_size=P, seed=0)
    pool = concurrent.futures.ThreadPoolExecutor(args.workers)
    bound_ms = 1e3 * 2 * B * P * P * (3 + 12) / (args.hbm_gbs * 1e9)
    lines = []
    for cls, mode in (("identity", 0), ("mirror", 4), ("transpose", 2)):
        rows = [(k % args.images, t, l, mode) for k, (_, t, l, _) in enumerate(batcher.draw([0] * B))]
        out = (torch.empty(B, 3, P, P, device=dev), torch.empty(B, 3, P, P, device=dev))

        def hip():
            batcher.form(rows=rows, out=out)

        def hip_kernel():
            wm.ops.paired_patches_u8(batcher.table, P, out=out)

        def torch_dev():
            lq = torch.stack([torch_sample(store.pair(i)[0], t, l, m) for i, t, l, m in rows])
            gt = torch.stack([torch_sample(store.pair(i)[1], t, l, m) for i, t, l, m in rows])
            return lq, gt

        def host():
            jobs = [(pairs[i][k], t, l, m) for k in (0, 1) for i, t, l, m in rows]
            done = list(pool.map(lambda j: host_sample(*j), jobs))
            return torch.stack(done[:B]).to(dev), torch.stack(done[B:]).to(dev)
        hip()
        want = cpu_twin.paired_patches(pairs, rows, P)
        equal = {name: all(torch.equal(g.cpu(), w) for g, w in zip(got, want))
                 for name, got in (("hip", out), ("torch_device", torch_dev()), ("host", host()))}
        torch_dev_max_abs = max(float((g.cpu() - w).abs().max()) for g, w in zip(torch_dev(), want))
        res = {"what": f"train batch {B}x3x{P}x{P} from {H}x{W} uint8, {cls} (mode {mode})", "build_id": wm._lib.build_id(),
               "hip_ms": round(time_ms(hip, args.iters), 4), "hip_kernel_ms": round(time_ms(hip_kernel, args.iters), 4),
               "torch_device_ms": round(time_ms(torch_dev, args.iters), 4),
               "host_ms": round(wall_ms(host, args.host_iters), 2), "host_workers": args.workers,
               "bytes_moved_bound_ms": round(bound_ms, 5), "hbm_gbs_assumed": args.hbm_gbs, "bit_equal_to_twin": equal,
               "torch_device_max_abs_diff": torch_dev_max_abs}
        res["hip_kernel_fraction_of_bound"] = round(bound_ms / res["hip_kernel_ms"], 3)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
