#!/usr/bin/env python3
"""The SSIM training loss (ops.ssim_mean, csrc/ssim_loss.hip.h) at the training batch, 8 x 3 x 512 x 512: forward + backward
(gradient for the prediction, as in training) on the HIP kernels against the ATen composition of the same definition (five
depth-wise 11 x 11 conv2d calls and the element-wise map, fp32, autograd) - ms from device events, kernel launches from
torch.profiler (all of the loss expression, and the ssim_loss kernels among them) - and, with --step, the BASELINE config-3 training step with ssim_weight=0.25 against ssim_weight=None.  GPU only.

    python tools/bench_ssim_loss.py [--iters 50] [--step]
Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wave_mamba_amd as wm
from wave_mamba_amd import cpu_twin


def aten_ssim(a, b, window):
    C = a.shape[1]
    blur = lambda t: F.conv2d(t, window, padding=5, groups=C)
    mu1, mu2 = blur(a), blur(b)
    s1, s2, s12 = blur(a * a) - mu1 * mu1, blur(b * b) - mu2 * mu2, blur(a * b) - mu1 * mu2
    return (((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * (s1 + s2 + 9e-4))).mean()


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


def launches(fn):
    from torch.profiler import profile, ProfilerActivity
    from torch.autograd import DeviceType
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]
    return len(names), sum("ssim_loss" in n for n in names)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--step", action="store_true", help="also time the config-3 training step with and without the SSIM term")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1234)
    gt = torch.rand(8, 3, 512, 512, generator=g).to(dev)
    pred = (gt + 0.1 * torch.randn(8, 3, 512, 512, generator=g).to(dev)).clamp(0, 1).requires_grad_(True)
    g1 = cpu_twin.ssim_window_1d()
    window = torch.outer(g1, g1).expand(3, 1, 11, 11).contiguous().to(dev)

    def hip():
        pred.grad = None
        (1 - wm.ops.ssim_mean(pred, gt)).backward()

    def hip_fwd():
        with torch.no_grad():
            wm.ops.ssim_mean(pred, gt)

    def aten():
        pred.grad = None
        (1 - aten_ssim(pred, gt, window)).backward()
    hip()
    g_hip, s_hip = pred.grad.clone(), float(wm.ops.ssim_mean(pred, gt))
    aten()
    g_aten, s_aten = pred.grad.clone(), float(aten_ssim(pred, gt, window))
    n_hip, n_own = launches(hip)
    n_aten, _ = launches(aten)
    res = {"what": "ssim_loss fwd+bwd 8x3x512x512", "build_id": wm._lib.build_id(), "hip_ms": round(time_ms(hip, args.iters), 4),
           "hip_fwd_only_ms": round(time_ms(hip_fwd, args.iters), 4), "aten_ms": round(time_ms(aten, args.iters), 4),
           "hip_launches": n_hip, "hip_launches_ssim_kernels": n_own, "aten_launches": n_aten,
           "ssim_hip": s_hip, "ssim_aten": s_aten,
           "grad_rel_max_vs_aten": float((g_hip - g_aten).abs().max() / g_aten.abs().max())}
    print(json.dumps(res), flush=True)
    if args.step:
        import bench
        lq = torch.rand(8, 3, 512, 512, generator=g).to(dev)
        out = {"what": "config-3 train_step, eager", "build_id": wm._lib.build_id()}
        for name, weight in (("none", None), ("ssim_0.25", 0.25), ("none_again", None)):
            torch.manual_seed(0)
            net = wm.WaveMamba(**bench.SHIPPED).train().to(dev)
            opt = wm.trainer.make_optimizer(net)
            out[f"step_ms_{name}"] = round(time_ms(lambda: wm.trainer.train_step(net, opt, lq, gt, as_float=False, ssim_weight=weight),
                                                   10, warmup=3), 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
