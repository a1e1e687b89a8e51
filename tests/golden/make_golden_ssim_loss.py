#!/usr/bin/env python3
"""Generate tests/golden/ssim_loss.npz: the reference's SSIM training loss (basicsr/models/cal_ssim.py, SSIM()) on seeded
float image pairs - its float32 value and gradients, and the same module evaluated in float64 (the truth).

TEST INFRASTRUCTURE - runs ONLY where the reference tree is mounted read-only at /root/reference (as make_golden.py).  The
fixture is data only.  cal_ssim.py imports torch and numpy alone, so it is loaded by path as it is.

Cases: `cases` lists "<kind>_<B>x<C>x<H>x<W>".  Kinds (seeded torch.Generators, one per case):
  noise      gt uniform in [0, 1), pred = clamp(gt + 0.1 N, 0, 1)
  smooth     gt = 7x7 box blur of uniform noise, pred = clamp(gt + 0.1 N, 0, 1)
  flat       gt: upper half 0.9, lower half 0.02; pred = clamp(gt + 0.02 N, 0, 1)   (the cancellation case: e11 - mu1^2 ~ 0)
  dark       gt = 0.05 * uniform, pred = clamp(gt + 0.1 * 0.05 N, 0, 1)
  unclamped  gt uniform, pred = gt + 0.5 N (values outside [0, 1])
  equal      gt uniform, pred = gt

Per case <c>:
  <c>.pred, <c>.gt                 float32 (B, C, H, W)      (`equal`: .gt only)
  <c>.ssim32, <c>.ssim64           the reference's value in float32 / float64
  <c>.gpred64, <c>.ggt64           d SSIM / d pred, d SSIM / d gt in float64   (not for `equal` above 1,000 elements)
  <c>.gpred32, <c>.ggt32           the same from the float32 run                (shapes of at most 1,000 elements)
  <c>.err32                        (6,) float64: the float32 run against the truth - |ssim32 - ssim64|, then (l2-relative,
                                   max-abs-relative) of gpred32 and of ggt32, then max |gpred32| (what `equal` is held against)

All six kinds are kept at the three small shapes.  The two multi-tile shapes hold incompressible noise - 32 bytes per element in
the full form, 1 MB for ONE (2, 3, 40, 130) case - so they carry the kinds that matter most there and leave the float32
gradients to err32: (2, 3, 33, 47) noise and equal, (2, 3, 40, 130) flat.  The file stays under 1 MB.

Usage:  python tests/golden/make_golden_ssim_loss.py
"""
import importlib.util
import os

import numpy as np
import torch
import torch.nn.functional as F

REF_ROOT = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ssim_loss.npz")
KINDS = ("noise", "smooth", "flat", "dark", "unclamped", "equal")
SMALL = [(1, 1, 5, 7), (1, 2, 1, 30), (1, 3, 11, 11)]
LARGE = {(2, 3, 33, 47): ("noise", "equal"), (2, 3, 40, 130): ("flat",)}
FULL_FORM_MAX = 1000


def load_reference():
    spec = importlib.util.spec_from_file_location("cal_ssim", os.path.join(REF_ROOT, "basicsr", "models", "cal_ssim.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def make_pair(kind, shape, seed):
    g = torch.Generator().manual_seed(seed)
    B, C, H, W = shape
    u = torch.rand(shape, generator=g)
    n = torch.randn(shape, generator=g)
    if kind == "noise":
        gt, pred = u, (u + 0.1 * n).clamp(0, 1)
    elif kind == "smooth":
        gt = F.avg_pool2d(F.pad(u, (3, 3, 3, 3), mode="replicate"), 7, stride=1)
        pred = (gt + 0.1 * n).clamp(0, 1)
    elif kind == "flat":
        gt = torch.full(shape, 0.02)
        gt[:, :, : (H + 1) // 2] = 0.9
        pred = (gt + 0.02 * n).clamp(0, 1)
    elif kind == "dark":
        gt = 0.05 * u
        pred = (gt + 0.005 * n).clamp(0, 1)
    elif kind == "unclamped":
        gt, pred = u, u + 0.5 * n
    elif kind == "equal":
        gt, pred = u, u.clone()
    else:
        raise ValueError(kind)
    return pred.contiguous(), gt.contiguous()


def evaluate(ref, pred, gt, dtype):
    a = pred.detach().clone().to(dtype).requires_grad_(True)
    b = gt.detach().clone().to(dtype).requires_grad_(True)
    s = ref.SSIM()(a, b)                       # a fresh module per call: its cached window follows the dtype
    s.backward()
    return s.detach(), a.grad, b.grad


def rel(a, t):
    a, t = a.double(), t.double()
    return float((a - t).norm() / t.norm().clamp_min(1e-300)), float((a - t).abs().max() / t.abs().max().clamp_min(1e-300))


def main():
    ref = load_reference()
    out, names = {}, []
    todo = [(k, s) for s in SMALL for k in KINDS] + [(k, s) for s, ks in LARGE.items() for k in ks]
    for i, (kind, shape) in enumerate(todo):
        name = f"{kind}_{'x'.join(map(str, shape))}"
        pred, gt = make_pair(kind, shape, 20261018 + i)
        s32, ga32, gb32 = evaluate(ref, pred, gt, torch.float32)
        s64, ga64, gb64 = evaluate(ref, pred, gt, torch.float64)
        assert s32.dtype == torch.float32 and s64.dtype == torch.float64
        names.append(name)
        small = pred.numel() <= FULL_FORM_MAX
        out[f"{name}.gt"] = gt.numpy()
        if kind != "equal":
            out[f"{name}.pred"] = pred.numpy()
        out[f"{name}.ssim32"], out[f"{name}.ssim64"] = s32.numpy(), s64.numpy()
        if kind != "equal" or small:
            out[f"{name}.gpred64"], out[f"{name}.ggt64"] = ga64.numpy(), gb64.numpy()
        if small:
            out[f"{name}.gpred32"], out[f"{name}.ggt32"] = ga32.numpy(), gb32.numpy()
        out[f"{name}.err32"] = np.array([abs(float(s32) - float(s64)), *rel(ga32, ga64), *rel(gb32, gb64), float(ga32.abs().max())])
        print(f"{name:28s} ssim64 {float(s64):+.9f}  err32: value {out[f'{name}.err32'][0]:.2e}  "
              f"gpred l2 {out[f'{name}.err32'][1]:.2e} max {out[f'{name}.err32'][2]:.2e}  "
              f"ggt l2 {out[f'{name}.err32'][3]:.2e} max {out[f'{name}.err32'][4]:.2e}  max|gpred32| {out[f'{name}.err32'][5]:.2e}")
    out["cases"] = np.array(names)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 1_000_000, size
    print(f"wrote {OUT} ({size} bytes, {len(names)} cases)")


if __name__ == "__main__":
    main()
