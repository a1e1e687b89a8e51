#!/usr/bin/env python3
"""Generate tests/golden/metrics.npz: the reference's own PSNR / SSIM / Y-channel values on seeded uint8 image pairs.

TEST INFRASTRUCTURE - runs ONLY where the reference tree is mounted read-only at /root/reference (as make_golden.py).  The
fixture is data only: image pairs, the values the reference computes for them, two Y planes and one hash.

How the import works: comput_psnr_ssim.py imports cv2, skimage and basicsr.utils.matlab_functions.  sys.modules is seeded with
  * empty package shells `basicsr`, `basicsr.utils` and the reference's own `basicsr/utils/matlab_functions.py` loaded by path
    (numpy + torch only): bgr2ycbcr, which to_y_channel calls, is the reference's real code;
  * an empty `skimage` (only the 3-channel SSIM path, which is not exercised, would use it);
  * a `cv2` stand-in with getGaussianKernel (OpenCV's formula for sigma > 0: exp(-0.5 / sigma^2 * x * x), normalised) and
    filter2D (BORDER_REPLICATE pad, then a float64 F.conv2d - a 2-D correlation, as filter2D is).
PSNR and the Y chain therefore run entirely on the reference's code; only SSIM's filter is the stand-in.

Contents:
  a{i}, b{i}             uint8 (H, W, 3) BGR pairs: 37x53, 64x96, 9x7, 5x300 (seeded) and one identical 31x45 pair
  crops                  (0, 1, 4)
  psnr_y, psnr_rgb, ssim_y   (cases, crops) float64: calculate_psnr(test_y_channel=True / False), calculate_ssim(True);
                         nan where the crop leaves no pixel
  y_a0, y_b0             to_y_channel of pair 0 (no crop), float32 (H, W)
  y_all_sha256           sha256 of the reference's float32 Y over the 4096 x 4096 image of every BGR triple (pixel v row-major:
                         b, g, r = v % 256, v // 256 % 256, v // 65536), little-endian float32 bytes (the 32-byte digest as uint8)

Usage:  python tests/golden/make_golden_metrics.py
"""
import hashlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

REF_ROOT = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "metrics.npz")
SHAPES = [(37, 53), (64, 96), (9, 7), (5, 300)]
IDENTICAL = (31, 45)
CROPS = (0, 1, 4)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def import_reference_metrics():
    for p in ("basicsr", "basicsr.utils"):
        m = types.ModuleType(p)
        m.__path__ = []
        sys.modules[p] = m
    _load("basicsr.utils.matlab_functions", os.path.join(REF_ROOT, "basicsr", "utils", "matlab_functions.py"))

    cv2 = types.ModuleType("cv2")
    cv2.BORDER_REPLICATE = 1

    def get_gaussian_kernel(n, sigma):
        x = np.arange(n, dtype=np.float64) - (n - 1) * 0.5
        k = np.exp(-0.5 / (sigma * sigma) * x * x)
        return (k * (1.0 / k.sum())).reshape(n, 1)

    def filter2d(img, ddepth, kernel, borderType=None):
        assert borderType == cv2.BORDER_REPLICATE and img.dtype == np.float64
        kh, kw = kernel.shape
        t = F.pad(torch.from_numpy(np.ascontiguousarray(img))[None, None], (kw // 2, kw // 2, kh // 2, kh // 2), mode="replicate")
        return F.conv2d(t, torch.from_numpy(np.ascontiguousarray(kernel))[None, None]).numpy()[0, 0]

    cv2.getGaussianKernel, cv2.filter2D = get_gaussian_kernel, filter2d
    sys.modules["cv2"] = cv2
    sk = types.ModuleType("skimage")
    sk.metrics = types.ModuleType("skimage.metrics")
    sys.modules["skimage"], sys.modules["skimage.metrics"] = sk, sk.metrics
    return _load("comput_psnr_ssim", os.path.join(REF_ROOT, "comput_psnr_ssim.py"))


def all_triples_image():
    v = np.arange(256 ** 3, dtype=np.int64)
    return np.stack([v % 256, v // 256 % 256, v // 65536], -1).astype(np.uint8).reshape(4096, 4096, 3)


def main():
    ref = import_reference_metrics()
    rng = np.random.default_rng(20261016)
    pairs = []
    for h, w in SHAPES:
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        b = np.clip(a.astype(np.int64) + rng.integers(-24, 25, a.shape), 0, 255).astype(np.uint8)
        pairs.append((a, b))
    a = rng.integers(0, 256, IDENTICAL + (3,), dtype=np.uint8)
    pairs.append((a, a.copy()))

    out = {"crops": np.array(CROPS, dtype=np.int64)}
    psnr_y = np.full((len(pairs), len(CROPS)), np.nan)
    psnr_rgb, ssim_y = psnr_y.copy(), psnr_y.copy()
    for i, (a, b) in enumerate(pairs):
        out[f"a{i}"], out[f"b{i}"] = a, b
        for j, c in enumerate(CROPS):
            if a.shape[0] - 2 * c < 1 or a.shape[1] - 2 * c < 1:
                continue
            psnr_y[i, j] = ref.calculate_psnr(a, b, crop_border=c, test_y_channel=True)
            psnr_rgb[i, j] = ref.calculate_psnr(a, b, crop_border=c, test_y_channel=False)
            ssim_y[i, j] = ref.calculate_ssim(a, b, crop_border=c, test_y_channel=True)
    out["psnr_y"], out["psnr_rgb"], out["ssim_y"] = psnr_y, psnr_rgb, ssim_y
    a, b = pairs[0]
    out["y_a0"] = ref.to_y_channel(a.astype(np.float64))[..., 0]
    out["y_b0"] = ref.to_y_channel(b.astype(np.float64))[..., 0]
    assert out["y_a0"].dtype == np.float32

    y = ref.to_y_channel(all_triples_image().astype(np.float64))[..., 0]
    assert y.dtype == np.float32 and y.shape == (4096, 4096)
    out["y_all_sha256"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(y).astype("<f4").tobytes()).digest(), np.uint8)

    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes); psnr_y\n{psnr_y}\nssim_y\n{ssim_y}")


if __name__ == "__main__":
    main()
