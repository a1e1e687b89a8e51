"""The reference's image-quality metrics (comput_psnr_ssim.py, as inference_wavemamba.py:116-117 calls them): PSNR and SSIM on
the BT.601 Y channel of uint8 BGR images, after cropping `crop_border` pixels from every edge.

    calculate_psnr(img1, img2, crop_border=1, input_order='HWC', test_y_channel=True)
    calculate_ssim(img1, img2, crop_border=1, input_order='HWC', test_y_channel=True)

CUDA uint8 tensors go to the HIP kernels (ops.psnr_ssim_y); numpy arrays and CPU tensors go to the float64 restatement below,
which is also what the GPU tests compare the kernels against.  Definition (pinned by tests/golden/metrics.npz):
  crop    img[c:-c, c:-c] (:426-428, :642-644); c = 0: none
  Y       x = float32(img) / 255 in float32; y64 = ((x_b 24.966 + x_g 128.553) + x_r 65.481) + 16 in float64;
          Y = float32(float32(y64 / 255) * 255)  (to_y_channel :374-385 -> bgr2ycbcr :210-237)
  PSNR    20 log10(255 / sqrt(mean((Y1 - Y2)^2))), inf for mse = 0 (:430-438).  The mean is float64 here; the reference forms it
          in float32 (its Y planes are float32): ~5e-6 dB apart at UHD.
  SSIM    float64 Y; 11 x 11 Gaussian window (sigma 1.5) applied with a replicated border, same size; C1 = (0.01 255)^2,
          C2 = (0.03 255)^2; the mean of the SSIM map (_ssim_cly :558-593).  Filtered separably here (11 taps along rows, then
          along columns): ~1e-15 from the reference's 2-D filter.

Differences from the reference: torch tensors are read in `input_order` (the reference's tensor branch assumes CHW and then
applies input_order again); on CUDA a batch (N, ...) with N > 1 returns an (N,) float64 CUDA tensor instead of a float.
Out of scope: SSIM without the Y channel (the reference's _ssim_3d, :522-556, a float32 3-D Gaussian on CUDA) raises
NotImplementedError; PSNR without the Y channel is computed by the CPU restatement only.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

C1 = (0.01 * 255) ** 2
C2 = (0.03 * 255) ** 2


def gaussian_window(n=11, sigma=1.5):
    """cv2.getGaussianKernel(n, sigma) for sigma > 0 as a float64 vector: exp(-0.5 / sigma^2 * x * x), x = i - (n - 1) / 2,
    normalised by multiplying with 1 / sum."""
    x = torch.arange(n, dtype=torch.float64) - (n - 1) * 0.5
    k = torch.exp(-0.5 / (sigma * sigma) * x * x)
    return k * (1.0 / k.sum())


def _check_order(input_order):
    if input_order not in ("HWC", "CHW"):
        raise ValueError(f'Wrong input_order {input_order}. Supported input_orders are "HWC" and "CHW"')


def _hwc64(img, input_order):
    """numpy array / CPU tensor (H, W, C), (C, H, W) or (1, ...) -> float64 (H, W, C) tensor (reorder_image + astype)."""
    t = img.detach().cpu() if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img))
    if t.dim() == 4:
        if t.shape[0] != 1:
            raise ValueError(f"expected one image, got a batch of {t.shape[0]}")
        t = t[0]
    if t.dim() == 2:
        t = t[..., None]
    elif input_order == "CHW":
        t = t.permute(1, 2, 0)
    return t.double()


def _crop(t, c):
    if c < 0 or t.shape[0] - 2 * c < 1 or t.shape[1] - 2 * c < 1:
        raise ValueError(f"crop_border {c} leaves nothing of a {t.shape[0]} x {t.shape[1]} image")
    return t[c:-c, c:-c] if c else t


def y_channel(img, bgr=True):
    """to_y_channel of an (H, W, 3) image with values in [0, 255] (numpy or tensor, HWC) -> float32 (H, W) tensor."""
    t = img if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img))
    x = t.cpu().float() / 255.0
    xb, xg, xr = (x[..., 0], x[..., 1], x[..., 2]) if bgr else (x[..., 2], x[..., 1], x[..., 0])
    y64 = ((xb.double() * 24.966 + xg.double() * 128.553) + xr.double() * 65.481) + 16.0
    return (y64 / 255.0).float() * 255.0


def _psnr(a, b, max_value=255.0):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return float("inf") if mse == 0 else 20.0 * math.log10(max_value / math.sqrt(mse))


def _filter(p, h, w, g):
    """Replicate-padded (h + 10, w + 10) float64 plane -> (h, w): the 11 x 11 window outer(g, g), rows then columns."""
    n = g.numel()
    r = g[0] * p[:, 0:w]
    for t in range(1, n):
        r = r + g[t] * p[:, t:t + w]
    c = g[0] * r[0:h]
    for t in range(1, n):
        c = c + g[t] * r[t:t + h]
    return c


def ssim_plane(y1, y2):
    """_ssim_cly of two (H, W) planes, in float64 -> float."""
    y1, y2 = y1.double(), y2.double()
    h, w = y1.shape
    g = gaussian_window()
    pad = g.numel() // 2
    p1 = F.pad(y1[None, None], (pad, pad, pad, pad), mode="replicate")[0, 0]
    p2 = F.pad(y2[None, None], (pad, pad, pad, pad), mode="replicate")[0, 0]
    mu1, mu2 = _filter(p1, h, w, g), _filter(p2, h, w, g)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 ** 2, mu2 ** 2, mu1 * mu2
    sigma1_sq = _filter(p1 * p1, h, w, g) - mu1_sq
    sigma2_sq = _filter(p2 * p2, h, w, g) - mu2_sq
    sigma12 = _filter(p1 * p2, h, w, g) - mu1_mu2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    return float(ssim_map.mean())


def psnr_ssim_y_cpu(img1, img2, crop_border=1, input_order="HWC", bgr=True):
    """The float64 restatement: (Y PSNR, Y SSIM) of one image pair given as numpy arrays or CPU tensors."""
    _check_order(input_order)
    a, b = _hwc64(img1, input_order), _hwc64(img2, input_order)
    if a.shape != b.shape:
        raise ValueError(f"Image shapes are different: {tuple(a.shape)}, {tuple(b.shape)}.")
    y1, y2 = y_channel(_crop(a, crop_border), bgr), y_channel(_crop(b, crop_border), bgr)
    return _psnr(y1, y2), ssim_plane(y1, y2)


def _on_gpu(img1, img2):
    g1 = isinstance(img1, torch.Tensor) and img1.is_cuda
    g2 = isinstance(img2, torch.Tensor) and img2.is_cuda
    if g1 != g2:
        raise RuntimeError("calculate_psnr / calculate_ssim: one image is a CUDA tensor and the other is not")
    return g1


def _gpu(img1, img2, crop_border, input_order, col):
    from . import ops
    out = ops.psnr_ssim_y(img1, img2, crop_border, layout=input_order)[:, col]
    return float(out[0]) if out.shape[0] == 1 else out


def calculate_psnr(img1, img2, crop_border=1, input_order="HWC", test_y_channel=True):
    """PSNR in dB (comput_psnr_ssim.calculate_psnr).  Images in [0, 255], BGR; see the module docstring."""
    _check_order(input_order)
    if _on_gpu(img1, img2):
        if not test_y_channel:
            raise NotImplementedError("calculate_psnr: test_y_channel=False is computed on the CPU only (pass numpy arrays "
                                      "or CPU tensors)")
        return _gpu(img1, img2, crop_border, input_order, 0)
    if test_y_channel:
        return psnr_ssim_y_cpu(img1, img2, crop_border, input_order)[0]
    a, b = _hwc64(img1, input_order), _hwc64(img2, input_order)
    if a.shape != b.shape:
        raise ValueError(f"Image shapes are different: {tuple(a.shape)}, {tuple(b.shape)}.")
    a, b = _crop(a, crop_border), _crop(b, crop_border)
    return _psnr(a, b, 1.0 if float(a.max()) <= 1 else 255.0)


def calculate_ssim(img1, img2, crop_border=1, input_order="HWC", test_y_channel=True):
    """SSIM of the Y channel (comput_psnr_ssim.calculate_ssim with test_y_channel=True).  See the module docstring."""
    _check_order(input_order)
    if not test_y_channel:
        raise NotImplementedError("calculate_ssim: only the Y-channel SSIM is implemented; the reference's 3-channel path "
                                  "(_ssim_3d, comput_psnr_ssim.py:522-556) is out of scope")
    if _on_gpu(img1, img2):
        return _gpu(img1, img2, crop_border, input_order, 1)
    return psnr_ssim_y_cpu(img1, img2, crop_border, input_order)[1]
