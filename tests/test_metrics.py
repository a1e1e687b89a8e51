"""Y-channel PSNR / SSIM (wave_mamba_amd.metrics, ops.psnr_ssim_y, csrc/metrics.hip.h) against the reference's own values
(tests/golden/metrics.npz, made by make_golden_metrics.py from comput_psnr_ssim.py) and against the float64 restatement.

CPU: the restatement vs the golden values, the Y chain over every BGR triple, the Python and C-ABI argument checks.
GPU: the HIP kernels vs the golden values and the restatement (odd sizes, planes below the 11 x 11 window, HWC / CHW, BGR / RGB,
UHD), determinism, graph capture, error codes, and UInt8Pipeline.run(images, targets)."""
import ctypes
import hashlib
import math

import numpy as np
import pytest
import torch

import wave_mamba_amd as wm
from wave_mamba_amd import _lib, inference, metrics

DEV = torch.device("cuda:0")
SSIM_TOL = 1e-10          # vs the reference and vs the restatement
PSNR_Y_REF_TOL = 2e-5     # dB: the reference forms its Y mse in float32, this package in float64
PSNR_TOL = 1e-9           # dB: float64 vs float64 (GPU vs restatement; RGB PSNR vs the reference)


def _cases(golden):
    g = golden("metrics")
    crops = [int(c) for c in g["crops"]]
    n = sum(1 for k in g if k.startswith("a") and k[1:].isdigit())
    for i in range(n):
        for j, c in enumerate(crops):
            if not math.isnan(float(g["ssim_y"][i, j])):
                yield (g[f"a{i}"].numpy(), g[f"b{i}"].numpy(), c, float(g["psnr_y"][i, j]), float(g["psnr_rgb"][i, j]),
                       float(g["ssim_y"][i, j]))


def _close_db(got, ref, tol):
    if math.isinf(ref):
        return math.isinf(got) and got > 0
    return abs(got - ref) <= tol


def _all_triples():
    v = np.arange(256 ** 3, dtype=np.int64)
    return np.stack([v % 256, v // 256 % 256, v // 65536], -1).astype(np.uint8).reshape(4096, 4096, 3)


def _pair(rng, shape, noise=24):
    a = rng.integers(0, 256, shape, dtype=np.uint8)
    b = np.clip(a.astype(np.int64) + rng.integers(-noise, noise + 1, shape), 0, 255).astype(np.uint8)
    return a, b


# ------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------
def test_restatement_matches_reference_values(golden):
    count = 0
    for a, b, c, psnr_y, psnr_rgb, ssim_y in _cases(golden):
        p, s = metrics.psnr_ssim_y_cpu(a, b, c)
        assert _close_db(p, psnr_y, PSNR_Y_REF_TOL), (a.shape, c, p, psnr_y)
        assert abs(s - ssim_y) <= SSIM_TOL, (a.shape, c, s, ssim_y)
        assert metrics.calculate_ssim(a, b, crop_border=c) == s
        assert metrics.calculate_psnr(a, b, crop_border=c) == p
        pr = metrics.calculate_psnr(a, b, crop_border=c, test_y_channel=False)
        assert _close_db(pr, psnr_rgb, PSNR_TOL), (a.shape, c, pr, psnr_rgb)
        count += 1
    assert count == 13


def test_restatement_y_planes_match_reference(golden):
    g = golden("metrics")
    assert torch.equal(metrics.y_channel(g["a0"].numpy()), g["y_a0"])
    assert torch.equal(metrics.y_channel(g["b0"].numpy()), g["y_b0"])
    # CHW input and RGB order reach the same plane
    chw = torch.from_numpy(g["a0"].numpy()).permute(2, 0, 1)
    p, s = metrics.psnr_ssim_y_cpu(chw, torch.from_numpy(g["b0"].numpy()).permute(2, 0, 1), 1, input_order="CHW")
    assert (p, s) == metrics.psnr_ssim_y_cpu(g["a0"].numpy(), g["b0"].numpy(), 1)
    rgb = g["a0"].numpy()[..., ::-1]
    assert torch.equal(metrics.y_channel(rgb, bgr=False), g["y_a0"])


def test_restatement_y_over_every_triple(golden):
    y = metrics.y_channel(_all_triples())
    assert y.dtype == torch.float32 and float(y.min()) == 16.0 and float(y.max()) == 235.0
    assert hashlib.sha256(y.numpy().astype("<f4").tobytes()).digest() == golden("metrics")["y_all_sha256"].numpy().tobytes()


def test_identical_images_cpu():
    a = np.random.default_rng(3).integers(0, 256, (23, 17, 3), dtype=np.uint8)
    for c in (0, 1, 4):
        p, s = metrics.psnr_ssim_y_cpu(a, a.copy(), c)
        assert p == float("inf") and abs(s - 1.0) <= 1e-14


def test_python_argument_checks_cpu():
    a = np.zeros((9, 7, 3), np.uint8)
    with pytest.raises(NotImplementedError, match="_ssim_3d"):
        metrics.calculate_ssim(a, a, test_y_channel=False)
    with pytest.raises(ValueError):
        metrics.calculate_psnr(a, a, input_order="WHC")
    with pytest.raises(ValueError):
        metrics.calculate_ssim(a, np.zeros((9, 8, 3), np.uint8))
    with pytest.raises(ValueError):
        metrics.calculate_psnr(a, a, crop_border=4)          # 9 x 7 minus 4 on each side: nothing left
    with pytest.raises(RuntimeError):
        wm.ops.psnr_ssim_y(torch.from_numpy(a), torch.from_numpy(a))        # CPU tensors never reach the HIP path
    with pytest.raises(RuntimeError):
        wm.ops.y_channel_u8(torch.from_numpy(a))


def test_cabi_metric_argument_checks_return_before_launch():
    lib = _lib.load()
    assert lib.wm_psnr_ssim_y_workspace_bytes(1, 2160, 3840, 1) == 1 * 90 * 120 * 16
    assert lib.wm_psnr_ssim_y_workspace_bytes(2, 9, 7, 3) == 2 * 16
    assert lib.wm_psnr_ssim_y_workspace_bytes(1, 9, 7, 4) == 0                  # crop >= min(H, W) / 2
    assert lib.wm_psnr_ssim_y_workspace_bytes(1, 9, 7, -1) == 0
    args = (0, 0, 0, 0, 1, 9, 7)
    assert lib.wm_psnr_ssim_y_u8(None, None, *args, 4, 1, None, None, 0, None) == _lib.WM_EINVAL
    assert lib.wm_psnr_ssim_y_u8(None, None, *args, 1, 1, None, None, 0, None) == _lib.WM_ENULL
    p = ctypes.c_void_p(1 << 20)                                               # never dereferenced: rejected before launch
    assert lib.wm_psnr_ssim_y_u8(p, p, *args, 1, 1, p, p, 0, None) == _lib.WM_EWORKSPACE
    assert lib.wm_psnr_ssim_y_u8(p, p, *args, 1, 1, ctypes.c_void_p((1 << 20) + 4), p, 64, None) == _lib.WM_EALIGN
    assert lib.wm_y_channel_u8(None, 0, 0, 0, 0, 1, 0, 7, 1, None, None) == _lib.WM_EINVAL
    assert lib.wm_y_channel_u8(None, 0, 0, 0, 0, 1, 9, 7, 1, None, None) == _lib.WM_ENULL


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
def _gpu_batch(a, b, crop, layout="HWC", bgr=True):
    """numpy (N, H, W, 3) pairs -> (N, 2) numpy float64 from the HIP kernels."""
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    if layout == "CHW":
        ta, tb = ta.permute(0, 3, 1, 2).contiguous(), tb.permute(0, 3, 1, 2).contiguous()
    return wm.ops.psnr_ssim_y(ta, tb, crop, layout=layout, bgr=bgr).cpu().numpy()


@pytest.mark.gpu
def test_gpu_y_channel_every_triple_bit_exact(golden):
    img = torch.from_numpy(_all_triples()).to(DEV)
    y = wm.ops.y_channel_u8(img).cpu()
    assert y.shape == (4096, 4096)
    assert hashlib.sha256(y.numpy().astype("<f4").tobytes()).digest() == golden("metrics")["y_all_sha256"].numpy().tobytes()
    g = golden("metrics")
    chw = torch.from_numpy(g["a0"].numpy()).permute(2, 0, 1).contiguous().to(DEV)
    assert torch.equal(wm.ops.y_channel_u8(chw, layout="CHW").cpu(), g["y_a0"])
    rgb = torch.from_numpy(np.ascontiguousarray(g["a0"].numpy()[..., ::-1])).to(DEV)
    assert torch.equal(wm.ops.y_channel_u8(rgb, bgr=False).cpu(), g["y_a0"])


@pytest.mark.gpu
def test_gpu_matches_reference_values(golden):
    for a, b, c, psnr_y, _, ssim_y in _cases(golden):
        (p, s), = _gpu_batch(a[None], b[None], c)
        assert _close_db(p, psnr_y, PSNR_Y_REF_TOL), (a.shape, c, p, psnr_y)
        assert abs(s - ssim_y) <= SSIM_TOL, (a.shape, c, s, ssim_y)
        ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
        assert metrics.calculate_psnr(ta, tb, crop_border=c) == p
        assert metrics.calculate_ssim(ta, tb, crop_border=c) == s


@pytest.mark.gpu
def test_gpu_identical_images():
    a = np.random.default_rng(5).integers(0, 256, (2, 37, 61, 3), dtype=np.uint8)
    for c in (0, 1, 4):
        out = _gpu_batch(a, a.copy(), c)
        assert np.all(np.isposinf(out[:, 0])) and np.all(np.abs(out[:, 1] - 1.0) <= 1e-14)


@pytest.mark.gpu
def test_gpu_matches_restatement_batches():
    rng = np.random.default_rng(11)
    for (h, w) in ((45, 67), (9, 7), (5, 300), (300, 5), (64, 96), (11, 11), (25, 33)):
        a, b = _pair(rng, (3, h, w, 3), noise=40)
        for crop in (0, 1, 2):
            if h - 2 * crop < 1 or w - 2 * crop < 1:
                continue
            for layout in ("HWC", "CHW"):
                for bgr in (True, False):
                    got = _gpu_batch(a, b, crop, layout, bgr)
                    for n in range(3):
                        ia, ib = (a[n], b[n]) if bgr else (a[n][..., ::-1], b[n][..., ::-1])
                        p, s = metrics.psnr_ssim_y_cpu(ia, ib, crop)
                        what = (h, w, crop, layout, bgr, n)
                        assert abs(got[n, 0] - p) <= PSNR_TOL, (what, got[n, 0], p)
                        assert abs(got[n, 1] - s) <= SSIM_TOL, (what, got[n, 1], s)


@pytest.mark.gpu
@pytest.mark.parametrize("h", [2160, 2176])
def test_gpu_matches_restatement_uhd(h):
    rng = np.random.default_rng(h)
    base = rng.integers(0, 256, (h // 16, 3840 // 16, 3), dtype=np.uint8)
    a = np.repeat(np.repeat(base, 16, 0), 16, 1)                           # smooth regions and sharp edges
    a = np.clip(a.astype(np.int64) + rng.integers(-3, 4, a.shape), 0, 255).astype(np.uint8)
    b = np.clip(a.astype(np.int64) + rng.integers(-12, 13, a.shape), 0, 255).astype(np.uint8)
    (pg, sg), = _gpu_batch(a[None], b[None], 1)
    p, s = metrics.psnr_ssim_y_cpu(a, b, 1)
    assert abs(pg - p) <= PSNR_TOL and abs(sg - s) <= SSIM_TOL, (pg, p, sg, s)


@pytest.mark.gpu
def test_gpu_deterministic_and_graph_capturable():
    rng = np.random.default_rng(7)
    a, b = _pair(rng, (2, 517, 643, 3))
    c, d = _pair(rng, (2, 517, 643, 3), noise=60)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    r1 = wm.ops.psnr_ssim_y(ta, tb)
    r2 = wm.ops.psnr_ssim_y(ta, tb)
    assert torch.equal(r1, r2)
    rcd = wm.ops.psnr_ssim_y(torch.from_numpy(c).to(DEV), torch.from_numpy(d).to(DEV))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        wm.ops.psnr_ssim_y(ta, tb)                                          # warm-up off the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = wm.ops.psnr_ssim_y(ta, tb)
    for rep in range(3):
        graph.replay()
        assert torch.equal(out, r1), rep
        # eager work between replays: other metric calls and an unrelated reduction
        e = wm.ops.psnr_ssim_y(torch.from_numpy(c).to(DEV), torch.from_numpy(d).to(DEV), crop_border=3)
        wm.ops.l1_mean(torch.randn(4096, device=DEV), torch.randn(4096, device=DEV))
        del e
    ta.copy_(torch.from_numpy(c)); tb.copy_(torch.from_numpy(d))           # new contents of the captured inputs
    graph.replay()
    assert torch.equal(out, rcd)


@pytest.mark.gpu
def test_gpu_error_codes():
    a = torch.zeros((1, 9, 7, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="crop_border"):
        wm.ops.psnr_ssim_y(a, a, crop_border=4)
    with pytest.raises(RuntimeError, match="shapes differ"):
        wm.ops.psnr_ssim_y(a, torch.zeros((1, 9, 8, 3), dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="uint8"):
        wm.ops.psnr_ssim_y(a.float(), a.float())
    with pytest.raises(RuntimeError, match="CUDA"):
        wm.ops.psnr_ssim_y(a, a.cpu())
    with pytest.raises(RuntimeError):
        metrics.calculate_psnr(a[0], a[0].cpu())
    with pytest.raises(NotImplementedError):
        metrics.calculate_psnr(a[0], a[0], test_y_channel=False)
    with pytest.raises(RuntimeError):
        wm.ops.psnr_ssim_y(a, a, layout="CHW")                               # (1, 9, 7, 3) is not (N, 3, H, W)
    lib = _lib.load()
    out = torch.empty(2, dtype=torch.float64, device=DEV)
    ws = torch.empty(64, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.wm_psnr_ssim_y_u8(a.data_ptr(), a.data_ptr(), 189, 21, 3, 1, 1, 9, 7, 4, 1, out.data_ptr(), ws.data_ptr(), 64,
                                 st) == _lib.WM_EINVAL
    assert lib.wm_psnr_ssim_y_u8(a.data_ptr(), a.data_ptr(), 189, 21, 3, 1, 1, 9, 7, 1, 1, out.data_ptr(), ws.data_ptr(), 8,
                                 st) == _lib.WM_EWORKSPACE


@pytest.mark.gpu
def test_gpu_uint8_pipeline_with_targets():
    torch.manual_seed(0)
    net = wm.WaveMamba(in_chn=3, wf=8, n_l_blocks=[1, 1, 1], n_h_blocks=[1, 1, 1], ffn_scale=2.0).eval().to(DEV)
    rng = np.random.default_rng(1)
    imgs = [rng.integers(0, 256, size=s, dtype=np.uint8) for s in ((97, 133, 3), (130, 71, 3), (77, 200, 3))]
    tgts = [np.clip(im.astype(np.int64) + rng.integers(-30, 31, im.shape), 0, 255).astype(np.uint8) for im in imgs]
    pipe = inference.UInt8Pipeline(net, DEV)
    plain = list(pipe.run(imgs))
    scored = list(pipe.run(imgs, tgts))
    assert len(scored) == 3
    for im, tg, o, (so, p, s) in zip(imgs, tgts, plain, scored):
        assert np.array_equal(so, o)
        to, tt = torch.from_numpy(so).to(DEV), torch.from_numpy(tg).to(DEV)
        assert p == metrics.calculate_psnr(to, tt) and s == metrics.calculate_ssim(to, tt)
        pr, sr = metrics.psnr_ssim_y_cpu(so, tg, 1)
        assert abs(p - pr) <= PSNR_TOL and abs(s - sr) <= SSIM_TOL
    ev = inference.evaluate(net, DEV, imgs, tgts, crop_border=1)
    assert ev["psnr"] == [p for _, p, _ in scored] and ev["ssim"] == [s for _, _, s in scored]
    assert ev["avg_psnr"] == sum(ev["psnr"]) / 3 and ev["avg_ssim"] == sum(ev["ssim"]) / 3
    with pytest.raises(ValueError):
        list(pipe.run(imgs[:1], [tgts[1]]))
