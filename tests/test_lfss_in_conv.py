"""GPU: SS2D's prologue as one kernel (wm_lfss_in_conv_fwd: ln_1 -> in_proj[:D] -> depth-wise 3x3 -> SiLU, x never stored) against
the two kernels it replaces (wm_lfss_in_fwd with z = NULL, then wm_dwconv3x3_fwd with SiLU): equal bit for bit on fp32 planes, at
the kernel and at the block; against the fp64 composition; status codes; run-to-run equality."""
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close
import wave_mamba_amd as wm
from wave_mamba_amd import _lib
from wave_mamba_amd.archs import wavemamba_arch as arch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4                  # test_gpu_parity.py::test_lfss_glue_kernels_c32_vs_fp64's bar for its plane outputs
C, D = 32, 64
WM_OK, WM_EUNSUPPORTED = 0, -5


def band_rows(B, H, W):
    rb = _lib.load().wm_lfss_in_conv_band_rows(B, H, W)
    assert rb > 0
    return rb


@functools.lru_cache(maxsize=None)
def params():
    g = torch.Generator(device=DEV); g.manual_seed(7)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    return dict(ln_w=rn(C) * 0.2 + 1, ln_b=rn(C) * 0.2, Win=rn(2 * D, C) / 6, cw=rn(D, 1, 3, 3) / 3, cb=rn(D) * 0.2)


@functools.lru_cache(maxsize=None)
def case(B, H, W):
    """Logical (B, L, C) tokens with one image row scaled x 30 (a band or strip that took its halo from the wrong row shows)."""
    g = torch.Generator(device=DEV); g.manual_seed(B * 1009 + H * 31 + W)
    t = torch.randn(B, H, W, C, device=DEV, generator=g)
    t[:, H // 2] *= 30.0
    return t.reshape(B, H * W, C)


def laid_out(tokens, nchw):
    return tokens.transpose(1, 2).contiguous() if nchw else tokens


def fused(tokens, B, H, W, nchw, fill=float("nan")):
    from wave_mamba_amd.ops import _ptr, _stream, check
    p, tok = params(), laid_out(tokens, nchw)
    xc = torch.full((B, D, H, W), fill, device=DEV)
    check(_lib.load().wm_lfss_in_conv_fwd(_ptr(tok), int(nchw), _ptr(p["ln_w"]), _ptr(p["ln_b"]), 1e-5, _ptr(p["Win"]), _ptr(p["cw"]),
                                          _ptr(p["cb"]), _ptr(xc), B, H, W, C, 0, _stream()), "wm_lfss_in_conv_fwd")
    return xc


def pair(tokens, B, H, W, nchw):
    from wave_mamba_amd.ops import _ptr, _stream, check
    lib, p, tok = _lib.load(), params(), laid_out(tokens, nchw)
    x = torch.full((B, D, H, W), float("nan"), device=DEV)
    xc = torch.full((B, D, H, W), float("nan"), device=DEV)
    check(lib.wm_lfss_in_fwd(_ptr(tok), int(nchw), _ptr(p["ln_w"]), _ptr(p["ln_b"]), 1e-5, _ptr(p["Win"]), _ptr(x), None, B, H * W, C, 0,
                             _stream()), "wm_lfss_in_fwd")
    check(lib.wm_dwconv3x3_fwd(_ptr(x), _ptr(p["cw"]), _ptr(p["cb"]), _ptr(xc), B, D, H, W, 1, 0, _stream()), "wm_dwconv3x3_fwd")
    return xc


SHAPES = [(1, 1, 32), (1, 2, 64), (2, 3, 32), (1, 5, 64), (1, 9, 128), (1, 40, 96), (2, 33, 160)]
SEAMS = ["rb-1", "rb", "rb+1", "2rb+1"]                       # band seams at W = 64, rb from the library's plan


def seam_shape(which):
    rb = band_rows(1, 8, 64)
    H = {"rb-1": rb - 1, "rb": rb, "rb+1": rb + 1, "2rb+1": 2 * rb + 1}[which]
    assert band_rows(1, H, 64) == rb, "the plan's band height moved with H: pick the seam heights from the plan at each H"
    return (1, H, 64)


@pytest.mark.parametrize("nchw", [False, True])
@pytest.mark.parametrize("shape", SHAPES + SEAMS, ids=str)
def test_kernel_bit_identical_to_the_pair(shape, nchw):
    B, H, W = seam_shape(shape) if isinstance(shape, str) else shape
    tokens = case(B, H, W)
    got, want = fused(tokens, B, H, W, nchw), pair(tokens, B, H, W, nchw)
    assert not torch.isnan(want).any()
    assert not torch.isnan(got).any(), "an output element was never written"
    assert torch.equal(got, want), f"max abs difference {float((got - want).abs().max()):.3e}"


@pytest.mark.parametrize("shape,nchw", [((1, 1088, 1920), True), ((1, 544, 960), False)], ids=str)
def test_kernel_bit_identical_at_the_shipped_band_heights(shape, nchw):
    """The two UHD maps the operator layer sends to the kernel: their bands are taller than the small maps' above (the plan's
    choice, 34 and 10 rows when this was written) and a launch fills the chip."""
    B, H, W = shape
    assert band_rows(B, H, W) > band_rows(1, 8, 64)
    assert wm.ops._fuse_in_conv_map(B, H, W)
    tokens = case(B, H, W)
    got, want = fused(tokens, B, H, W, nchw), pair(tokens, B, H, W, nchw)
    assert not torch.isnan(got).any(), "an output element was never written"
    assert torch.equal(got, want)


@pytest.mark.parametrize("nchw", [False, True])
@pytest.mark.parametrize("shape", [(1, 9, 128), (2, 33, 160)], ids=str)
def test_kernel_vs_fp64(shape, nchw):
    """LayerNorm -> linear (rows [0, D)) -> depth-wise 3x3 with zero padding -> SiLU in float64."""
    B, H, W = shape
    tokens, p = case(B, H, W), params()
    d = lambda t: t.double()
    x = F.linear(F.layer_norm(d(tokens), (C,), d(p["ln_w"]), d(p["ln_b"]), 1e-5), d(p["Win"][:D])).transpose(1, 2).reshape(B, D, H, W)
    want = F.silu(F.conv2d(x, d(p["cw"]), d(p["cb"]), padding=1, groups=D))
    assert_close(fused(tokens, B, H, W, nchw), want.float(), TOL, "lfss_in_conv xc")


def block():
    torch.manual_seed(11)
    blk = arch.LFSSBlock(32, expand=2.0).eval().to(DEV)
    with torch.no_grad():
        for p in blk.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return blk


def block_forward(blk, x, H, W, nchw, fuse):
    """ops.lfss_block_forward with the one-kernel prologue on every map the entry supports (fuse) or on none; returns the output and
    the library entry points the call launched."""
    ops = wm.ops
    launched = []
    real = ops._launch

    def spy(dev, name, *a, **k):
        launched.append(name)
        return real(dev, name, *a, **k)

    saved = ops._FUSE_IN_CONV, ops._FUSE_IN_CONV_MIN_POSITIONS, ops._launch
    ops._FUSE_IN_CONV, ops._FUSE_IN_CONV_MIN_POSITIONS, ops._launch = fuse, 0, spy
    try:
        with torch.no_grad():
            out = ops.lfss_block_forward(x, (H, W), blk, tok_nchw=nchw, out_nchw=nchw)
    finally:
        ops._FUSE_IN_CONV, ops._FUSE_IN_CONV_MIN_POSITIONS, ops._launch = saved
    return out, launched


@pytest.mark.parametrize("B,H,W,nchw", [(1, 40, 96, True), (2, 33, 32, False), (2, 5, 64, False), (1, 272, 480, True)])
def test_block_bit_identical(B, H, W, nchw):
    blk = block()
    x = torch.randn(B, 32, H, W, device=DEV) if nchw else torch.randn(B, H * W, 32, device=DEV)
    got, names = block_forward(blk, x, H, W, nchw, True)
    want, names_pair = block_forward(blk, x, H, W, nchw, False)
    assert "wm_lfss_in_conv_fwd" in names and "wm_lfss_in_fwd" not in names
    assert "wm_lfss_in_fwd" in names_pair and "wm_lfss_in_conv_fwd" not in names_pair
    assert torch.equal(got, want), f"max abs difference {float((got - want).abs().max()):.3e}"


def test_status_codes_and_block_fallback():
    from wave_mamba_amd.ops import _ptr, _stream
    lib, p = _lib.load(), params()
    tok, xc = torch.randn(1, 8 * 64, C, device=DEV), torch.empty(1, D, 8, 64, device=DEV)
    call = lambda B, H, W, Cc, dtype=0: lib.wm_lfss_in_conv_fwd(_ptr(tok), 0, _ptr(p["ln_w"]), _ptr(p["ln_b"]), 1e-5, _ptr(p["Win"]),
                                                                 _ptr(p["cw"]), _ptr(p["cb"]), _ptr(xc), B, H, W, Cc, dtype, _stream())
    assert call(1, 8, 64, 16) == WM_EUNSUPPORTED             # C = 16
    assert call(1, 8, 40, 32) == WM_EUNSUPPORTED             # a width without a tile form (W % 32 != 0)
    assert call(1, 8, 64, 32, 1) == WM_EUNSUPPORTED          # bf16 planes
    assert call(0, 8, 64, 32) == WM_OK and call(1, 0, 64, 32) == WM_OK
    assert lib.wm_lfss_in_conv_band_rows(1, 8, 40) == WM_EUNSUPPORTED
    # the block on such a map takes the pair whatever the switch says
    blk = block()
    x = torch.randn(1, 12 * 40, 32, device=DEV)
    got, names = block_forward(blk, x, 12, 40, False, True)
    want, _ = block_forward(blk, x, 12, 40, False, False)
    assert "wm_lfss_in_fwd" in names and "wm_lfss_in_conv_fwd" not in names
    assert torch.equal(got, want)
    # and so does a C = 16 block
    torch.manual_seed(12)
    blk16 = arch.LFSSBlock(16, expand=2.0).eval().to(DEV)
    x = torch.randn(1, 8 * 32, 16, device=DEV)
    got, names = block_forward(blk16, x, 8, 32, False, True)
    want, _ = block_forward(blk16, x, 8, 32, False, False)
    assert "wm_lfss_in_fwd" in names and "wm_lfss_in_conv_fwd" not in names
    assert torch.equal(got, want)


def test_two_calls_bit_equal():
    B, H, W = 2, 33, 160
    tokens = case(B, H, W)
    for nchw in (False, True):
        assert torch.equal(fused(tokens, B, H, W, nchw), fused(tokens, B, H, W, nchw, fill=0.0))
