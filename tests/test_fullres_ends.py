"""GPU: the two full-resolution 32-channel planes at the ends of the forward, folded into the convolutions beside them, against the
two launches each replaces - equal bit for bit at the kernel and at the model; status codes.
  head  wm_conv2d_dwt_fwd: (ll, hl, lh, hh) = dwt(conv3x3(img) + bias), UNet.conv_01 with the level-1 Haar analysis formed in its
        epilogue (wm_conv2d_fwd + wm_dwt2d_fwd)
  tail  wm_idwt_conv2d_fwd: y = conv3x3(iwt(low, high)) + bias + img, UNet.last forming its input tile from the bands of the level-1
        Haar synthesis (wm_idwt2d_fwd + wm_conv2d_fwd)"""
import functools

import pytest
import torch

import wave_mamba_amd as wm
from wave_mamba_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 32
ops = wm.ops

# one quad, every neighbour is padding | exactly one 64 x 8 tile: the store path without predicates | 2 x 2 exact tiles | batch 2, a
# 2-row ragged row tile and a 6-column ragged column tile | both ragged, more than one persistent step per workgroup
SHAPES = [(1, 2, 2), (1, 8, 64), (1, 16, 128), (2, 18, 70), (1, 34, 130)]
# 17 x 18 = 306 tiles on at most 256 workgroups: some walk two tiles, the chunk stream running across the tile boundary (the last column
# of tiles ragged)
SHAPES_PERSISTENT = [(1, 144, 1026)]
# the convolution kernel families the fused form exists in (the first-generation kernel has none: test_status_codes)
FAMILIES = [ops.CONV3X3_WAVE_SPECIALISED]


@functools.lru_cache(maxsize=None)
def params():
    g = torch.Generator(device=DEV); g.manual_seed(11)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    return dict(w=rn(C, 3, 3, 3) / 27 ** 0.5, b=rn(C) * 0.2, wl=rn(3, C, 3, 3) / (9 * C) ** 0.5, bl=rn(3) * 0.2)


@functools.lru_cache(maxsize=None)
def case(B, H, W):
    """The image and the pair's four bands (computed once, with the wave-specialised kernel pinned as for the fused call)."""
    g = torch.Generator(device=DEV); g.manual_seed(B * 1009 + H * 31 + W)
    img = torch.rand(B, 3, H, W, device=DEV, generator=g)
    p = params()
    ops.conv2d_select(ops.CONV3X3_WAVE_SPECIALISED)
    try:
        want = ops.dwt_init(ops.conv2d(img, p["w"], p["b"]))
    finally:
        ops.conv2d_select(ops.CONV3X3_AUTO)
    return img, want


@functools.lru_cache(maxsize=None)
def tail_case(B, H, W):
    """(low, high, image) and the pair's output; one band row and one band column of `high` scaled x 30: a quad that took a band value
    from the wrong row or column, or put a pixel at the wrong place of its 2x2, shows."""
    g = torch.Generator(device=DEV); g.manual_seed(B * 2003 + H * 37 + W)
    h, w = H // 2, W // 2
    low, high = torch.randn(B, C, h, w, device=DEV, generator=g), torch.randn(B, 3 * C, h, w, device=DEV, generator=g)
    high[:, :, h // 2] *= 30.0
    high[:, :, :, w // 2] *= 30.0
    img = torch.rand(B, 3, H, W, device=DEV, generator=g)
    p = params()
    ops.conv2d_select(ops.CONV3X3_WAVE_SPECIALISED)
    try:
        want = ops.conv2d(ops.iwt_init_pair(low, high), p["wl"], p["bl"], residual=img)
    finally:
        ops.conv2d_select(ops.CONV3X3_AUTO)
    return low, high, img, want


@pytest.fixture(params=FAMILIES, ids=["wave_specialised"])
def family(request):
    ops.conv2d_select(request.param)
    yield request.param
    ops.conv2d_select(ops.CONV3X3_AUTO)


@pytest.mark.parametrize("shape", SHAPES + SHAPES_PERSISTENT, ids=str)
def test_conv2d_dwt_bit_identical_to_the_pair(shape, family):
    img, want = case(*shape)
    p = params()
    got = ops.conv2d_dwt(img, p["w"], p["b"])
    B, H, W = shape
    for name, g, w in zip(("ll", "hl", "lh", "hh"), got, want):
        assert torch.isfinite(w).all()
        assert g.shape == w.shape == (B, C, H // 2, W // 2)
        assert torch.equal(g, w), f"{name}: max abs difference {float((g - w).abs().max()):.3e}"
    for g, w in zip(ops.conv2d_dwt(img, p["w"], None), ops.dwt_init(ops.conv2d(img, p["w"], None))):
        assert torch.equal(g, w), "without bias"


@pytest.mark.parametrize("shape", SHAPES + SHAPES_PERSISTENT, ids=str)
def test_iwt_conv2d_bit_identical_to_the_pair(shape, family):
    low, high, img, want = tail_case(*shape)
    p = params()
    got = ops.iwt_conv2d(low, high, p["wl"], p["bl"], residual=img)
    assert torch.isfinite(want).all()
    assert got.shape == want.shape == (shape[0], 3, shape[1], shape[2])
    assert torch.equal(got, want), f"max abs difference {float((got - want).abs().max()):.3e}"
    assert torch.equal(ops.iwt_conv2d(low, high, p["wl"], None), ops.conv2d(ops.iwt_init_pair(low, high), p["wl"], None)), \
        "without bias and residual"


def test_pair_kernels_agree():
    """The reference of the test above does not depend on which kernel computed the convolution."""
    img, want = case(2, 18, 70)
    p = params()
    ops.conv2d_select(ops.CONV3X3_FIRST_GEN)
    try:
        first = ops.dwt_init(ops.conv2d(img, p["w"], p["b"]))
    finally:
        ops.conv2d_select(ops.CONV3X3_AUTO)
    assert all(torch.equal(a, b) for a, b in zip(first, want))
    low, high, img, want = tail_case(2, 18, 70)
    ops.conv2d_select(ops.CONV3X3_FIRST_GEN)
    try:
        first = ops.conv2d(ops.iwt_init_pair(low, high), p["wl"], p["bl"], residual=img)
    finally:
        ops.conv2d_select(ops.CONV3X3_AUTO)
    assert torch.equal(first, want)


def test_status_codes():
    from wave_mamba_amd.ops import _ptr, _stream
    lib, p = _lib.load(), params()
    img, want = case(1, 8, 64)
    bands = [torch.empty_like(t) for t in want]
    frag = ops._conv2d_wfrag(p["w"], cache=False)
    torch.cuda.synchronize()

    def call(B=1, Cin=3, Cout=32, H=8, W=64, dtype=_lib.WM_F32, xp=_ptr(img), fp=frag.data_ptr(), hh=_ptr(bands[3])):
        return lib.wm_conv2d_dwt_fwd(xp, fp, _ptr(p["b"]), *[_ptr(t) for t in bands[:3]], hh, B, Cin, Cout, H, W, dtype, _stream())
    assert call() == _lib.WM_OK
    assert call(H=7) == _lib.WM_EINVAL and call(W=63) == _lib.WM_EINVAL and call(B=-1) == _lib.WM_EINVAL
    assert call(Cout=48) == _lib.WM_EUNSUPPORTED and call(Cout=64) == _lib.WM_EUNSUPPORTED
    assert call(dtype=_lib.WM_BF16) == _lib.WM_EUNSUPPORTED
    assert call(xp=None) == _lib.WM_ENULL and call(fp=None) == _lib.WM_ENULL and call(hh=None) == _lib.WM_ENULL
    assert call(fp=frag.data_ptr() + 4) == _lib.WM_EALIGN
    assert call(B=0) == _lib.WM_OK and call(H=0) == _lib.WM_OK
    assert call(H=8192, W=4096) == _lib.WM_EUNSUPPORTED           # a 4-GiB plane: beyond the kernel's 32-bit offsets, not launched
    ops.conv2d_select(ops.CONV3X3_FIRST_GEN)                      # the first-generation kernel has no analysis form
    try:
        assert call() == _lib.WM_EUNSUPPORTED
        got, names = launches(lambda: ops.conv2d_dwt(img, p["w"], p["b"]))          # ... and the operator runs the pair
        assert names == ["wm_conv2d_dwt_fwd", "wm_conv2d_fwd", "wm_dwt2d_fwd"]
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    finally:
        ops.conv2d_select(ops.CONV3X3_AUTO)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(bands, want))


def test_tail_status_codes():
    from wave_mamba_amd.ops import _ptr, _stream
    lib, p = _lib.load(), params()
    low, high, img, want = tail_case(1, 8, 64)
    y = torch.empty_like(want)
    frag = ops._conv2d_wfrag(p["wl"], cache=False)
    torch.cuda.synchronize()

    def call(B=1, Cin=32, Cout=3, H=8, W=64, dtype=_lib.WM_F32, lp=_ptr(low), hp=_ptr(high), fp=frag.data_ptr(), yp=_ptr(y)):
        return lib.wm_idwt_conv2d_fwd(lp, hp, fp, _ptr(p["bl"]), _ptr(img), yp, B, Cin, Cout, H, W, dtype, _stream())
    assert call() == _lib.WM_OK
    assert call(H=7) == _lib.WM_EINVAL and call(W=63) == _lib.WM_EINVAL and call(B=-1) == _lib.WM_EINVAL
    assert call(Cin=48) == _lib.WM_EUNSUPPORTED and call(Cin=16) == _lib.WM_EUNSUPPORTED
    assert call(dtype=_lib.WM_BF16) == _lib.WM_EUNSUPPORTED
    assert call(lp=None) == _lib.WM_ENULL and call(hp=None) == _lib.WM_ENULL and call(fp=None) == _lib.WM_ENULL
    assert call(yp=None) == _lib.WM_ENULL
    assert call(fp=frag.data_ptr() + 4) == _lib.WM_EALIGN
    assert call(B=0) == _lib.WM_OK and call(H=0) == _lib.WM_OK
    assert call(H=8192, W=4096) == _lib.WM_EUNSUPPORTED           # a 4-GiB plane: beyond the kernel's 32-bit offsets, not launched
    ops.conv2d_select(ops.CONV3X3_FIRST_GEN)                      # the first-generation kernel has no synthesis form
    try:
        assert call() == _lib.WM_EUNSUPPORTED
        got, names = launches(lambda: ops.iwt_conv2d(low, high, p["wl"], p["bl"], residual=img))
        assert names == ["wm_idwt_conv2d_fwd", "wm_idwt2d_fwd", "wm_conv2d_fwd"]
        assert torch.equal(got, want)
    finally:
        ops.conv2d_select(ops.CONV3X3_AUTO)
    torch.cuda.synchronize()
    assert torch.equal(y, want)


def launches(fn):
    """fn()'s result and the library entry points it launched."""
    names = []
    real = ops._launch

    def spy(dev, name, *a, **k):
        if not name.endswith("_prep"):                                    # (weight / parameter preparation: cached by whichever path ran first)
            names.append(name)
        return real(dev, name, *a, **k)
    ops._launch = spy
    try:
        with torch.no_grad():
            out = fn()
    finally:
        ops._launch = real
    return out, names


@pytest.mark.parametrize("two_streams", [True, False])
def test_model_bit_identical(monkeypatch, two_streams):
    """The dispatch recorder's wf = 32 model at (1, 3, 64, 128): both ends on the fused paths (floors lowered) against the shipped
    rules, which keep an image this small on the pairs."""
    torch.manual_seed(0)                                                  # (make_golden_dispatch.run_mode's model and input)
    net = wm.WaveMamba(in_chn=3, wf=32, n_l_blocks=[1, 1, 1], n_h_blocks=[1, 1, 1], ffn_scale=2).to(DEV).eval()
    net.restoration_network.two_streams = two_streams
    x = torch.rand(1, 3, 64, 128, device=DEV)
    want, names_pair = launches(lambda: net(x))
    torch.cuda.synchronize()
    assert "wm_conv2d_dwt_fwd" not in names_pair and "wm_idwt_conv2d_fwd" not in names_pair
    monkeypatch.setattr(ops, "_FUSE_CONV_DWT_MIN_POSITIONS", 0)
    monkeypatch.setattr(ops, "_FUSE_IWT_CONV_MIN_POSITIONS", 0)
    got, names = launches(lambda: net(x))
    torch.cuda.synchronize()
    assert names.count("wm_conv2d_dwt_fwd") == 1 and names.count("wm_idwt_conv2d_fwd") == 1
    assert len(names) == len(names_pair) - 2                              # each end: two launches -> one
    assert names.count("wm_dwt2d_fwd") == names_pair.count("wm_dwt2d_fwd") - 1
    assert names.count("wm_idwt2d_fwd") == names_pair.count("wm_idwt2d_fwd") - 1
    assert torch.equal(got, want), f"max abs difference {float((got - want).abs().max()):.3e}"
