"""GPU: a depth-wise 3x3 folded into the 1x1 convolution that reads it (wm_dwconv_conv1x1_fwd: y = conv1x1(act(dwconv3x3(x))) + bias
(+ residual), the plane between the two never stored) against the two launches it replaces (wm_dwconv3x3_fwd, wm_conv2d_fwd):
equal bit for bit at the kernel, at the HFE block and at the model; against the fp64 composition; status codes; run-to-run
equality."""
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close
import wave_mamba_amd as wm
from wave_mamba_amd import _lib
from wave_mamba_amd.archs import wavemamba_arch as arch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 32
ops = wm.ops


@functools.lru_cache(maxsize=None)
def params():
    g = torch.Generator(device=DEV); g.manual_seed(5)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    return dict(wd=rn(C, 1, 3, 3) / 3, bd=rn(C) * 0.2, w=rn(C, C, 1, 1) / C ** 0.5, b=rn(C) * 0.2)


@functools.lru_cache(maxsize=None)
def case(B, H, W):
    """(x, residual); one image row and one image column of x scaled x 30: a strip or band that took a neighbour from the wrong
    row or column shows."""
    g = torch.Generator(device=DEV); g.manual_seed(B * 1009 + H * 31 + W)
    x = torch.randn(B, C, H, W, device=DEV, generator=g)
    x[:, :, H // 2] *= 30.0
    x[:, :, :, W // 2] *= 30.0
    return x, torch.randn(B, C, H, W, device=DEV, generator=g)


def fused(x, act, dw_bias, pw_bias, residual):
    p = params()
    return ops.dwconv_conv1x1(x, p["wd"], p["bd"] if dw_bias else None, act, p["w"], p["b"] if pw_bias else None,
                              residual=residual)


def pair(x, act, dw_bias, pw_bias, residual):
    p = params()
    return ops.conv2d(ops.dwconv3x3(x, p["wd"], p["bd"] if dw_bias else None, act), p["w"], p["b"] if pw_bias else None,
                      residual=residual)


def check_equal(x, act, dw_bias, pw_bias, residual):
    got, want = fused(x, act, dw_bias, pw_bias, residual), pair(x, act, dw_bias, pw_bias, residual)
    assert torch.isfinite(want).all()
    assert got.shape == want.shape
    assert torch.equal(got, want), f"max abs difference {float((got - want).abs().max()):.3e}"
    assert torch.equal(got, fused(x, act, dw_bias, pw_bias, residual)), "two runs of the fused kernel differ"


# (1,1,1) | an image smaller than any strip | one column past a 32-column strip | exact strips, rows not a multiple of the band |
# ragged right and bottom, batch 2 | | several strips and bands on several workgroups
SHAPES = [(1, 1, 1), (1, 3, 5), (1, 2, 33), (1, 17, 64), (2, 40, 70), (1, 70, 150), (1, 136, 256)]


@pytest.mark.parametrize("act", ["gelu", "none"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_shipped_forms_bit_identical_to_the_pair(shape, act):
    """The ffn tail (GELU) and the value path (no activation), each with both biases and the residual."""
    x, r = case(*shape)
    check_equal(x, act, True, True, r)


@pytest.mark.parametrize("act,dw_bias,pw_bias,res", list(itertools.product(["gelu", "none"], [False, True], [False, True], [False, True])))
@pytest.mark.parametrize("shape", [(2, 40, 70), (1, 17, 64)], ids=str)
def test_every_operand_form_bit_identical_to_the_pair(shape, act, dw_bias, pw_bias, res):
    x, r = case(*shape)
    check_equal(x, act, dw_bias, pw_bias, r if res else None)


@pytest.mark.parametrize("shape", [(1, 1088, 1920), (1, 544, 960)], ids=str)
def test_taller_bands_of_the_chip_filling_maps(shape):
    """UHD levels 1 and 2: the maps on which the launch walks 16- and 8-row bands (smaller maps: 4) - and the sizes the step runs
    the kernel at."""
    g = torch.Generator(device=DEV); g.manual_seed(3)
    x = torch.randn(1, C, *shape[1:], device=DEV, generator=g)
    r = torch.randn(1, C, *shape[1:], device=DEV, generator=g)
    for act in ("gelu", "none"):
        got, want = fused(x, act, True, True, r), pair(x, act, True, True, r)
        assert torch.equal(got, want), f"{act}: max abs difference {float((got - want).abs().max()):.3e}"


@pytest.mark.parametrize("act", ["gelu", "none"])
def test_input_as_a_channel_slice(act):
    """x = channels 64..95 of a (2, 96, 9, 35) tensor: batch stride 96 H W, a plane base that is only 4-byte aligned."""
    g = torch.Generator(device=DEV); g.manual_seed(9)
    big = torch.randn(2, 96, 9, 35, device=DEV, generator=g)
    r = torch.randn(2, C, 9, 35, device=DEV, generator=g)
    x = big[:, 64:96]
    assert not x.is_contiguous() and (x.stride(1) * 4) % 16 != 0 and x.stride(0) == 96 * 9 * 35
    launched = []
    real = ops._launch

    def spy(dev, name, *a, **k):
        launched.append((name, a[0].data_ptr() if isinstance(a[0], torch.Tensor) else a[0]))
        return real(dev, name, *a, **k)
    ops._launch = spy
    try:
        got = fused(x, act, True, True, r)
    finally:
        ops._launch = real
    assert ("wm_dwconv_conv1x1_fwd", x.data_ptr()) in launched, "the slice was copied instead of read in place"
    want = pair(x.contiguous(), act, True, True, r)
    assert torch.equal(got, want), f"max abs difference {float((got - want).abs().max()):.3e}"


@pytest.mark.parametrize("act", ["gelu", "none"])
def test_large_values_on_the_border(act):
    """Magnitude 1e3 in the first and last rows and columns: a padding slip (a clamped row or column read as data) is far outside
    any tolerance."""
    x, r = case(2, 40, 70)
    x = x.clone()
    for sl in ((..., 0, slice(None)), (..., -1, slice(None)), (..., slice(None), 0), (..., slice(None), -1)):
        x[sl] = torch.where(x[sl] < 0, -1e3, 1e3)
    check_equal(x, act, True, True, r)


def test_vs_fp64():
    """The float64 composition, at the bar of test_conv2d_gated_vs_torch (which the pair meets)."""
    x, r = case(1, 70, 150)
    p = params()
    d = lambda t: t.double()
    want = F.conv2d(F.gelu(F.conv2d(d(x), d(p["wd"]), d(p["bd"]), padding=1, groups=C)), d(p["w"]), d(p["b"])) + d(r)
    assert_close(fused(x, "gelu", True, True, r), want.float(), 2e-5, "dwconv_conv1x1 (1, 70, 150)")
    assert_close(pair(x, "gelu", True, True, r), want.float(), 2e-5, "dwconv3x3 + conv2d (1, 70, 150)")


def test_status_codes():
    from wave_mamba_amd.ops import _ptr, _stream
    lib, p = _lib.load(), params()
    x, r = case(1, 17, 64)
    y = torch.empty_like(x)
    frag = ops._conv2d_wfrag(p["w"], cache=False)
    torch.cuda.synchronize()

    def call(B=1, Cin=32, Cout=32, H=17, W=64, act=2, xp=_ptr(x), fp=frag.data_ptr(), yp=_ptr(y)):
        return lib.wm_dwconv_conv1x1_fwd(xp, Cin * H * W, _ptr(p["wd"]), _ptr(p["bd"]), act, fp, _ptr(p["b"]), _ptr(r), yp,
                                         B, Cin, Cout, H, W, _stream())
    assert call() == _lib.WM_OK
    assert call(Cin=16) == _lib.WM_EUNSUPPORTED and call(Cout=64) == _lib.WM_EUNSUPPORTED
    assert call(xp=None) == _lib.WM_ENULL and call(fp=None) == _lib.WM_ENULL and call(yp=None) == _lib.WM_ENULL
    assert call(act=7) == _lib.WM_EINVAL and call(act=1) == _lib.WM_EINVAL and call(B=-1) == _lib.WM_EINVAL
    assert call(fp=frag.data_ptr() + 4) == _lib.WM_EALIGN
    assert call(B=0) == _lib.WM_OK and call(H=0) == _lib.WM_OK
    assert call(H=8192, W=8192) == _lib.WM_EUNSUPPORTED          # offsets beyond the kernel's 32-bit range: refused, not launched
    torch.cuda.synchronize()
    assert torch.equal(y, pair(x, "gelu", True, True, r))


def hfe_block():
    torch.manual_seed(21)
    blk = arch.HFEBlock(32, match_factor=1, ffn_expansion_factor=1).eval().to(DEV)
    with torch.no_grad():
        for q in blk.parameters():
            q.add_(0.05 * torch.randn_like(q))
    return blk


def launches(fn):
    """fn()'s result and the library entry points it launched."""
    names = []
    real = ops._launch

    def spy(dev, name, *a, **k):
        if name != "wm_conv2d_prep":                                      # (weight preparation: cached by whichever path ran first)
            names.append(name)
        return real(dev, name, *a, **k)
    ops._launch = spy
    try:
        with torch.no_grad():
            out = fn()
    finally:
        ops._launch = real
    return out, names


@pytest.mark.parametrize("B,H,W", [(1, 40, 72), (2, 24, 40)])
def test_hfe_block_bit_identical(monkeypatch, B, H, W):
    """Every map sent to the fused call (threshold 0) against the switch off.  Batch 1 fuses both sites; batch 2 the ffn tail only
    (the value path keeps the 96-channel depth-wise conv: its q | k slice is not contiguous)."""
    blk = hfe_block()
    g = torch.Generator(device=DEV); g.manual_seed(B + H)
    x = torch.randn(B, 32, H, W, device=DEV, generator=g)
    per = torch.randn(B, 32, H, W, device=DEV, generator=g)
    monkeypatch.setattr(ops, "_FUSE_DW_PW_MIN_POSITIONS", 0)
    got, names = launches(lambda: blk(x, per))
    got_early, _ = launches(lambda: blk(x, per, qkv=blk.qkv_of(x)))      # the qkv head issued ahead of time, as the U-Net does
    monkeypatch.setattr(ops, "_FUSE_DW_PW", False)
    want, names_pair = launches(lambda: blk(x, per))
    assert names.count("wm_dwconv_conv1x1_fwd") == (2 if B == 1 else 1)
    assert "wm_dwconv_conv1x1_fwd" not in names_pair
    assert len(names) == len(names_pair) - 1                              # the ffn tail's launch; the value path trades one for one
    assert torch.equal(got, want), f"max abs difference {float((got - want).abs().max()):.3e}"
    assert torch.equal(got_early, want)


@pytest.mark.parametrize("two_streams", [True, False])
def test_model_bit_identical(monkeypatch, two_streams):
    """The dispatch recorder's wf = 32 model at (1, 3, 64, 128): every HFE map on the fused path against the shipped rule, which
    keeps maps this small on the pair."""
    torch.manual_seed(0)                                                  # (make_golden_dispatch.run_mode's model and input)
    net = wm.WaveMamba(in_chn=3, wf=32, n_l_blocks=[1, 1, 1], n_h_blocks=[1, 1, 1], ffn_scale=2).to(DEV).eval()
    net.restoration_network.two_streams = two_streams
    x = torch.rand(1, 3, 64, 128, device=DEV)
    want, names_pair = launches(lambda: net(x))
    torch.cuda.synchronize()
    assert "wm_dwconv_conv1x1_fwd" not in names_pair
    monkeypatch.setattr(ops, "_FUSE_DW_PW_MIN_POSITIONS", 0)
    got, names = launches(lambda: net(x))
    torch.cuda.synchronize()
    assert names.count("wm_dwconv_conv1x1_fwd") == 12                    # 6 HFE blocks, two sites each
    assert torch.equal(got, want), f"max abs difference {float((got - want).abs().max()):.3e}"
