"""CPU: the size rules by which UNet.conv_01 and the level-1 Haar analysis (wm_conv2d_dwt_fwd), and the level-1 Haar synthesis and
UNet.last (wm_idwt_conv2d_fwd), run as one kernel each - the shipped switches and floors, not forced ones -, the arch file's predicates
on top of them, and the entries' refusals that need no device."""
import torch
import torch.nn as nn

from oracle import backend as oracle_backend
import wave_mamba_amd as wm
from wave_mamba_amd import _lib
from wave_mamba_amd.archs import wavemamba_arch as arch


def test_shipped_rule_takes_uhd_and_refuses_the_dispatch_recorders_image():
    ops = wm.ops
    assert ops._FUSE_CONV_DWT is True
    assert ops._fuse_conv_dwt_map(1, 2176, 3840)                 # the UHD image: measured faster (profiles/fullres_ends/per_call.txt)
    assert ops._fuse_conv_dwt_map(1, 1088, 1920)                 # the smaller measured map: faster too
    assert not ops._fuse_conv_dwt_map(1, 1087, 1920)             # below it: not measured
    assert ops._FUSE_CONV_DWT_MIN_POSITIONS > 64 * 128           # tests/golden/arch_dispatch.json was recorded on the pair
    assert not ops._fuse_conv_dwt_map(1, 64, 128)
    assert not ops._fuse_conv_dwt_map(2, 2176, 3840)             # batch 2: not measured
    assert not ops._fuse_conv_dwt_map(0, 2176, 3840)


def test_shipped_tail_rule_takes_uhd_and_refuses_the_dispatch_recorders_image():
    ops = wm.ops
    assert ops._FUSE_IWT_CONV is True
    assert ops._fuse_iwt_conv_map(1, 2176, 3840)                 # measured faster at both maps (profiles/fullres_ends/per_call.txt)
    assert ops._fuse_iwt_conv_map(1, 1088, 1920)
    assert not ops._fuse_iwt_conv_map(1, 1087, 1920)             # below them: not measured
    assert ops._FUSE_IWT_CONV_MIN_POSITIONS > 64 * 128
    assert not ops._fuse_iwt_conv_map(1, 64, 128)
    assert not ops._fuse_iwt_conv_map(2, 2176, 3840)
    assert not ops._fuse_iwt_conv_map(0, 2176, 3840)


class _Covers:
    """A backend that has the fused operator and covers every operand: what is left is the size rule and the grad rule."""
    conv2d_dwt = staticmethod(lambda *a: None)
    conv2d_dwt_supported = staticmethod(lambda x, w: True)
    iwt_conv2d = staticmethod(lambda *a: None)
    iwt_conv2d_supported = staticmethod(lambda low, w: True)


def test_arch_predicate_refuses_small_images_and_gradients():
    conv = nn.Conv2d(3, 32, 3, 1, 1)
    uhd, small = torch.empty(1, 3, 2176, 3840, device="meta"), torch.empty(1, 3, 64, 128, device="meta")
    with oracle_backend.ops_backend(_Covers()):
        with torch.no_grad():
            assert arch._conv_dwt_fused(conv, uhd)
            assert not arch._conv_dwt_fused(conv, small)
        assert not arch._conv_dwt_fused(conv, uhd)               # grad mode on, trainable weights: the pair (autograd)
        for q in conv.parameters():
            q.requires_grad_(False)
        assert arch._conv_dwt_fused(conv, uhd)                   # frozen weights, an input without grad: nothing to differentiate
        assert not arch._conv_dwt_fused(conv, torch.empty(1, 3, 2176, 3840, device="meta", requires_grad=True))
    with oracle_backend.ops_backend(type("Plain", (), {})()), torch.no_grad():
        assert not arch._conv_dwt_fused(conv, uhd)               # a backend without the operator


def test_tail_arch_predicate_refuses_small_images_and_gradients():
    net = nn.Sequential(nn.Conv2d(32, 32, 1), nn.Conv2d(32, 3, 3, 1, 1))    # `last` and another layer of the network it closes
    last = net[1]
    meta = lambda *s, **k: torch.empty(*s, device="meta", **k)
    with oracle_backend.ops_backend(_Covers()):
        with torch.no_grad():
            assert arch._iwt_conv_fused(net, last, meta(1, 32, 1088, 1920), meta(1, 3, 2176, 3840))
            assert not arch._iwt_conv_fused(net, last, meta(1, 32, 32, 64), meta(1, 3, 64, 128))
        assert not arch._iwt_conv_fused(net, last, meta(1, 32, 1088, 1920), meta(1, 3, 2176, 3840))     # trainable weights
        for q in last.parameters():
            q.requires_grad_(False)
        assert not arch._iwt_conv_fused(net, last, meta(1, 32, 1088, 1920), meta(1, 3, 2176, 3840))     # ... anywhere in the network
        for q in net.parameters():
            q.requires_grad_(False)
        assert arch._iwt_conv_fused(net, last, meta(1, 32, 1088, 1920), meta(1, 3, 2176, 3840))
        assert not arch._iwt_conv_fused(net, last, meta(1, 32, 1088, 1920, requires_grad=True), meta(1, 3, 2176, 3840))
    with oracle_backend.ops_backend(type("Plain", (), {})()), torch.no_grad():
        assert not arch._iwt_conv_fused(net, last, meta(1, 32, 1088, 1920), meta(1, 3, 2176, 3840))


def test_entry_refusals_before_any_pointer_is_read():
    lib = _lib.load()
    args = lambda B, Cin, Cout, H, W, dtype=_lib.WM_F32: (None,) * 7 + (B, Cin, Cout, H, W, dtype, None)
    assert lib.wm_conv2d_dwt_fwd(*args(0, 3, 32, 8, 64)) == _lib.WM_OK
    assert lib.wm_conv2d_dwt_fwd(*args(1, 3, 32, 8, 64)) == _lib.WM_ENULL
    assert lib.wm_conv2d_dwt_fwd(*args(1, 3, 32, 7, 64)) == _lib.WM_EINVAL
    assert lib.wm_conv2d_dwt_fwd(*args(1, 3, 32, 8, 63)) == _lib.WM_EINVAL
    assert lib.wm_conv2d_dwt_fwd(*args(1, 3, 48, 8, 64)) == _lib.WM_EUNSUPPORTED
    assert lib.wm_conv2d_dwt_fwd(*args(1, 3, 32, 8, 64, _lib.WM_BF16)) == _lib.WM_EUNSUPPORTED
    args = lambda B, Cin, Cout, H, W, dtype=_lib.WM_F32: (None,) * 6 + (B, Cin, Cout, H, W, dtype, None)
    assert lib.wm_idwt_conv2d_fwd(*args(0, 32, 3, 8, 64)) == _lib.WM_OK
    assert lib.wm_idwt_conv2d_fwd(*args(1, 32, 3, 8, 64)) == _lib.WM_ENULL
    assert lib.wm_idwt_conv2d_fwd(*args(1, 32, 3, 7, 64)) == _lib.WM_EINVAL
    assert lib.wm_idwt_conv2d_fwd(*args(1, 32, 3, 8, 63)) == _lib.WM_EINVAL
    assert lib.wm_idwt_conv2d_fwd(*args(1, 48, 3, 8, 64)) == _lib.WM_EUNSUPPORTED
    assert lib.wm_idwt_conv2d_fwd(*args(1, 32, 3, 8, 64, _lib.WM_BF16)) == _lib.WM_EUNSUPPORTED
