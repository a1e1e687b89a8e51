"""CPU: the size rule by which the HFE branch sends a depth-wise 3x3 and the 1x1 convolution that reads it to the one-kernel form
(wm_dwconv_conv1x1_fwd) - the shipped switch and threshold, not forced ones - and the entry's refusals that need no device."""
import wave_mamba_amd as wm
from wave_mamba_amd import _lib


def test_shipped_rule_at_the_uhd_levels():
    ops = wm.ops
    assert ops._FUSE_DW_PW is True
    assert ops._FUSE_DW_PW_MIN_POSITIONS >= 272 * 480        # never below UHD level 3: nothing smaller is measured
    assert ops._fuse_dw_pw_map(1, 1088, 1920)                # UHD level 1: measured faster
    assert ops._fuse_dw_pw_map(1, 544, 960)                  # level 2: measured faster
    assert ops._fuse_dw_pw_map(1, 272, 480)                  # level 3: measured faster
    assert not ops._fuse_dw_pw_map(1, 271, 480)              # below level 3: not measured
    assert not ops._fuse_dw_pw_map(0, 1088, 1920)


def test_the_dispatch_recorders_maps_keep_the_pair():
    """tests/test_arch_dispatch.py pins the operator calls of a wf = 32 model on a 64 x 128 image: its HFE maps stay where they were."""
    for (H, W) in [(32, 64), (16, 32), (8, 16)]:
        for B in (1, 2, 64):
            assert not wm.ops._fuse_dw_pw_map(B, H, W)


def test_false_beyond_the_entrys_offset_range():
    ops = wm.ops
    assert ops._fuse_dw_pw_map(1, 8191, 8192)
    assert not ops._fuse_dw_pw_map(1, 8192, 8192)            # H W = 2^26: the kernel's offsets are 32-bit
    assert not ops._fuse_dw_pw_map(1, 16384, 16384)
    lib = _lib.load()
    # the entry agrees, before it looks at a pointer; an empty problem is WM_OK, a wrong channel count or activation a refusal
    args = lambda B, C, Cout, H, W, act=0: (None, C * H * W, None, None, act, None, None, None, None, B, C, Cout, H, W, None)
    assert lib.wm_dwconv_conv1x1_fwd(*args(0, 32, 32, 8, 64)) == _lib.WM_OK
    assert lib.wm_dwconv_conv1x1_fwd(*args(1, 32, 32, 8, 64)) == _lib.WM_ENULL
    assert lib.wm_dwconv_conv1x1_fwd(*args(1, 16, 32, 8, 64)) == _lib.WM_EUNSUPPORTED
    assert lib.wm_dwconv_conv1x1_fwd(*args(1, 32, 32, 8, 64, act=7)) == _lib.WM_EINVAL
