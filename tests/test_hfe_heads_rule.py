"""CPU: the size rule by which an HFE block sends its two heads (LayerNorm2d -> 1x1 -> depth-wise 3x3) to the one-kernel form
(wm_ln_conv1x1_dwconv_fwd) - the shipped switch and floors, not forced ones - and the entry's refusals that need no device."""
import wave_mamba_amd as wm
from wave_mamba_amd import _lib

LEVELS = [(1088, 1920), (544, 960), (272, 480)]              # UHD levels 1, 2, 3


def test_shipped_rule_at_the_uhd_levels():
    ops = wm.ops
    assert ops._FUSE_PW_DW is True
    assert set(ops._FUSE_PW_DW_MIN_POSITIONS) == {"qkv", "project_in"}
    for head, floor in ops._FUSE_PW_DW_MIN_POSITIONS.items():
        assert floor in [h * w for h, w in LEVELS]           # a measured level; never below level 3: nothing smaller is measured
        for (h, w) in LEVELS:                                 # true at and above the head's floor, false below it
            assert ops._fuse_pw_dw_map(1, h, w, head) == (h * w >= floor)
        assert not ops._fuse_pw_dw_map(1, floor - 1, 1, head)
        fh, fw = next((h, w) for h, w in LEVELS if h * w == floor)
        assert not ops._fuse_pw_dw_map(1, fh - 1, fw, head) and not ops._fuse_pw_dw_map(0, 1088, 1920, head)


def test_the_dispatch_recorders_maps_keep_the_pair():
    """tests/test_arch_dispatch.py pins the operator calls of a wf = 32 model on a 64 x 128 image: its HFE maps stay where they were."""
    for head in wm.ops._FUSE_PW_DW_MIN_POSITIONS:
        for (H, W) in [(32, 64), (16, 32), (8, 16)]:
            for B in (1, 2, 64):
                assert not wm.ops._fuse_pw_dw_map(B, H, W, head)


def test_false_with_the_switch_off(monkeypatch):
    monkeypatch.setattr(wm.ops, "_FUSE_PW_DW", False)
    for head in wm.ops._FUSE_PW_DW_MIN_POSITIONS:
        assert not any(wm.ops._fuse_pw_dw_map(1, h, w, head) for h, w in LEVELS)


def test_false_beyond_the_entrys_offset_range():
    ops = wm.ops
    for head in ops._FUSE_PW_DW_MIN_POSITIONS:
        assert ops._fuse_pw_dw_map(1, 4095, 8192, head)
        assert not ops._fuse_pw_dw_map(1, 4096, 8192, head)      # H W = 2^25: a 32-plane output tile no longer fits one raw buffer
        assert not ops._fuse_pw_dw_map(1, 8192, 8192, head)      # H W = 2^26
        assert not ops._fuse_pw_dw_map(1, 16384, 16384, head)
    lib = _lib.load()
    # the entry agrees, before it looks at a pointer; an empty problem is WM_OK, a channel count that is neither head's a refusal
    args = lambda B, C, Cout, Cdw, H, W, rows=0: (None, None, None, 1e-6, None, None, None, None, None, B, C, Cout, Cdw, H, W, rows, None)
    assert lib.wm_ln_conv1x1_dwconv_fwd(*args(0, 32, 96, 64, 8, 64)) == _lib.WM_OK
    assert lib.wm_ln_conv1x1_dwconv_fwd(*args(1, 32, 96, 64, 8, 64)) == _lib.WM_ENULL
    assert lib.wm_ln_conv1x1_dwconv_fwd(*args(1, 32, 32, 32, 8, 64)) == _lib.WM_ENULL
    assert lib.wm_ln_conv1x1_dwconv_fwd(*args(1, 16, 96, 64, 8, 64)) == _lib.WM_EUNSUPPORTED
    assert lib.wm_ln_conv1x1_dwconv_fwd(*args(1, 32, 96, 32, 8, 64)) == _lib.WM_EUNSUPPORTED
    assert lib.wm_ln_conv1x1_dwconv_fwd(*args(1, 32, 64, 64, 8, 64)) == _lib.WM_EUNSUPPORTED
    assert lib.wm_ln_conv1x1_dwconv_fwd(*args(1, 32, 96, 64, 8, 64, rows=-1)) == _lib.WM_EINVAL
    assert lib.wm_ln_conv1x1_dwconv_fwd(*args(-1, 32, 96, 64, 8, 64)) == _lib.WM_EINVAL
