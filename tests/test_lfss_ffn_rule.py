"""CPU: the size rule by which ops.lfss_block_forward chooses the one-kernel ffn (wm_lfss_mid_rz_tok_fwd + wm_lfss_ffn_fwd) - the
shipped switch and predicate, not a forced one - and the plan query's refusals (host arithmetic only)."""
import wave_mamba_amd as wm
from wave_mamba_amd import _lib


def test_shipped_rule_at_the_uhd_levels():
    ops = wm.ops
    assert ops._FUSE_FFN is True and ops._RECOMPUTE_Z is True
    assert ops._fuse_ffn_map(1, 1088, 1920)                  # UHD level 1: measured faster
    assert ops._fuse_ffn_map(1, 544, 960)                    # level 2: measured faster
    assert not ops._fuse_ffn_map(1, 272, 480)                # level 3: not faster
    assert not ops._fuse_ffn_map(8, 272, 480)                # a batch of level-3 maps is still level-3 maps
    assert not ops._fuse_ffn_map(1, 384, 704)                # between levels 3 and 2: not measured
    assert not ops._fuse_ffn_map(1, 1088, 1900)              # a width the entry has no tile form for
    assert not ops._fuse_ffn_map(1, 4096, 4096)              # past the entry's 2^23 positions per image


def test_band_plan_is_host_arithmetic():
    lib = _lib.load()
    for (B, H, W) in [(1, 1088, 1920), (1, 544, 960), (1, 272, 480), (1, 1, 32), (2, 33, 160)]:
        rb = lib.wm_lfss_ffn_band_rows(B, H, W)
        assert 4 <= rb <= 64, (B, H, W, rb)
        assert lib.wm_lfss_ffn_band_rows(B, H, W) == rb
    assert lib.wm_lfss_ffn_band_rows(1, 8, 40) == _lib.WM_EUNSUPPORTED
    assert lib.wm_lfss_ffn_band_rows(1, 4096, 4096) == _lib.WM_EUNSUPPORTED
    assert lib.wm_lfss_ffn_band_rows(-1, 8, 64) == _lib.WM_EINVAL
    # an empty problem is WM_OK before any pointer is looked at; outside the domain the refusal comes first
    ffn = lambda B, H, W, C: lib.wm_lfss_ffn_fwd(None, None, None, 1e-5, *([None] * 8), 0, B, H, W, C, 0, 0, None)
    assert ffn(0, 8, 64, 32) == _lib.WM_OK
    assert ffn(1, 8, 64, 16) == _lib.WM_EUNSUPPORTED
    assert ffn(1, 8, 64, 32) == _lib.WM_ENULL
