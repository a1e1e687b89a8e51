"""CPU: the C-ABI shared library loads and exports every symbol include/wavemamba_hip.h declares.
No compute calls (no GPU here) - only host-side entry points (version, strerror, workspace sizing,
argument validation that returns before any launch)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
import wave_mamba_amd as wm
from wave_mamba_amd import _lib


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "wavemamba_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(wm_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    names = declared_symbols()
    assert len(names) >= 12
    for n in names:
        assert hasattr(lib, n), f"libwavemamba_hip.so does not export {n}"
    assert set(_lib.SIGNATURES) == set(names), "ctypes binding and header disagree"


def test_host_side_entry_points():
    lib = _lib.load()
    assert lib.wm_abi_version() == _lib.ABI_VERSION
    assert lib.wm_strerror(0) == b"ok"
    assert b"shape" in lib.wm_strerror(-1)
    # workspace sizing is pure host arithmetic: UHD level-1 scan (B=1, KD=256, L=2,088,960)
    ws = lib.wm_selscan_fwd_workspace_bytes(1, 256, 2088960, 16, 4)
    assert 0 < ws < 512 * 2 ** 20
    assert lib.wm_selscan_fwd_workspace_bytes(1, 256, 32, 16, 4) == 0       # single chunk
    assert lib.wm_selscan_fwd_workspace_bytes(1, 256, 1024, 64, 4) == 0      # N > 32 unsupported -> 0


def test_argument_validation_returns_before_launch():
    lib = _lib.load()
    # odd H: the reference raises RuntimeError (strided slices disagree); here WM_EINVAL
    assert lib.wm_dwt2d_fwd(None, None, None, None, None, 1, 1, 5, 4, 0, None) == -1
    # NULL tensors
    assert lib.wm_dwt2d_fwd(None, None, None, None, None, 1, 1, 4, 4, 0, None) == -2
    assert lib.wm_selscan_fwd(*([None] * 10), None, 0, 1, 8, 16, 4, 2, 1, None) == -2
    assert lib.wm_selscan_fwd(*([None] * 10), None, 0, 1, 8, 16, 4, 3, 1, None) == -1   # dim % G
    assert lib.wm_selscan_fwd(*([None] * 10), None, 0, 1, 8, 16, 40, 2, 1, None) == -5  # N > 32
    # the 3x3 kernel selector is host state: 0 / 1 / 2 accepted, anything else WM_EINVAL (and the mode stays)
    assert lib.wm_conv2d_select(3) == -1 and lib.wm_conv2d_select(-1) == -1
    assert lib.wm_conv2d_select(2) == 0 and lib.wm_conv2d_select(1) == 0 and lib.wm_conv2d_select(0) == 0
    # convolution arguments are checked before any device work: kernel size, NULLs, fragment alignment
    assert lib.wm_conv2d_fwd(*([None] * 8), 1, 32, 0, 0, 32, 8, 8, 5, None) == -5           # ks = 5
    assert lib.wm_conv2d_fwd(*([None] * 8), 1, 32, 0, 0, 32, 8, 8, 3, None) == -2           # NULL tensors
    assert lib.wm_conv2d_fwd(*([None] * 8), 0, 32, 0, 0, 32, 8, 8, 3, None) == 0            # empty batch
    # empty problems are a no-op
    assert lib.wm_dwt2d_fwd(None, None, None, None, None, 0, 3, 4, 4, 0, None) == 0
    assert lib.wm_selscan_fwd(*([None] * 10), None, 0, 0, 8, 16, 4, 2, 1, None) == 0


def test_deterministic_forms_and_gathers_validate_before_launch():
    """The wm_*_det entry points and the channel gathers refuse a negative size, a NULL output and an unsupported width by host
    arithmetic alone, and their workspace queries answer 0 for an empty or unsupported shape (the refusals that need real device
    buffers - a short or NULL workspace, the gather's M limit, an odd pointer: tests/test_deterministic_reference.py, on the GPU)."""
    lib = _lib.load()
    N, EINVAL, ENULL, EUNSUP = None, _lib.WM_EINVAL, _lib.WM_ENULL, _lib.WM_EUNSUPPORTED
    assert lib.wm_dwconv3x3_wgrad_det(N, N, N, N, N, 0, -1, 4, 6, 8, N) == EINVAL
    assert lib.wm_dwconv3x3_wgrad_det(N, N, N, N, N, 0, 2, 4, 6, 8, N) == ENULL
    assert lib.wm_dwconv3x3_wgrad_det(N, N, N, N, N, 0, 2, 0, 6, 8, N) == 0                   # no channel: nothing to write
    assert lib.wm_layernorm2d_bwd_det(N, N, N, 1e-6, N, N, N, N, 0, -1, 35, 16, N) == EINVAL
    assert lib.wm_layernorm2d_bwd_det(N, N, N, 1e-6, N, N, N, N, 0, 2, 35, 12, N) == EUNSUP
    assert lib.wm_layernorm2d_bwd_det(N, N, N, 1e-6, N, N, N, N, 0, 2, 35, 16, N) == ENULL
    assert lib.wm_layernorm_tok_bwd_det(N, N, N, 1e-5, N, N, N, N, 0, -1, 16, N) == EINVAL
    assert lib.wm_layernorm_tok_bwd_det(N, N, N, 1e-5, N, N, N, N, 0, 37, 12, N) == EUNSUP
    assert lib.wm_layernorm_tok_bwd_det(N, N, N, 1e-5, N, N, N, N, 0, 37, 16, N) == ENULL
    assert lib.wm_linear_wgrad_det(N, N, N, N, 0, -1, 16, 16, N) == EINVAL
    assert lib.wm_linear_wgrad_det(N, N, N, N, 0, 100, 16, 16, N) == ENULL
    assert lib.wm_plane_sums_det(N, N, N, 0, -1, 3, 5, 7, N) == EINVAL
    assert lib.wm_plane_sums_det(N, N, N, 0, 2, 3, 5, 7, N) == ENULL
    assert lib.wm_plane_sums_det(N, N, N, 0, 2, 0, 5, 7, N) == 0
    assert lib.wm_scale_add_bwd_det(N, N, N, N, N, N, 0, 2, 4, -1, N) == EINVAL
    assert lib.wm_scale_add_bwd_det(N, N, N, N, N, N, 0, 2, 4, 35, N) == ENULL
    assert lib.wm_l1_mean_fwd_det(N, N, N, N, 0, -1, N) == EINVAL
    assert lib.wm_l1_mean_fwd_det(N, N, N, N, 0, 1000, N) == ENULL
    scan = lambda batch, dim, L, n, G: lib.wm_selscan_bwd_det(*([N] * 15), N, 0, batch, dim, L, n, G, 1, N)
    assert scan(-1, 8, 20, 4, 2) == EINVAL and scan(1, 8, 20, 4, 3) == EINVAL                 # a negative size; dim % G
    assert scan(1, 8, 20, 40, 2) == EUNSUP and scan(1, 8, 20, 4, 2) == ENULL                  # N > 32; NULL tensors
    assert scan(0, 8, 20, 4, 2) == 0                                                          # empty, and nothing to zero (NULL outputs)
    assert lib.wm_dwconv3x3_wgrad_det_workspace_bytes(0, 4, 6, 8) == 0 and lib.wm_dwconv3x3_wgrad_det_workspace_bytes(2, 4, 6, 8) > 0
    assert lib.wm_layernorm2d_bwd_det_workspace_bytes(2, 35, 12) == 0 and lib.wm_layernorm_tok_bwd_det_workspace_bytes(37, 12) == 0
    assert lib.wm_linear_wgrad_det_workspace_bytes(100, 15, 16) == 0 and lib.wm_linear_wgrad_det_workspace_bytes(100, 16, 16) == 16 * 16 * 4
    assert lib.wm_plane_sums_det_workspace_bytes(2, 3, 5, 0) == 0 and lib.wm_scale_add_bwd_det_workspace_bytes(0, 4, 35) == 0
    assert lib.wm_l1_mean_fwd_det_workspace_bytes(0) == 0 and lib.wm_l1_mean_fwd_det_workspace_bytes(5) == 4096
    assert lib.wm_selscan_bwd_det_workspace_bytes(1, 8, 20, 40, 2) == 0 and lib.wm_selscan_bwd_det_workspace_bytes(1, 8, 20, 4, 2) > 0
    # the channel gathers: a negative size, C = 0 with something to gather, NULL tensors; empty problems are a no-op
    assert lib.wm_channel_gather_fwd(N, N, N, 1, 2, -1, 4, N) == EINVAL and lib.wm_channel_gather_bwd(N, N, N, 1, 2, 5, -4, N) == EINVAL
    assert lib.wm_channel_gather_fwd(N, N, N, 1, 0, 5, 4, N) == EINVAL
    assert lib.wm_channel_gather_fwd(N, N, N, 1, 2, 5, 4, N) == ENULL and lib.wm_channel_gather_bwd(N, N, N, 1, 2, 5, 4, N) == ENULL
    assert lib.wm_channel_gather_fwd(N, N, N, 0, 2, 5, 4, N) == 0 and lib.wm_channel_gather_bwd(N, N, N, 1, 2, 5, 0, N) == 0


def test_conv2d_entries_and_core_return_codes_in_order():
    """Every entry over Conv2dArgs, and wm_ss2d_core_fwd, by host arithmetic alone (all pointers NULL): the code for each refusal and
    the order in which the refusals are reached - a bad dimension, then the entry's unsupported form, then an empty problem (WM_OK),
    then a NULL tensor.  The order is observable: a case that fails two checks answers with the earlier one."""
    lib = _lib.load()
    N, OK, EINVAL, ENULL, EUNSUP = None, _lib.WM_OK, _lib.WM_EINVAL, _lib.WM_ENULL, _lib.WM_EUNSUPPORTED

    def conv(B=1, Ca=32, Cb=0, Cb_src=0, Cout=32, H=8, W=8, ks=3):
        return lib.wm_conv2d_fwd(*[N] * 8, B, Ca, Cb, Cb_src, Cout, H, W, ks, N)
    assert conv(B=-1) == EINVAL and conv(Cb=-1) == EINVAL and conv(Cb_src=-1) == EINVAL and conv(Ca=0) == EINVAL and conv(Ca=-4) == EINVAL
    assert conv(Cout=0) == EINVAL and conv(H=-1) == EINVAL and conv(W=-1) == EINVAL
    assert conv(B=-1, ks=5) == EINVAL                                      # a bad dimension precedes the unsupported form
    assert conv(ks=5) == EUNSUP and conv(ks=0) == EUNSUP and conv(ks=2) == EUNSUP
    assert conv(ks=5, B=0) == EUNSUP                                       # ... which precedes the empty check
    assert conv(B=0) == OK and conv(H=0) == OK and conv(W=0) == OK and conv(B=0, ks=1) == OK
    assert conv(B=0, Cb=16) == OK                                          # ... which precedes the NULL check
    assert conv() == ENULL and conv(ks=1) == ENULL
    assert conv(Cb=16, Cb_src=16) == ENULL                                 # Cb > 0 with a NULL xb
    assert conv(Ca=36, Cb=16, Cb_src=16) == ENULL                          # (before the Ca % 8 rule of the second source)
    assert conv(B=65536) == ENULL and conv(H=1 << 16, W=1 << 15) == ENULL  # (before the size limits)

    def ln(B=1, Cin=32, Cout=32, H=8, W=8):
        return lib.wm_conv2d_ln_fwd(N, N, N, 1e-6, N, N, N, N, B, Cin, Cout, H, W, N)
    assert ln(B=-1) == EINVAL and ln(Cin=0) == EINVAL and ln(Cout=0) == EINVAL and ln(H=-1) == EINVAL and ln(W=-1) == EINVAL
    assert ln(B=-1, Cin=16) == EINVAL
    assert ln(Cin=16) == EUNSUP and ln(Cin=64) == EUNSUP and ln(Cin=16, B=0) == EUNSUP
    assert ln(B=0) == OK and ln(H=0) == OK and ln(W=0) == OK
    assert ln() == ENULL and ln(Cout=96) == ENULL and ln(B=65536) == ENULL

    def f16(B=1, Cin=32, Cout=32, H=8, W=8, ks=3, dgrad=0):
        return lib.wm_conv2d_f16_steps(*[N] * 6, B, Cin, Cout, H, W, ks, dgrad, N)
    assert f16(H=-1) == EINVAL and f16(B=-1) == EINVAL and f16(Cin=0) == EINVAL and f16(Cout=0) == EINVAL and f16(W=-1) == EINVAL
    assert f16(H=-1, ks=5) == EINVAL
    assert f16(ks=5) == EUNSUP and f16(ks=5, B=0) == EUNSUP
    assert f16(B=0) == OK and f16(H=0) == OK and f16(W=0) == OK and f16(B=0, ks=1) == OK
    assert f16() == ENULL and f16(ks=1) == ENULL and f16(dgrad=1) == ENULL

    def cdwt(B=1, Cin=3, Cout=32, H=8, W=8, dtype=_lib.WM_F32):
        return lib.wm_conv2d_dwt_fwd(*[N] * 7, B, Cin, Cout, H, W, dtype, N)
    assert cdwt(B=-1) == EINVAL and cdwt(Cin=0) == EINVAL and cdwt(Cout=0) == EINVAL
    assert cdwt(H=7) == EINVAL and cdwt(W=7) == EINVAL
    assert cdwt(H=7, Cout=64) == EINVAL and cdwt(H=7, dtype=_lib.WM_BF16) == EINVAL   # an odd side precedes the unsupported form
    assert cdwt(Cout=64) == EUNSUP and cdwt(dtype=_lib.WM_BF16) == EUNSUP
    assert cdwt(Cout=64, B=0) == EUNSUP
    assert cdwt(B=0) == OK and cdwt(H=0) == OK and cdwt(W=0) == OK
    assert cdwt() == ENULL and cdwt(Cin=32) == ENULL and cdwt(B=65536) == ENULL

    def idwtc(B=1, Cin=32, Cout=32, H=8, W=8, dtype=_lib.WM_F32):
        return lib.wm_idwt_conv2d_fwd(*[N] * 6, B, Cin, Cout, H, W, dtype, N)
    assert idwtc(B=-1) == EINVAL and idwtc(Cin=0) == EINVAL and idwtc(Cout=0) == EINVAL
    assert idwtc(W=7) == EINVAL and idwtc(H=7) == EINVAL and idwtc(W=7, Cin=16) == EINVAL
    assert idwtc(Cin=16) == EUNSUP and idwtc(dtype=_lib.WM_BF16) == EUNSUP and idwtc(Cin=16, B=0) == EUNSUP
    assert idwtc(B=0) == OK and idwtc(H=0) == OK and idwtc(W=0) == OK
    assert idwtc() == ENULL and idwtc(Cout=3) == ENULL and idwtc(B=65536) == ENULL

    def gated(B=1, Ca=32, Cb=0, Cb_src=0, Cout=32, H=8, W=8):
        return lib.wm_conv2d_gated_fwd(*[N] * 7, B, Ca, Cb, Cb_src, Cout, H, W, N)
    assert gated(Cout=0) == EINVAL and gated(B=-1) == EINVAL and gated(Ca=0) == EINVAL and gated(Cb=-1) == EINVAL
    assert gated(Cb_src=-1) == EINVAL and gated(H=-1) == EINVAL and gated(W=-1) == EINVAL
    assert gated(Cout=0, B=0) == EINVAL
    assert gated(B=0) == OK and gated(H=0) == OK and gated(W=0) == OK and gated(B=0, Cb=16) == OK
    assert gated() == ENULL and gated(Cout=64) == ENULL
    assert gated(Cb=16, Cb_src=16) == ENULL and gated(Ca=36, Cb=16, Cb_src=16) == ENULL and gated(B=65536) == ENULL

    # the SS2D core's launch: an empty problem answers first here, then the plane dtype and the plan's limits, then the NULLs
    def core(B=1, D=64, H=8, W=8, n=16, R=2, dtype=_lib.WM_F32, merged=1):
        return lib.wm_ss2d_core_fwd(*[N] * 10, merged, N, 0, N, B, D, H, W, n, R, dtype, N)
    assert core(n=33) == EUNSUP and core(n=64) == EUNSUP and core(dtype=2) == EUNSUP
    assert core(B=0) == OK and core(H=0) == OK and core(B=0, n=33) == OK
    assert core(B=0, H=-1) == EINVAL
    assert core() == ENULL and core(n=32) == ENULL and core(merged=0) == ENULL and core(dtype=_lib.WM_BF16) == ENULL


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libwavemamba_hip.so")
    with pytest.raises(_lib.WaveMambaHipError):
        _lib.load()


def test_core_work_split_is_consistent():
    """wm_ss2d_core_plan (host-only): the work split wm_ss2d_core_fwd uses covers the map exactly once in every direction,
    is the same on every call (the search result is cached per shape), and the UHD level-1 launch is not the 480 equal
    workgroups of round 2 (two dispatch rounds, the second 7/8 full) but column workgroups + shorter row workgroups."""
    import ctypes
    from wave_mamba_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_int * 10)()
    for (B, H, W, N) in [(1, 1088, 1920, 16), (1, 544, 960, 16), (1, 272, 480, 16), (1, 2048, 2048, 32), (8, 256, 256, 16),
                         (2, 24, 40, 16), (1, 8, 12, 16), (1, 33, 72, 32), (1, 16, 2048, 16), (1, 8192, 16, 16),
                         (1, 10, 14, 16), (1, 9, 7, 32), (2, 33, 71, 16), (1, 1, 1, 16)]:      # odd widths: same plan, element-wise tiles
        assert lib.wm_ss2d_core_plan(B, 64, H, W, N, 2, out) == 0
        nw, seg, nseg, ctiles, cwgs, rchunk, rnchunks, rwgs, grid, span = list(out)
        L = H * W
        assert nw == (16 if N <= 16 else 8)
        assert seg % 16 == 0 and seg * nseg >= H and seg * (nseg - 1) < H            # column segments tile the rows
        assert ctiles * nw >= W and (ctiles - 1) * nw < W and cwgs >= ctiles * nseg and cwgs % 8 == 0
        assert rchunk % 16 == 0 and rchunk * rnchunks >= L and rchunk * (rnchunks - 1) < L
        assert rwgs * nw >= rnchunks and grid == B * (2 * rwgs + 2 * cwgs) and span > 0
        again = (ctypes.c_int * 10)()
        assert lib.wm_ss2d_core_plan(B, 64, H, W, N, 2, again) == 0 and list(again) == list(out)
    assert lib.wm_ss2d_core_plan(1, 64, 1088, 1920, 16, 2, out) == 0
    assert out[2] == 1 and out[5] // 16 < 1088 // 16            # one segment per column; row chunks shorter than a column
    assert lib.wm_ss2d_core_plan(1, 64, 8, 8, 64, 2, out) == -5        # N > 32
    assert lib.wm_ss2d_core_prep_bytes(16) > 0 and lib.wm_ss2d_core_prep_bytes(33) == 0


def test_core_plan_cache_keeps_serving_new_shapes():
    """the plan cache stopped inserting at 256 shapes, so every later shape re-ran the list-scheduling search on
    every call (5-18 ms under a global mutex, 14 core calls per image).  It is an LRU now: after far more distinct shapes
    than it holds, a NEW shape is searched once and then served from the cache, and plans are unchanged by eviction."""
    import ctypes
    import time
    from wave_mamba_amd import _lib
    lib = _lib.load()
    out, again = (ctypes.c_int * 10)(), (ctypes.c_int * 10)()
    assert lib.wm_ss2d_core_plan(1, 64, 272, 480, 16, 2, out) == 0
    first = list(out)
    for i in range(1300):                                        # > the cache's 1024 entries, all distinct (small maps: fast searches)
        assert lib.wm_ss2d_core_plan(1, 64, 16 + 8 * (i % 50), 16 + 4 * (i // 50), 16, 2, again) == 0
    t0 = time.perf_counter()
    assert lib.wm_ss2d_core_plan(1, 64, 1096, 1928, 16, 2, again) == 0          # a new, UHD-sized shape: searched now
    cold = time.perf_counter() - t0
    t0 = time.perf_counter()
    for _ in range(20):
        assert lib.wm_ss2d_core_plan(1, 64, 1096, 1928, 16, 2, out) == 0 and list(out) == list(again)
    warm = (time.perf_counter() - t0) / 20
    assert warm < 2e-3 and warm < 0.5 * max(cold, 4e-3), (cold, warm)           # cached: no search per call
    assert lib.wm_ss2d_core_plan(1, 64, 272, 480, 16, 2, out) == 0 and list(out) == first   # evicted and re-planned: same plan


def test_library_isa_has_no_scalar_source_packed_f32_with_routed_halves():
    """tools/lint_packed_f32.py on the built library: `v_pk_{fma,mul,add}_f32` with a scalar source (SGPR pair / inline constant)
    AND a VGPR source read through op_sel = 1 returns a zero half in lanes 48..63 on MI355X while LDS-fed MFMAs of another kernel
    share the SIMD (tools/ubench_pk_coexec.hip, profiles/r05/) - the multi-stream mismatch of rounds 4-5.  The library must not
    contain the form; the lint's pattern matcher is checked on the instruction that did the damage."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import lint_packed_f32 as lint
    finally:
        sys.path.pop(0)
    sample = ("0000000000001000 <_ZN2wm16dwconv3x3_kernelILi1ELb1EtEEvPKT1_PKfS5_PS1_iiix>:\n"
              "\tv_pk_fma_f32 v[42:43], s[48:49], v[20:21], v[42:43] op_sel:[0,0,1] op_sel_hi:[1,1,0] // 000000001000: D3B0402A 1CAA2830\n"
              "\tv_pk_fma_f32 v[42:43], s[76:77], v[24:25], v[42:43]\n"
              "\tv_pk_fma_f32 v[50:51], v[26:27], v[48:49], v[50:51] op_sel:[0,0,1] op_sel_hi:[1,1,0]\n"
              "\tv_pk_mul_f32 v[48:49], v[48:49], s[18:19] op_sel_hi:[1,0]\n"
              "\tv_pk_fma_f32 v[6:7], v[8:9], 2.0, v[6:7] op_sel:[0,0,1] op_sel_hi:[1,0,0]\n"
              "\tv_pk_add_f32 v[10:11], v[12:13], v[10:11] op_sel:[0,1] op_sel_hi:[1,0]\n"
              "\tv_pk_mul_f32 v[14:15], v[14:15], v[16:17] op_sel:[1,0]\n"
              "\tv_pk_fma_f32 v[18:19], s[2:3], v[20:21], v[18:19] op_sel_hi:[1,0,1]\n")
    hits = lint.offending(sample)
    # flagged: the dwconv3x3<bf16> form, (conservatively) the all-VGPR swap, the inline-constant form, round 4's v_pk_add_f32
    assert [h[1].split()[1] for h in hits] == ["v[42:43],", "v[50:51],", "v[6:7],", "v[10:11],"], hits
    if not os.path.exists(os.path.join(lint.LLVM, "llvm-objdump")):
        pytest.skip("llvm-objdump not available")
    from wave_mamba_amd import build
    texts = lint.disassemble_all(_lib.LIB_PATH)             # one device code object per translation unit: all of them are read
    print(f"ISA lint: {len(texts)} device code objects in {_lib.LIB_PATH}")
    assert len(texts) == len(build.units()), (len(texts), build.units())
    bad = [b for t in texts for b in lint.offending(t)]
    assert not bad, f"{len(bad)} packed-fp32 instruction(s) with unsafe op_sel routing, first: {bad[0]}"


def test_zero_arena_registry_bookkeeping():
    """wm_zero_arena_register / _unregister (include/wavemamba_hip.h): pure host bookkeeping, so it runs without a GPU - empty and
    overlapping ranges and unknown bases are refused, a range can be registered again after it was unregistered."""
    lib = _lib.load()
    base = 0x7f0000000000
    assert lib.wm_zero_arena_register(None, 4096) == _lib.WM_ENULL
    assert lib.wm_zero_arena_register(base, 0) == _lib.WM_EINVAL
    assert lib.wm_zero_arena_register(base, 4096) == _lib.WM_OK
    try:
        assert lib.wm_zero_arena_register(base + 4000, 4096) == _lib.WM_EINVAL          # overlaps the tail
        assert lib.wm_zero_arena_register(base - 100, 200) == _lib.WM_EINVAL            # overlaps the head
        assert lib.wm_zero_arena_register(base + 4096, 4096) == _lib.WM_OK              # adjacent: fine
        assert lib.wm_zero_arena_unregister(base + 4096) == _lib.WM_OK
        assert lib.wm_zero_arena_unregister(base + 8) == _lib.WM_EINVAL                 # not a base
    finally:
        assert lib.wm_zero_arena_unregister(base) == _lib.WM_OK
    assert lib.wm_zero_arena_unregister(base) == _lib.WM_EINVAL
    assert lib.wm_zero_arena_register(base, 64) == _lib.WM_OK and lib.wm_zero_arena_unregister(base) == _lib.WM_OK


def declared_prototypes():
    """include/wavemamba_hip.h -> {name: (return kind, [argument kinds])}, a kind being 'pointer' or the C scalar type."""
    text = open(os.path.join(ROOT, "include", "wavemamba_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)

    def kind(decl, named):
        if "*" in decl or "[" in decl:
            return "pointer"
        words = [w for w in decl.split() if w != "const"]
        return " ".join(words[:-1] if named else words)

    protos = {}
    for ret, name, args in re.findall(r"^([A-Za-z_][\w \t\*]*?)\s*\b(wm_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text, flags=re.M):
        args = [a.strip() for a in args.split(",")]
        if args in ([""], ["void"]):
            args = []
        assert name not in protos, f"{name} is declared twice"
        protos[name] = (kind(ret, False), [kind(a, True) for a in args])
    return protos


def ctypes_kind(t):
    scalars = {ctypes.c_int: "int", ctypes.c_int64: "int64_t", ctypes.c_size_t: "size_t", ctypes.c_float: "float",
               ctypes.c_uint: "unsigned", None: "void"}
    if t in scalars:                                # (c_size_t is an alias of an integer type distinct from c_int / c_int64 here)
        return scalars[t]
    assert t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer), t
    return "pointer"


def test_binding_signatures_match_the_header_argument_by_argument():
    """_lib.SIGNATURES against the prototypes of include/wavemamba_hip.h, position by position: the argument count, each argument's
    kind (pointer, int, int64_t, size_t, float, unsigned) and the return kind.  A wrong type or count in the binding would shift
    every later argument of a launch; the set of names alone (above) would not notice."""
    assert len({ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_uint, ctypes.c_float}) == 5
    protos = declared_prototypes()
    assert set(protos) == set(declared_symbols()) == set(_lib.SIGNATURES)
    assert len(protos) >= 63
    for name, (ret, args) in protos.items():
        res, argtypes = _lib.SIGNATURES[name]
        assert all(k in ("pointer", "int", "int64_t", "size_t", "float", "unsigned") for k in args), (name, args)
        assert ctypes_kind(res) == ret, f"{name}: the binding returns {ctypes_kind(res)}, the header {ret}"
        assert len(argtypes) == len(args), f"{name}: the binding passes {len(argtypes)} arguments, the header takes {len(args)}"
        for i, (t, k) in enumerate(zip(argtypes, args)):
            assert ctypes_kind(t) == k, f"{name}: argument {i} is {ctypes_kind(t)} in the binding, {k} in the header"


def test_launch_names_in_ops_are_bound_entry_points():
    """wave_mamba_amd/ops.py names the entry point of every launch as a string (ops._launch looks it up and reports errors
    under it): every such literal is a key of _lib.SIGNATURES whose last argument is the stream, and nothing launches otherwise."""
    import ast
    tree = ast.parse(open(os.path.join(ROOT, "wave_mamba_amd", "ops.py")).read())
    launched = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "_launch":
            name = node.args[1]
            assert isinstance(name, ast.Constant) and isinstance(name.value, str), f"line {node.lineno}: the name must be a literal"
            launched.append(name.value)
        if isinstance(node, ast.Constant) and isinstance(node.value, str) and re.fullmatch(r"wm_[a-z0-9_]+", node.value):
            assert node.value in _lib.SIGNATURES, f"ops.py line {node.lineno}: {node.value!r} is not an entry point of the library"
    assert len(launched) >= 45 and len(set(launched)) >= 43, sorted(set(launched))      # 45 launch sites of 43 entry points today
    for name in launched:
        assert name in _lib.SIGNATURES, f"{name!r} is launched but not bound"
        assert _lib.SIGNATURES[name][0] is ctypes.c_int and _lib.SIGNATURES[name][1][-1] is ctypes.c_void_p, name
    # no launch beside the helper: an entry point called as an attribute of the library takes no stream
    text = re.sub(r'""".*?"""', "", open(os.path.join(ROOT, "wave_mamba_amd", "ops.py")).read(), flags=re.S)
    direct = set(re.findall(r"\.(wm_[a-z0-9_]+)\b", text))
    assert direct <= {"wm_zero_arena_register", "wm_zero_arena_unregister", "wm_event_synchronize_relaxed", "wm_conv2d_select",
                      "wm_conv2d_wfrag_bytes", "wm_ss2d_core_prep_bytes", "wm_prof_enable", "wm_prof_collect"} | {
                          n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes")}, sorted(direct)
