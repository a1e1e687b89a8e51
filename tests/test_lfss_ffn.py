"""GPU: the gated ffn of an LFSSBlock as one kernel (wm_lfss_ffn_fwd: ln_2 -> conv1 -> depth-wise 3x3 -> GELU gate -> conv3 -> skip, f
never stored) behind the middle kernel that ends at tok1 (wm_lfss_mid_rz_tok_fwd), against the pair they replace (wm_lfss_mid_rz_fwd's
f stage, then wm_lfss_out_conv_fwd): equal bit for bit on fp32 planes, at the kernel, the block and the model; against the float64
composition; write coverage; status codes."""
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
TOL = 1e-4                  # test_gpu_parity.py::test_lfss_glue_kernels_c32_vs_fp64's bar for these kernels
C, D = 32, 64
WM_OK, WM_ENULL, WM_EUNSUPPORTED = _lib.WM_OK, _lib.WM_ENULL, _lib.WM_EUNSUPPORTED


def band_rows(B, H, W):
    rb = _lib.load().wm_lfss_ffn_band_rows(B, H, W)
    assert rb > 0
    return rb


def block(width=32):
    torch.manual_seed(11)
    blk = arch.LFSSBlock(width, expand=2.0).eval().to(DEV)
    with torch.no_grad():
        for p in blk.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return blk


@functools.lru_cache(maxsize=None)
def params():
    """The ffn's parameters, perturbed from the default initialisation."""
    blk, w = block(), wm.ops._w
    ff = blk.conv_blk
    return dict(ln2_w=w(blk.ln_2.weight), ln2_b=w(blk.ln_2.bias), eps=float(blk.ln_2.eps), W1=w(ff.conv1.weight).reshape(D, C),
                b1=w(ff.conv1.bias), cw=w(ff.conv2.weight), cb=w(ff.conv2.bias), W3=w(ff.conv3.weight).reshape(C, C),
                b3=w(ff.conv3.bias), skip2=w(blk.skip_scale2))


@functools.lru_cache(maxsize=None)
def case(B, H, W):
    """tok1 (B, L, C) with one image row scaled x 30 (a band or strip that took its halo from the wrong row shows)."""
    g = torch.Generator(device=DEV); g.manual_seed(B * 1009 + H * 31 + W)
    t = torch.randn(B, H, W, C, device=DEV, generator=g)
    t[:, H // 2] *= 30.0
    return t.reshape(B, H * W, C)


def fused(tok1, B, H, W, nchw, bias, fill=float("nan"), rows=0):
    from wave_mamba_amd.ops import _ptr, _stream, check
    p = params()
    out = torch.full((B, C, H, W) if nchw else (B, H * W, C), fill, device=DEV)
    check(_lib.load().wm_lfss_ffn_fwd(_ptr(tok1), _ptr(p["ln2_w"]), _ptr(p["ln2_b"]), p["eps"], _ptr(p["W1"]), _ptr(p["b1"]), _ptr(p["cw"]),
                                      _ptr(p["cb"]) if bias else None, _ptr(p["W3"]), _ptr(p["b3"]), _ptr(p["skip2"]), _ptr(out), int(nchw),
                                      B, H, W, C, 0, rows, _stream()), "wm_lfss_ffn_fwd")
    return out


def pair(tok1, B, H, W, nchw, bias):
    """The existing entries: wm_lfss_mid_rz_fwd on a zero core output, a zero out_proj and a unit skip scale passes its token input
    through as tok1 bit for bit and writes f = conv1(ln_2(tok1)); wm_lfss_out_conv_fwd closes the block from f and tok1."""
    from wave_mamba_amd.ops import _ptr, _stream, check
    lib, p, L = _lib.load(), params(), H * W
    ones, zeros = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    y = torch.zeros(B, D, L, device=DEV)
    Win, Wout = torch.zeros(2 * D, C, device=DEV), torch.zeros(C, D, device=DEV)
    t1 = torch.full((B, L, C), float("nan"), device=DEV)
    f = torch.full((B, D, H, W), float("nan"), device=DEV)
    check(lib.wm_lfss_mid_rz_fwd(_ptr(y), 1, 0, _ptr(tok1), 0, _ptr(ones), _ptr(zeros), 1e-5, _ptr(Win), _ptr(ones), _ptr(zeros), 1e-5,
                                 _ptr(Wout), _ptr(ones), _ptr(p["ln2_w"]), _ptr(p["ln2_b"]), p["eps"], _ptr(p["W1"]), _ptr(p["b1"]), _ptr(t1),
                                 _ptr(f), B, L, C, 0, _stream()), "wm_lfss_mid_rz_fwd")
    assert torch.equal(t1, tok1), "the middle kernel did not pass the tokens through"
    out = torch.full((B, C, H, W) if nchw else (B, L, C), float("nan"), device=DEV)
    check(lib.wm_lfss_out_conv_fwd(_ptr(f), _ptr(p["cw"]), _ptr(p["cb"]) if bias else None, _ptr(tok1), _ptr(p["W3"]), _ptr(p["b3"]),
                                   _ptr(p["skip2"]), _ptr(out), int(nchw), B, H, W, C, 0, _stream()), "wm_lfss_out_conv_fwd")
    return out


SHAPES = [(1, 1, 32), (1, 2, 64), (2, 3, 32), (1, 5, 64), (1, 9, 128), (1, 40, 96), (2, 33, 160)]
SEAMS = ["rb-1", "rb", "rb+1", "2rb+1"]                       # band seams at W = 64, rb from the library's plan


def seam_shape(which):
    rb = band_rows(1, 8, 64)
    H = {"rb-1": rb - 1, "rb": rb, "rb+1": rb + 1, "2rb+1": 2 * rb + 1}[which]
    assert band_rows(1, H, 64) == rb, "the plan's band height moved with H: pick the seam heights from the plan at each H"
    return (1, H, 64)


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("nchw", [False, True], ids=["tokens", "nchw"])
@pytest.mark.parametrize("shape", SHAPES + SEAMS, ids=str)
def test_kernel_bit_identical_to_the_pair(shape, nchw, bias):
    B, H, W = seam_shape(shape) if isinstance(shape, str) else shape
    tok1 = case(B, H, W)
    got, want = fused(tok1, B, H, W, nchw, bias), pair(tok1, B, H, W, nchw, bias)
    assert not torch.isnan(want).any()
    assert not torch.isnan(got).any(), "an output element was never written"
    assert torch.equal(got, want), f"max abs difference {float((got - want).abs().max()):.3e}"


@pytest.mark.parametrize("shape,nchw", [((1, 1088, 1920), True), ((1, 544, 960), False)], ids=str)
def test_kernel_bit_identical_at_the_shipped_band_heights(shape, nchw):
    """The two UHD maps whose bands are taller than the small maps' above (the plan's choice) and whose launches fill the chip."""
    B, H, W = shape
    assert band_rows(B, H, W) > band_rows(1, 8, 64)
    tok1 = case(B, H, W)
    got, want = fused(tok1, B, H, W, nchw, True), pair(tok1, B, H, W, nchw, True)
    assert not torch.isnan(got).any(), "an output element was never written"
    assert torch.equal(got, want)


@pytest.mark.parametrize("tok_nchw", [0, 1])
@pytest.mark.parametrize("shape", [(1, 9, 128), (2, 33, 160), (1, 272, 480)], ids=str)
def test_tok1_of_the_middle_kernel_without_f(shape, tok_nchw):
    from wave_mamba_amd.ops import _ptr, _stream, check
    B, H, W = shape
    L = H * W
    lib, blk, w = _lib.load(), block(), wm.ops._w
    ss = blk.self_attention
    g = torch.Generator(device=DEV); g.manual_seed(5 + H)
    y4 = torch.randn(4, B, D, L, device=DEV, generator=g)
    tok = torch.randn(B, C, L, device=DEV, generator=g) if tok_nchw else torch.randn(B, L, C, device=DEV, generator=g)
    head = (_ptr(y4), 4, B * D * L, _ptr(tok), tok_nchw, _ptr(w(blk.ln_1.weight)), _ptr(w(blk.ln_1.bias)), float(blk.ln_1.eps),
            _ptr(w(ss.in_proj.weight)), _ptr(w(ss.out_norm.weight)), _ptr(w(ss.out_norm.bias)), float(ss.out_norm.eps),
            _ptr(w(ss.out_proj.weight)), _ptr(w(blk.skip_scale)))
    p = params()
    want, f = torch.full((B, L, C), float("nan"), device=DEV), torch.empty(B, D, L, device=DEV)
    got = torch.full((B, L, C), float("nan"), device=DEV)
    check(lib.wm_lfss_mid_rz_fwd(*head, _ptr(p["ln2_w"]), _ptr(p["ln2_b"]), p["eps"], _ptr(p["W1"]), _ptr(p["b1"]), _ptr(want), _ptr(f),
                                 B, L, C, 0, _stream()), "wm_lfss_mid_rz_fwd")
    check(lib.wm_lfss_mid_rz_tok_fwd(*head, _ptr(got), B, L, C, 0, _stream()), "wm_lfss_mid_rz_tok_fwd")
    assert not torch.isnan(want).any()
    assert torch.equal(got, want)


@pytest.mark.parametrize("nchw", [False, True], ids=["tokens", "nchw"])
@pytest.mark.parametrize("shape", [(1, 9, 128), (2, 33, 160)], ids=str)
def test_kernel_vs_fp64(shape, nchw):
    """LayerNorm -> linear -> depth-wise 3x3 with zero padding -> GELU gate -> linear -> skip in float64."""
    B, H, W = shape
    tok1, p = case(B, H, W), params()
    d = lambda t: t.double()
    f = F.linear(F.layer_norm(d(tok1), (C,), d(p["ln2_w"]), d(p["ln2_b"]), p["eps"]), d(p["W1"]), d(p["b1"]))
    fc = F.conv2d(f.transpose(1, 2).reshape(B, D, H, W), d(p["cw"]), d(p["cb"]), padding=1, groups=D)
    gated = (F.gelu(fc[:, :C]) * fc[:, C:]).reshape(B, C, H * W).transpose(1, 2)
    want = d(tok1) * d(p["skip2"]) + F.linear(gated, d(p["W3"]), d(p["b3"]))
    if nchw:
        want = want.transpose(1, 2).reshape(B, C, H, W)
    assert_close(fused(tok1, B, H, W, nchw, True), want.float(), TOL, "lfss_ffn tok2")


def block_forward(blk, x, H, W, nchw, fuse):
    """ops.lfss_block_forward with the one-kernel ffn on every map the entry supports (fuse) or on none; returns the output and the
    library entry points the call launched."""
    ops = wm.ops
    launched = []
    real = ops._launch

    def spy(dev, name, *a, **k):
        launched.append(name)
        return real(dev, name, *a, **k)

    saved = ops._FUSE_FFN, ops._FUSE_FFN_MIN_POSITIONS, ops._launch
    ops._FUSE_FFN, ops._FUSE_FFN_MIN_POSITIONS, ops._launch = fuse, 0, spy
    try:
        with torch.no_grad():
            out = ops.lfss_block_forward(x, (H, W), blk, tok_nchw=nchw, out_nchw=nchw)
    finally:
        ops._FUSE_FFN, ops._FUSE_FFN_MIN_POSITIONS, ops._launch = saved
    return out, launched


NEW = ("wm_lfss_mid_rz_tok_fwd", "wm_lfss_ffn_fwd")
OLD = ("wm_lfss_mid_rz_fwd", "wm_lfss_out_conv_fwd")


@pytest.mark.parametrize("B,H,W,nchw", [(1, 40, 96, True), (2, 33, 32, False), (2, 5, 64, False), (1, 272, 480, True)])
def test_block_bit_identical(B, H, W, nchw):
    blk = block()
    x = torch.randn(B, 32, H, W, device=DEV) if nchw else torch.randn(B, H * W, 32, device=DEV)
    got, names = block_forward(blk, x, H, W, nchw, True)
    want, names_pair = block_forward(blk, x, H, W, nchw, False)
    assert all(n in names for n in NEW) and not any(n in names for n in OLD)
    assert all(n in names_pair for n in OLD) and not any(n in names_pair for n in NEW)
    assert torch.equal(got, want), f"max abs difference {float((got - want).abs().max()):.3e}"


def test_block_fallback():
    """A width outside the entry's domain and a C = 16 block take the old launches whatever the switch says."""
    blk = block()
    x = torch.randn(1, 12 * 40, 32, device=DEV)
    got, names = block_forward(blk, x, 12, 40, False, True)
    want, _ = block_forward(blk, x, 12, 40, False, False)
    assert "wm_lfss_mid_rz_fwd" in names and not any(n in names for n in NEW)
    assert torch.equal(got, want)
    blk16 = block(16)
    x = torch.randn(1, 8 * 32, 16, device=DEV)
    got, names = block_forward(blk16, x, 8, 32, False, True)
    want, _ = block_forward(blk16, x, 8, 32, False, False)
    assert "wm_lfss_mid_fwd" in names and not any(n in names for n in NEW)
    assert torch.equal(got, want)


def test_model_bit_identical(monkeypatch):
    """The shipped config on a 256 x 256 image: the rule forced on against the switch off; the shipped rule keeps maps this small on
    the old pair."""
    ops = wm.ops
    torch.manual_seed(0)
    net = wm.WaveMamba(in_chn=3, wf=32, n_l_blocks=[1, 2, 4], n_h_blocks=[1, 1, 2], ffn_scale=2.0).to(DEV).eval()
    x = torch.rand(1, 3, 256, 256, device=DEV)
    names = []
    real = ops._launch

    def spy(dev, name, *a, **k):
        names.append(name)
        return real(dev, name, *a, **k)

    monkeypatch.setattr(ops, "_launch", spy)
    with torch.no_grad():
        shipped = net(x)
        assert not any(n in names for n in NEW)
        del names[:]
        monkeypatch.setattr(ops, "_FUSE_FFN_MIN_POSITIONS", 0)
        monkeypatch.setattr(ops, "_FUSE_FFN", True)
        got = net(x)
        n_new = names.count("wm_lfss_ffn_fwd")
        assert n_new >= 7 and names.count("wm_lfss_mid_rz_tok_fwd") == n_new and not any(n in names for n in OLD)   # 1 + 2 + 4 blocks
        del names[:]
        monkeypatch.setattr(ops, "_FUSE_FFN", False)
        want = net(x)
        assert names.count("wm_lfss_out_conv_fwd") == n_new and not any(n in names for n in NEW)
    assert torch.equal(got, want), f"max abs difference {float((got - want).abs().max()):.3e}"
    assert torch.equal(got, shipped)


def test_every_element_written_and_nothing_else():
    B, H, W = 2, 33, 160
    tok1 = case(B, H, W)
    for nchw in (False, True):
        assert torch.equal(fused(tok1, B, H, W, nchw, True, fill=0.0), fused(tok1, B, H, W, nchw, True))


def test_status_codes():
    from wave_mamba_amd.ops import _ptr, _stream
    lib, p = _lib.load(), params()
    tok1, out = torch.randn(1, 8 * 64, C, device=DEV), torch.empty(1, 8 * 64, C, device=DEV)
    def call(B, H, W, Cc, dtype=0, t=tok1, o=out):
        return lib.wm_lfss_ffn_fwd(_ptr(t), _ptr(p["ln2_w"]), _ptr(p["ln2_b"]), p["eps"], _ptr(p["W1"]), _ptr(p["b1"]), _ptr(p["cw"]),
                                   _ptr(p["cb"]), _ptr(p["W3"]), _ptr(p["b3"]), _ptr(p["skip2"]), _ptr(o), 0, B, H, W, Cc, dtype, 0, _stream())
    assert call(1, 8, 64, 16) == WM_EUNSUPPORTED             # C = 16
    assert call(1, 8, 40, 32) == WM_EUNSUPPORTED             # a width without a tile form (W % 32 != 0)
    assert call(1, 8, 64, 32, 1) == WM_EUNSUPPORTED          # bf16 planes
    assert call(0, 8, 64, 32) == WM_OK and call(1, 0, 64, 32) == WM_OK
    assert call(0, 8, 64, 32, t=None, o=None) == WM_OK       # empty: before any pointer is looked at
    assert call(1, 8, 64, 32, t=None) == WM_ENULL and call(1, 8, 64, 32, o=None) == WM_ENULL
    assert lib.wm_lfss_ffn_band_rows(1, 8, 40) == WM_EUNSUPPORTED
    tok_args = [None, 4, 0, None, 0, None, None, 1e-5, None, None, None, 1e-5, None, None, None]
    assert lib.wm_lfss_mid_rz_tok_fwd(*tok_args, 1, 64, 16, 0, None) == WM_EUNSUPPORTED
    assert lib.wm_lfss_mid_rz_tok_fwd(*tok_args, 1, 64, 32, 1, None) == WM_EUNSUPPORTED
    assert lib.wm_lfss_mid_rz_tok_fwd(*tok_args, 0, 64, 32, 0, None) == WM_OK
    assert lib.wm_lfss_mid_rz_tok_fwd(*tok_args, 1, 64, 32, 0, None) == WM_ENULL
