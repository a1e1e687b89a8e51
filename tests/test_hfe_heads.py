"""GPU: the two heads of an HFE block as one kernel each (wm_ln_conv1x1_dwconv_fwd: LayerNorm2d -> 1x1 -> depth-wise 3x3 on the 1x1's
first channels, the plane between the two never stored) against the two launches it replaces (wm_conv2d_ln_fwd, wm_dwconv3x3_fwd):
equal bit for bit - torch.equal, no tolerance anywhere - at the kernel, at the HFE block and at the model, and two launches fewer per
HFE block."""
import functools

import pytest
import torch

import wave_mamba_amd as wm
from wave_mamba_amd.archs import wavemamba_arch as arch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 32
ops = wm.ops
HEADS = {"qkv": (96, 64), "project_in": (32, 32)}            # head -> (Cout, channels under the depth-wise conv)
EPS = 1e-6


@functools.lru_cache(maxsize=None)
def params(head):
    cout, cdw = HEADS[head]
    g = torch.Generator(device=DEV); g.manual_seed(7 + cout)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    return dict(lw=1.0 + 0.3 * rn(C), lb=0.2 * rn(C), w=rn(cout, C, 1, 1) / C ** 0.5, b=rn(cout) * 0.2, wd=rn(cdw, 1, 3, 3) / 3,
                bd=rn(cdw) * 0.2)


@functools.lru_cache(maxsize=None)
def case(B, H, W):
    """x; one image row and one image column scaled x 30: a strip or band that took a neighbour from the wrong row or column shows."""
    g = torch.Generator(device=DEV); g.manual_seed(B * 1009 + H * 31 + W)
    x = torch.randn(B, C, H, W, device=DEV, generator=g)
    x[:, :, H // 2] *= 30.0
    x[:, :, :, W // 2] *= 30.0
    return x


@functools.lru_cache(maxsize=None)
def pair(head, shape, biases):
    """(the 1x1's own output, the pair's result): computed once per case, read by every test that needs it."""
    p, (cout, cdw) = params(head), HEADS[head]
    pre = ops.conv2d_ln(case(*shape), p["lw"], p["lb"], EPS, p["w"], p["b"] if biases else None)
    qk = ops.dwconv3x3(pre[:, :cdw].contiguous(), p["wd"], p["bd"] if biases else None)
    return pre, torch.cat([qk, pre[:, cdw:]], 1)


def fused(head, shape, biases, band_rows=0):
    p = params(head)
    return ops.ln_conv1x1_dwconv(case(*shape), p["lw"], p["lb"], EPS, p["w"], p["b"] if biases else None, p["wd"],
                                 p["bd"] if biases else None, HEADS[head][1], band_rows=band_rows)


# every tap is padding | exactly one 30-column strip, one strip plus one column, the strip seams on both sides (60 | 61, 62 | 63) |
# batch stride | several strips and bands
SHAPES = [(1, 1, 1), (1, 2, 3), (1, 3, 30), (1, 5, 31), (1, 4, 61), (1, 9, 62), (1, 7, 63), (2, 18, 70), (1, 34, 130)]


def check(head, shape, biases, band_rows=0):
    cdw = HEADS[head][1]
    pre, want = pair(head, shape, biases)
    got = fused(head, shape, biases, band_rows)
    assert torch.isfinite(want).all() and got.shape == want.shape
    assert torch.equal(got[:, :cdw], want[:, :cdw]), \
        f"depth-wise channels: max abs difference {float((got[:, :cdw] - want[:, :cdw]).abs().max()):.3e}"
    if head == "qkv":                                         # the value third: the 1x1's own output
        assert torch.equal(got[:, cdw:], pre[:, cdw:]), f"value third: max abs difference {float((got[:, cdw:] - pre[:, cdw:]).abs().max()):.3e}"
    assert torch.equal(got, fused(head, shape, biases, band_rows)), "two runs of the fused kernel differ"


@pytest.mark.parametrize("biases", [True, False], ids=["biases", "no_biases"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("head", list(HEADS))
def test_kernel_bit_identical_to_the_pair(head, shape, biases):
    check(head, shape, biases)


@pytest.mark.parametrize("biases", [True, False], ids=["biases", "no_biases"])
@pytest.mark.parametrize("head", list(HEADS))
def test_five_bands_of_two_rows(head, biases):
    """(1, 9, 64) with the band height forced to 2: five bands, the last one ragged, halo rows shared between bands."""
    check(head, (1, 9, 64), biases, band_rows=2)


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
        if not name.endswith("_prep"):                                    # (weight preparation: cached by whichever path ran first)
            names.append(name)
        return real(dev, name, *a, **k)
    ops._launch = spy
    try:
        with torch.no_grad():
            out = fn()
    finally:
        ops._launch = real
    return out, names


def lower_the_floors(monkeypatch):
    """Every HFE map to the fused heads - and to the folded value path, without which the qkv head keeps its 96-channel depth-wise conv."""
    monkeypatch.setattr(ops, "_FUSE_PW_DW_MIN_POSITIONS", {h: 0 for h in HEADS})
    monkeypatch.setattr(ops, "_FUSE_DW_PW_MIN_POSITIONS", 0)


def test_hfe_block_bit_identical_and_two_launches_fewer(monkeypatch):
    blk = hfe_block()
    g = torch.Generator(device=DEV); g.manual_seed(41)
    x = torch.randn(1, 32, 40, 72, device=DEV, generator=g)
    per = torch.randn(1, 32, 40, 72, device=DEV, generator=g)
    lower_the_floors(monkeypatch)
    got, names = launches(lambda: blk(x, per))
    got_early, _ = launches(lambda: blk(x, per, qkv=blk.qkv_of(x)))      # the qkv head issued ahead of time, as the U-Net does
    monkeypatch.setattr(ops, "_FUSE_PW_DW", False)
    want, names_pair = launches(lambda: blk(x, per))
    assert names.count("wm_ln_conv1x1_dwconv_fwd") == 2 and "wm_ln_conv1x1_dwconv_fwd" not in names_pair
    assert "wm_conv2d_ln_fwd" not in names and names_pair.count("wm_conv2d_ln_fwd") == 2
    assert len(names) == len(names_pair) - 2
    assert torch.equal(got, want), f"max abs difference {float((got - want).abs().max()):.3e}"
    assert torch.equal(got_early, want)


@pytest.mark.parametrize("two_streams", [True, False])
def test_model_bit_identical(monkeypatch, two_streams):
    """The dispatch recorder's wf = 32 model at (1, 3, 64, 128), both stream orders: every HFE map on the fused heads against the
    switch off; two launches fewer per HFE block."""
    torch.manual_seed(0)                                                  # (make_golden_dispatch.run_mode's model and input)
    net = wm.WaveMamba(in_chn=3, wf=32, n_l_blocks=[1, 1, 1], n_h_blocks=[1, 1, 1], ffn_scale=2).to(DEV).eval()
    net.restoration_network.two_streams = two_streams
    x = torch.rand(1, 3, 64, 128, device=DEV)
    shipped, names_shipped = launches(lambda: net(x))
    torch.cuda.synchronize()
    assert "wm_ln_conv1x1_dwconv_fwd" not in names_shipped               # the shipped rule keeps maps this small on the pair
    lower_the_floors(monkeypatch)
    got, names = launches(lambda: net(x))
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "_FUSE_PW_DW", False)
    want, names_pair = launches(lambda: net(x))
    torch.cuda.synchronize()
    assert names.count("wm_ln_conv1x1_dwconv_fwd") == 12                 # 6 HFE blocks, two heads each
    assert "wm_ln_conv1x1_dwconv_fwd" not in names_pair and len(names) == len(names_pair) - 12
    assert torch.equal(got, want), f"max abs difference {float((got - want).abs().max()):.3e}"
    assert torch.equal(got, shipped)
