"""GPU: the bf16-plane kernels against their fp32 forms, bit for bit.

The bf16-storage mode (`ops.set_plane_dtype(torch.bfloat16)`) runs every kernel it touches as the same
template as the kernel's fp32 form, with TP = bf16_t: a plane element is widened to fp32 when it is read
(`ld1`, `load4`, `load8`) and rounded once to nearest even when it is written (`st1`, `store4`, `store8`:
`float_to_bf16_bits`, csrc/haar.hip.h).  That gives each bf16 entry point an exact oracle:

    bf16 form(x) == fp32 form(x.float()) with every plane output rounded once (.bfloat16());
    outputs that are fp32 (tok1, out, the IWT output) are bit-equal.

The mode's own bars (rel-l2 2e-2 per block, PSNR >= 40 dB for the network: test_gpu_parity.py) measure what bf16 costs
anyway; a defect smaller than that cost - a store that truncates instead of rounding, a plane read from the wrong
direction, a ragged edge left unwritten - shows only against this oracle.  Every bf16 check here has a float64 partner
for the fp32 form it is held to (here, or in test_gpu_parity.py where one exists).

"Bit-equal" is torch.equal on the bit patterns (`.view(int16)` / `.view(int32)`), so NaNs compare too."""
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close
from oracle import backend as oracle_backend
from test_gpu_parity import TOL, gen
import wave_mamba_amd as wm
from wave_mamba_amd import _lib
from wave_mamba_amd._lib import WM_BF16, WM_F32, check
from wave_mamba_amd.archs import wavemamba_arch as arch
from wave_mamba_amd.ops import _ptr, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def assert_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, \
        f"{what}: {tuple(got.shape)} {got.dtype} vs {tuple(want.shape)} {want.dtype}"
    it = torch.int16 if got.dtype == torch.bfloat16 else torch.int32
    a, b = got.view(it), want.view(it)
    if not torch.equal(a, b):
        bad = a != b
        first = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {a.numel()} elements differ; first at {first}: "
                             f"{float(got[first]):.9g} vs {float(want[first]):.9g}")


def misaligned(t, off):
    """A copy of t that starts `off` elements into a larger buffer (data_ptr not 16-byte aligned for off = 1..3)."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


# ------------------------------------------------------------------------------------------------
# 1. depth-wise 3x3 (wm_dwconv3x3_fwd, wm_dwconv3x3_wgrad)
# ------------------------------------------------------------------------------------------------
def dwconv_f64(x, w, b=None, act="none", flip=False):
    """F.conv2d(x, w, b, padding=1, groups=C) [+ SiLU / exact GELU] in float64, as a sum of nine shifted products
    (flip: the taps rotated by 180 degrees)."""
    x = x.double()
    B, C, H, W = x.shape
    k = w.double().reshape(C, 3, 3)
    if flip:
        k = k.flip(1, 2)
    xp = F.pad(x, (1, 1, 1, 1))
    y = torch.zeros_like(x) if b is None else b.double().view(1, C, 1, 1).expand(B, C, H, W).clone()
    for i in range(3):
        for j in range(3):
            y += k[:, i, j].view(1, C, 1, 1) * xp[:, :, i:i + H, j:j + W]
    return F.silu(y) if act == "silu" else F.gelu(y) if act == "gelu" else y


def dwconv_wgrad_f64(x, gy):
    """(dW (C, 1, 3, 3), db (C,)) of the depth-wise 3x3 in float64: dW[c, i, j] = sum gy * x shifted by (i - 1, j - 1)."""
    x, gy = x.double(), gy.double()
    B, C, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    dW = torch.stack([(gy * xp[:, :, i:i + H, j:j + W]).sum((0, 2, 3)) for i in range(3) for j in range(3)], 1)
    return dW.view(C, 1, 3, 3), gy.sum((0, 2, 3))


def check_dwconv_bf16(xb, w, b, act, flip, what):
    """xb: a bf16 map (any alignment).  bf16 form == fp32 form on the same values, rounded once; fp32 form vs float64."""
    got = wm.ops.dwconv3x3(xb, w, b, act, flip)
    xf = xb.float() if xb.data_ptr() % 16 == 0 else misaligned(xb.float(), (xb.data_ptr() % 16) // 2)
    want = wm.ops.dwconv3x3(xf, w, b, act, flip)
    assert got.dtype == torch.bfloat16
    assert_bits(got, want.bfloat16(), f"{what}: bf16 vs rounded fp32")
    assert_close(want, dwconv_f64(xb, w, b, act, flip), 1e-5, f"{what}: fp32 vs float64")


DW_SHAPES = [
    (2, 3, 5, 1), (1, 7, 2, 5), (3, 5, 1, 37),        # element-wise form (W % 4 != 0); H = 1, 2
    (3, 7, 37, 64), (1, 5, 16, 8), (2, 1, 2, 4),      # 16 lanes per row, 4 planes per wave: B*C = 21, 5, 2 leave the last group part-filled
    (1, 9, 20, 100), (3, 1, 1, 128),                  # 32 lanes per row, 2 planes per wave: B*C odd
    (1, 2, 33, 260), (2, 3, 1, 136),                  # 64 lanes per row (W > 128)
    (1, 3, 150, 36), (2, 2, 97, 7), (1, 1, 70, 300),  # tall maps: several row strips per plane (each form)
]


@pytest.mark.parametrize("shape", DW_SHAPES)
@pytest.mark.parametrize("act", ["none", "silu", "gelu"])
def test_dwconv3x3_bf16_is_the_rounded_fp32_form(shape, act):
    """Each dispatch form of dwconv3x3_kernel<ACT, VEC, bf16_t, LPR> (csrc/lfss.hip: dw_lanes_per_row), with and without
    bias, plain and flipped taps (act + 4)."""
    B, C, H, W = shape
    g = gen(B * 7919 + C * 131 + H * 17 + W)
    xb = torch.randn(*shape, generator=g).bfloat16().to(DEV)
    w = (torch.randn(C, 1, 3, 3, generator=g) * 0.3).to(DEV)
    b = torch.randn(C, generator=g).to(DEV)
    for flip in (False, True):
        for bias in (b, None):
            check_dwconv_bf16(xb, w, bias, act, flip, f"{shape} {act} flip={flip} bias={bias is not None}")


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("act", ["none", "silu"])
def test_dwconv3x3_bf16_misaligned_view(off, act):
    """A bf16 map that starts 1-3 elements into its buffer (W % 4 == 0, but not 16-byte aligned) takes the element-wise
    form; several row strips, so the strips' halo rows are read."""
    g = gen(100 + off)
    x = torch.randn(2, 3, 41, 40, generator=g).bfloat16().to(DEV)
    w = (torch.randn(3, 1, 3, 3, generator=g) * 0.3).to(DEV)
    b = torch.randn(3, generator=g).to(DEV)
    xb = misaligned(x, off)
    assert xb.data_ptr() % 16 != 0
    for flip in (False, True):
        check_dwconv_bf16(xb, w, b, act, flip, f"offset {off} {act} flip={flip}")


@pytest.mark.parametrize("W", [20, 19])
def test_dwconv3x3_bf16_inf_and_nan(W):
    """One plane holds +inf, -inf and NaN: whatever the fp32 form makes of them, the bf16 form stores the same, rounded
    (NaN as the canonical 0x7fc0 on both sides).  The other planes against float64."""
    g = gen(W)
    x = torch.randn(2, 4, 12, W, generator=g)
    x[0, 0, 3, 4], x[0, 0, 7, 10], x[0, 0, 9, 15] = float("inf"), float("-inf"), NAN
    xb = x.bfloat16().to(DEV)
    w = (torch.randn(4, 1, 3, 3, generator=g) * 0.3).to(DEV)
    b = torch.randn(4, generator=g).to(DEV)
    for act in ("none", "silu", "gelu"):
        for flip in (False, True):
            got = wm.ops.dwconv3x3(xb, w, b, act, flip)
            want = wm.ops.dwconv3x3(xb.float(), w, b, act, flip)
            assert not torch.isfinite(want[0, 0]).all()
            assert_bits(got, want.bfloat16(), f"W={W} {act} flip={flip}")
            assert_close(want.flatten(0, 1)[1:], dwconv_f64(xb, w, b, act, flip).flatten(0, 1)[1:], 1e-5,
                         f"W={W} {act} flip={flip}: finite planes vs float64")


@pytest.mark.parametrize("shape", [(2, 131075, 3, 8),      # 16 lanes per row: 262150 planes = 65538 groups of 4
                                   (1, 65541, 5, 7)])      # element-wise form: one plane per group, 65541 groups
def test_dwconv3x3_past_the_grid_z_cap(shape):
    """wm_dwconv3x3_fwd and wm_dwconv3x3_wgrad launch at most 65535 plane groups in grid z and loop over the rest
    (csrc/lfss.hip: `pgroups < 65535 ? pgroups : 65535`): forward (fp32 and bf16), input gradient and weight / bias
    gradient past the cap, against float64."""
    B, C, H, W = shape
    g = torch.Generator(device=DEV); g.manual_seed(C)
    x = torch.randn(*shape, device=DEV, generator=g)
    w = torch.randn(C, 1, 3, 3, device=DEV, generator=g) * 0.3
    b = torch.randn(C, device=DEV, generator=g)
    gy = torch.randn(*shape, device=DEV, generator=g)
    assert_close(wm.ops.dwconv3x3(x, w, b, "silu"), dwconv_f64(x, w, b, "silu"), 1e-5, "fp32 forward")
    xb = x.bfloat16()
    check_dwconv_bf16(xb, w, b, "silu", False, "bf16 forward")
    check_dwconv_bf16(xb, w, None, "none", True, "bf16 forward, flipped, no bias")
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    dx, dW, db = torch.autograd.grad(wm.ops.dwconv3x3_train(xr, wr, br), (xr, wr, br), gy)
    dW64, db64 = dwconv_wgrad_f64(x, gy)
    assert_close(dx, dwconv_f64(gy, w, None, "none", True), 1e-5, "input gradient")
    assert_close(dW, dW64, 1e-5, "weight gradient")
    assert_close(db, db64, 1e-5, "bias gradient")


# ------------------------------------------------------------------------------------------------
# 2. Haar DWT / IWT with bf16 tensors
# ------------------------------------------------------------------------------------------------
def dwt_eager(x):
    """The reference's dwt_init (wavemamba_arch.py:97-110) in the tensor's own dtype: eager bf16 rounds every op."""
    x01, x02 = x[:, :, 0::2, :] / 2, x[:, :, 1::2, :] / 2
    x1, x2, x3, x4 = x01[..., 0::2], x02[..., 0::2], x01[..., 1::2], x02[..., 1::2]
    return x1 + x2 + x3 + x4, -x1 - x2 + x3 + x4, -x1 + x2 - x3 + x4, x1 - x2 - x3 + x4


def iwt_eager(x):
    """The reference's iwt_init (:113-130): sub-band arithmetic in x's dtype, written into a float32 map."""
    B, C4, h, w = x.shape
    C = C4 // 4
    x1, x2, x3, x4 = (x[:, k * C:(k + 1) * C] / 2 for k in range(4))
    out = torch.zeros(B, C, 2 * h, 2 * w, dtype=torch.float32, device=x.device)
    out[:, :, 0::2, 0::2] = x1 - x2 - x3 + x4
    out[:, :, 1::2, 0::2] = x1 - x2 + x3 - x4
    out[:, :, 0::2, 1::2] = x1 + x2 - x3 - x4
    out[:, :, 1::2, 1::2] = x1 + x2 + x3 + x4
    return out


# (B, C, H, W) of the full-resolution map: w = W / 2 % 4 != 0 (scalar form) and == 0 (vector form); B*C*h not a multiple
# of the 4 rows of a workgroup; a sub-band row wider than 64 column groups
HAAR_SHAPES = [(3, 5, 6, 10), (2, 3, 8, 16), (1, 7, 4, 24), (3, 5, 2, 130), (1, 1, 2, 2), (2, 3, 10, 520)]


@pytest.mark.parametrize("shape", HAAR_SHAPES)
def test_haar_forward_bf16_matches_the_eager_formula(shape):
    """dwt_init / iwt_init on bf16 tensors against the reference's formulas in eager bf16 (one rounding per op) - bit-equal,
    aligned and from a misaligned view (the scalar form); the fp32 forms against float64."""
    B, C, H, W = shape
    x = torch.randn(*shape, generator=gen(H * W + C)).bfloat16()
    y = torch.randn(B, 4 * C, H // 2, W // 2, generator=gen(H * W + C + 1)).bfloat16()
    for off in (0, 1):
        xd, yd = x.to(DEV), y.to(DEV)
        if off:
            xd, yd = misaligned(xd, off), misaligned(yd, off)
        for k, (got, want) in enumerate(zip(wm.ops.dwt_init(xd), dwt_eager(x))):
            assert got.dtype == torch.bfloat16
            assert_bits(got.cpu(), want, f"dwt sub-band {k}, offset {off}")
        got = wm.ops.iwt_init(yd)
        assert got.dtype == torch.float32
        assert_bits(got.cpu(), iwt_eager(y), f"iwt, offset {off}")
    for k, (got, want) in enumerate(zip(wm.ops.dwt_init(x.float().to(DEV)), dwt_eager(x.double()))):
        assert_close(got, want, 1e-6, f"fp32 dwt sub-band {k} vs float64")
    assert_close(wm.ops.iwt_init(y.float().to(DEV)), iwt_eager(y.double()), 1e-6, "fp32 iwt vs float64")


@pytest.mark.parametrize("shape", HAAR_SHAPES)
def test_haar_backward_bf16_is_the_rounded_fp32_backward(shape):
    """Backward of dwt_init (launch_synthesis<bf16_t, bf16_t, false>) and of iwt_init (launch_analysis<float, bf16_t, false>)
    through autograd with bf16 inputs and bf16 gradient values: each equals the fp32 backward on the same values, rounded
    once.  That is this build's contract (fp32 arithmetic, one rounding), and it deliberately differs from the reference's
    eager bf16 autograd, which rounds after every op of the backward graph.  The fp32 backwards against float64."""
    B, C, H, W = shape
    g = gen(H * W + C + 7)
    x = torch.randn(*shape, generator=g).bfloat16().to(DEV).requires_grad_(True)
    outs = wm.ops.dwt_init(x)
    gs = [torch.randn(o.shape, generator=g).bfloat16().to(DEV) for o in outs]
    (dx,) = torch.autograd.grad(outs, x, gs)
    x32 = x.detach().float().requires_grad_(True)
    (dx32,) = torch.autograd.grad(wm.ops.dwt_init(x32), x32, [t.float() for t in gs])
    assert dx.dtype == torch.bfloat16
    assert_bits(dx, dx32.bfloat16(), "dwt backward")
    assert_close(dx32, iwt_eager(torch.cat(gs, 1).double()), 1e-6, "fp32 dwt backward vs float64")

    y = torch.randn(B, 4 * C, H // 2, W // 2, generator=g).bfloat16().to(DEV).requires_grad_(True)
    out = wm.ops.iwt_init(y)
    go = torch.randn(out.shape, generator=g).bfloat16().float().to(DEV)
    (dy,) = torch.autograd.grad(out, y, go)
    y32 = y.detach().float().requires_grad_(True)
    (dy32,) = torch.autograd.grad(wm.ops.iwt_init(y32), y32, go)
    assert dy.dtype == torch.bfloat16
    assert_bits(dy, dy32.bfloat16(), "iwt backward")
    assert_close(dy32, torch.cat(dwt_eager(go.double()), 1), 1e-6, "fp32 iwt backward vs float64")


# (B, C, h, w) of the sub-bands: C*h*w odd or == 4 (mod 8) - the x_h sub-band pointers are not 16-byte aligned, so the
# scalar form even at w % 4 == 0 - and a fully aligned vector case
@pytest.mark.parametrize("B,C,h,w", [(2, 3, 5, 7), (1, 1, 1, 4), (3, 1, 3, 12), (2, 4, 3, 8)])
def test_iwt_init_pair_bf16(B, C, h, w):
    """iwt_init_pair with a bf16 pair: forward against the eager formula, backward the rounded fp32 backward (as for
    iwt_init).  A mixed bf16 / fp32 pair takes the fp32 path: forward and x_h gradient bit-equal to the fp32 pair's, the
    x_l gradient that one rounded."""
    g = gen(B * 1000 + C * 100 + h * 10 + w)
    xl = torch.randn(B, C, h, w, generator=g).bfloat16()
    xh = torch.randn(B, 3 * C, h, w, generator=g).bfloat16()
    go = torch.randn(B, C, 2 * h, 2 * w, generator=g).bfloat16().float().to(DEV)
    yl, yh = (t.to(DEV).requires_grad_(True) for t in (xl, xh))
    out = wm.ops.iwt_init_pair(yl, yh)
    assert out.dtype == torch.float32
    assert_bits(out.cpu(), iwt_eager(torch.cat([xl, xh], 1)), "pair forward")
    dl, dh = torch.autograd.grad(out, (yl, yh), go)
    fl, fh = (t.detach().float().requires_grad_(True) for t in (yl, yh))
    out32 = wm.ops.iwt_init_pair(fl, fh)
    dl32, dh32 = torch.autograd.grad(out32, (fl, fh), go)
    assert dl.dtype == dh.dtype == torch.bfloat16
    assert_bits(dl, dl32.bfloat16(), "pair backward x_l")
    assert_bits(dh, dh32.bfloat16(), "pair backward x_h")
    assert_close(torch.cat([dl32, dh32], 1), torch.cat(dwt_eager(go.double()), 1), 1e-6, "fp32 pair backward vs float64")
    # mixed pair
    ml, mh = yl.detach().requires_grad_(True), fh.detach().requires_grad_(True)
    outm = wm.ops.iwt_init_pair(ml, mh)
    assert_bits(outm, out32.detach(), "mixed pair forward")
    dml, dmh = torch.autograd.grad(outm, (ml, mh), go)
    assert dml.dtype == torch.bfloat16 and dmh.dtype == torch.float32
    assert_bits(dml, dl32.bfloat16(), "mixed pair backward x_l")
    assert_bits(dmh, dh32, "mixed pair backward x_h")


# ------------------------------------------------------------------------------------------------
# 3. / 4. LFSS glue kernels at C = 32 (the fp32 matrix-core kernels of lfss_mfma.hip.h)
# ------------------------------------------------------------------------------------------------
C32, D64 = 32, 64
# L = 270001 (B = 1): 4219 groups of 64 positions, the last one 49 long.  lfss_groups_per_wave (lfss_mfma.hip.h) gives
# ceil(4219 / slots) groups per wave for slots = 1024 x waves per SIMD at the call sites: lfss_in 4096 -> 2, lfss_mid 3072 -> 2,
# lfss_mid_rz 2048 -> 3, lfss_out 2048 -> 3 - and the last waves walk fewer groups than that.
LARGE_L = 270001


def glue_params(seed):
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    C, D = C32, D64
    p = dict(ln1w=rn(C) * 0.2 + 1, ln1b=rn(C) * 0.2, ln2w=rn(C) * 0.2 + 1, ln2b=rn(C) * 0.2,
             onw=rn(D) * 0.2 + 1, onb=rn(D) * 0.2, Win=rn(2 * D, C) / 6, Wout=rn(C, D) / 8, W1=rn(D, C) / 6,
             b1=rn(D) * 0.2, W3=rn(C, C) / 6, b3=rn(C) * 0.2, sk1=rn(C) * 0.2 + 1, sk2=rn(C) * 0.2 + 1,
             w2=rn(D, 1, 3, 3) * 0.3, b2=rn(D) * 0.2)
    return p, rn


def run_in(p, tok, nchw, x, z, B, L, code):
    check(_lib.load().wm_lfss_in_fwd(_ptr(tok), int(nchw), _ptr(p["ln1w"]), _ptr(p["ln1b"]), 1e-5, _ptr(p["Win"]), _ptr(x),
                                     _ptr(z), B, L, C32, code, _stream()), "wm_lfss_in_fwd")


def run_mid(p, y, ny, ystride, z, tok, nchw, tok1, f, B, L, code, rz):
    lib = _lib.load()
    tail = (_ptr(p["onw"]), _ptr(p["onb"]), 1e-5, _ptr(p["Wout"]), _ptr(p["sk1"]), _ptr(p["ln2w"]), _ptr(p["ln2b"]), 1e-5,
            _ptr(p["W1"]), _ptr(p["b1"]), _ptr(tok1), _ptr(f), B, L, C32, code, _stream())
    if rz:
        check(lib.wm_lfss_mid_rz_fwd(_ptr(y), ny, ystride, _ptr(tok), int(nchw), _ptr(p["ln1w"]), _ptr(p["ln1b"]), 1e-5,
                                     _ptr(p["Win"]), *tail), "wm_lfss_mid_rz_fwd")
    else:
        check(lib.wm_lfss_mid_fwd(_ptr(y), ny, ystride, _ptr(z), _ptr(tok), int(nchw), *tail), "wm_lfss_mid_fwd")


def run_out(p, fc, tok1, out, nchw, B, L, code):
    check(_lib.load().wm_lfss_out_fwd(_ptr(fc), _ptr(tok1), _ptr(p["W3"]), _ptr(p["b3"]), _ptr(p["sk2"]), _ptr(out), int(nchw),
                                      B, L, C32, code, _stream()), "wm_lfss_out_fwd")


def run_out_conv(p, f, bias, tok1, out, nchw, B, H, W, code):
    check(_lib.load().wm_lfss_out_conv_fwd(_ptr(f), _ptr(p["w2"]), _ptr(bias), _ptr(tok1), _ptr(p["W3"]), _ptr(p["b3"]),
                                           _ptr(p["sk2"]), _ptr(out), int(nchw), B, H, W, C32, code, _stream()),
          "wm_lfss_out_conv_fwd")


def nans(*shape, dtype=torch.float32):
    """An output buffer pre-filled with NaN: a position a kernel leaves unwritten cannot pass for a right one."""
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def strided_planes(planes, ystride):
    """The four direction planes (4, B, D, L) at `ystride` elements from each other, NaN in between."""
    n = planes[0].numel()
    buf = torch.full((3 * ystride + n,), NAN, dtype=planes.dtype, device=planes.device)
    for q in range(4):
        buf[q * ystride:q * ystride + n] = planes[q].reshape(-1)
    return buf


GLUE_SHAPES = [(1, 1), (2, 1), (3, 37), (2, 64), (1, 1000), (3, 1000), (1, 4097), (2, 4097), (1, LARGE_L)]


@pytest.mark.parametrize("B,L", GLUE_SHAPES)
@pytest.mark.parametrize("nchw", [False, True])
def test_lfss_glue_kernels_bf16_are_the_rounded_fp32_forms(B, L, nchw):
    """wm_lfss_in_fwd (z written, and z = NULL), wm_lfss_mid_fwd and wm_lfss_mid_rz_fwd (ny = 1, and ny = 4 with the
    direction planes at ystride = B*D*L and inside a larger buffer), wm_lfss_out_fwd: WM_BF16 against WM_F32 on the same
    bf16 values.  Plane outputs (x, z, f) equal the fp32 ones rounded once; tok1 and out are bit-equal.  The fp32 forms
    take their direction planes at ystride = B*D*L, so a bf16 stride taken in the wrong units cannot agree with them.
    Float64 partners: test_lfss_glue_kernels_c32_vs_fp64 (test_gpu_parity.py) and test_lfss_glue_kernels_c32_vs_fp64_ny4_rz."""
    C, D = C32, D64
    p, rn = glue_params(B * 131 + L + 7 * nchw)
    tokens = rn(B, L, C)
    tok = tokens.transpose(1, 2).contiguous() if nchw else tokens
    # lfss_in
    x32, z32 = nans(B, D, L), nans(B, D, L)
    run_in(p, tok, nchw, x32, z32, B, L, WM_F32)
    xb, zb = nans(B, D, L, dtype=torch.bfloat16), nans(B, D, L, dtype=torch.bfloat16)
    run_in(p, tok, nchw, xb, zb, B, L, WM_BF16)
    assert_bits(xb, x32.bfloat16(), "lfss_in x"); assert_bits(zb, z32.bfloat16(), "lfss_in z")
    xb = nans(B, D, L, dtype=torch.bfloat16)
    run_in(p, tok, nchw, xb, None, B, L, WM_BF16)
    assert_bits(xb, x32.bfloat16(), "lfss_in x (z = NULL)")
    # lfss_mid, lfss_mid_rz
    S = B * D * L
    y4 = (rn(4, B, D, L) * 2).bfloat16()
    zz = (rn(B, D, L) * 2).bfloat16()
    for ny, ystride in ((1, 0), (4, S), (4, S + 4099)):
        yb = y4[0] if ny == 1 else (y4 if ystride == S else strided_planes(y4, ystride))
        y32 = y4[0].float() if ny == 1 else y4.float()
        for rz in (False, True):
            what = f"lfss_mid{'_rz' if rz else ''} ny={ny} ystride={ystride}"
            t32, f32 = nans(B, L, C), nans(B, D, L)
            run_mid(p, y32, ny, S, zz.float(), tok, nchw, t32, f32, B, L, WM_F32, rz)
            tb, fb = nans(B, L, C), nans(B, D, L, dtype=torch.bfloat16)
            run_mid(p, yb, ny, ystride, zz, tok, nchw, tb, fb, B, L, WM_BF16, rz)
            assert_bits(tb, t32, what + " tok1"); assert_bits(fb, f32.bfloat16(), what + " f")
    # lfss_out
    fc = rn(B, D, L).bfloat16()
    tok1 = rn(B, L, C)
    shape = (B, C, L) if nchw else (B, L, C)
    o32, ob = nans(*shape), nans(*shape)
    run_out(p, fc.float(), tok1, o32, nchw, B, L, WM_F32)
    run_out(p, fc, tok1, ob, nchw, B, L, WM_BF16)
    assert_bits(ob, o32, "lfss_out")


def glue_f64(p, tokens):
    """The float64 composition of reference :483-494, :524-526, :226-230 for the C = 32 kernels (as in
    test_lfss_glue_kernels_c32_vs_fp64)."""
    d = lambda t: t.double()
    C, D = C32, D64
    xz = F.linear(F.layer_norm(d(tokens), (C,), d(p["ln1w"]), d(p["ln1b"]), 1e-5), d(p["Win"])).transpose(1, 2)

    def mid(ysum, z):
        yy = F.layer_norm(d(ysum).transpose(1, 2), (D,), d(p["onw"]), d(p["onb"]), 1e-5) * F.silu(d(z).transpose(1, 2))
        t1 = d(tokens) * d(p["sk1"]) + F.linear(yy, d(p["Wout"]))
        return t1, F.linear(F.layer_norm(t1, (C,), d(p["ln2w"]), d(p["ln2b"]), 1e-5), d(p["W1"]), d(p["b1"])).transpose(1, 2)

    def out(fc, tok1):
        gg = (F.gelu(d(fc[:, :C])) * d(fc[:, C:])).transpose(1, 2)
        return d(tok1) * d(p["sk2"]) + F.linear(gg, d(p["W3"]), d(p["b3"]))
    return xz, mid, out


@pytest.mark.parametrize("B,L", [(2, 37), (3, 1000), (1, 4097), (1, LARGE_L)])
@pytest.mark.parametrize("nchw", [False, True])
def test_lfss_glue_kernels_c32_vs_fp64_ny4_rz(B, L, nchw):
    """The fp32 glue kernels as the block calls them, against the float64 composition at TOL: wm_lfss_mid_fwd and the shipped
    wm_lfss_mid_rz_fwd with ny = 4 separate direction planes (ystride = B*D*L, and inside a larger buffer), wm_lfss_mid_rz_fwd
    with ny = 1, and L = 270001, where every kernel walks several groups of 64 positions per wave with a ragged last group."""
    C, D = C32, D64
    p, rn = glue_params(B * 977 + L + 3 * nchw)
    tokens = rn(B, L, C)
    tok = tokens.transpose(1, 2).contiguous() if nchw else tokens
    xz, mid, out = glue_f64(p, tokens)
    x, z = nans(B, D, L), nans(B, D, L)
    run_in(p, tok, nchw, x, z, B, L, WM_F32)
    assert_close(x, xz[:, :D], TOL, "lfss_in x"); assert_close(z, xz[:, D:], TOL, "lfss_in z")
    S = B * D * L
    y4 = rn(4, B, D, L)
    zz = rn(B, D, L) * 2
    want = {False: mid(y4.double().sum(0), zz), True: mid(y4.double().sum(0), xz[:, D:])}
    want1 = mid(y4[0], xz[:, D:])
    tok1 = None
    for ny, ystride, rz in ((4, S, False), (4, S + 4099, False), (4, S, True), (4, S + 4099, True), (1, 0, True)):
        what = f"lfss_mid{'_rz' if rz else ''} ny={ny} ystride={ystride}"
        y = y4[0] if ny == 1 else (y4 if ystride == S else strided_planes(y4, ystride))
        t1, f = nans(B, L, C), nans(B, D, L)
        run_mid(p, y, ny, ystride, zz, tok, nchw, t1, f, B, L, WM_F32, rz)
        wt, wf = want1 if ny == 1 else want[rz]
        assert_close(t1, wt, TOL, what + " tok1"); assert_close(f, wf, TOL, what + " f")
        tok1 = t1
    fc = rn(B, D, L)
    o = nans(*((B, C, L) if nchw else (B, L, C)))
    run_out(p, fc, tok1, o, nchw, B, L, WM_F32)
    assert_close(o.transpose(1, 2) if nchw else o, out(fc, tok1), TOL, "lfss_out")


@pytest.mark.parametrize("B,H,W", [(1, 40, 96), (2, 3, 32), (1, 1, 64), (1, 5, 160), (2, 7, 192),
                                   (1, 520, 512)])                  # >= 2^18 positions, W % 64 == 0: the row-window form
@pytest.mark.parametrize("nchw", [False, True])
def test_lfss_out_conv_bf16_with_bias_is_the_rounded_fp32_form(B, H, W, nchw):
    """wm_lfss_out_conv_fwd(WM_BF16) with a conv2 bias: bit-equal to its WM_F32 form on the same bf16 f; the fp32 form with
    the bias against float64 (reference :226-230)."""
    C, D, L = C32, D64, H * W
    p, rn = glue_params(B * 1000 + H * 10 + W)
    f = rn(B, D, H, W).bfloat16()
    tok1 = rn(B, L, C)
    shape = (B, C, H, W) if nchw else (B, L, C)
    o32, ob = nans(*shape), nans(*shape)
    run_out_conv(p, f.float(), p["b2"], tok1, o32, nchw, B, H, W, WM_F32)
    run_out_conv(p, f, p["b2"], tok1, ob, nchw, B, H, W, WM_BF16)
    assert_bits(ob, o32, "lfss_out_conv bf16 vs fp32")
    fc64 = dwconv_f64(f, p["w2"], p["b2"])
    gv = F.gelu(fc64[:, :C]) * fc64[:, C:]
    want = F.conv2d(gv, p["W3"].double().view(C, C, 1, 1), p["b3"].double()) + \
        (tok1.double() * p["sk2"].double()).transpose(1, 2).reshape(B, C, H, W)
    if not nchw:
        want = want.reshape(B, C, L).transpose(1, 2)
    assert_close(o32, want, 1e-5, "lfss_out_conv fp32 with conv2 bias vs float64")


# ------------------------------------------------------------------------------------------------
# 5. / 6. the block and the network: the bf16 mode against its emulation on the fp32 kernels
# ------------------------------------------------------------------------------------------------
def emulated_bf16_block(tok, x_size, blk, tok_nchw=False, out_nchw=False):
    """ops.lfss_block_forward in the bf16-storage mode, restated on the WM_F32 kernels: the same calls in the same order,
    with `.bfloat16().float()` wherever the mode stores a plane - x (and z when ops._RECOMPUTE_Z is off) after lfss_in,
    xc after dwconv + SiLU, each of the core's four direction planes, f after the middle kernel, fc in the unfused form.
    Blocks the mode leaves in fp32 planes (C != 32, or W % 4 != 0) are not rounded."""
    ops = wm.ops
    lib = _lib.load()
    H, W = x_size
    L = H * W
    ss, ff = blk.self_attention, blk.conv_blk
    C, D = ss.d_model, ss.d_inner
    B = tok.shape[0]
    tok = tok.contiguous().float()
    dev = tok.device
    st = _stream()
    w = ops._w
    rnd = (lambda t: t.bfloat16().float()) if (C == 32 and W % 4 == 0) else (lambda t: t)
    rz = C == 32 and ops._RECOMPUTE_Z
    x = torch.empty((B, D, H, W), device=dev)
    z = None if rz else torch.empty((B, D, L), device=dev)
    check(lib.wm_lfss_in_fwd(_ptr(tok), int(tok_nchw), _ptr(w(blk.ln_1.weight)), _ptr(w(blk.ln_1.bias)), float(blk.ln_1.eps),
                             _ptr(w(ss.in_proj.weight)), _ptr(x), _ptr(z), B, L, C, WM_F32, st), "wm_lfss_in_fwd")
    x = rnd(x)
    z = None if z is None else rnd(z)
    xc = rnd(ops.dwconv3x3(x, ss.conv2d.weight, ss.conv2d.bias, "silu"))
    core_params = (ss.x_proj_weight, ss.dt_projs_weight, ss.dt_projs_bias, ss.A_logs, ss.Ds)
    y4 = ops._ss2d_core_fwd([xc] + [w(t) for t in core_params], merged=0, prepared=ops._ss2d_core_prepared(core_params))
    y4 = rnd(torch.stack(y4))                                              # (4, B, D, L)
    tok1 = torch.empty((B, L, C), device=dev)
    f = torch.empty((B, D, H, W), device=dev)
    common = (_ptr(w(ss.out_norm.weight)), _ptr(w(ss.out_norm.bias)), float(ss.out_norm.eps), _ptr(w(ss.out_proj.weight)),
              _ptr(w(blk.skip_scale)), _ptr(w(blk.ln_2.weight)), _ptr(w(blk.ln_2.bias)), float(blk.ln_2.eps),
              _ptr(w(ff.conv1.weight)), _ptr(w(ff.conv1.bias)), _ptr(tok1), _ptr(f), B, L, C, WM_F32, st)
    if rz:
        check(lib.wm_lfss_mid_rz_fwd(_ptr(y4), 4, B * D * L, _ptr(tok), int(tok_nchw), _ptr(w(blk.ln_1.weight)),
                                     _ptr(w(blk.ln_1.bias)), float(blk.ln_1.eps), _ptr(w(ss.in_proj.weight)), *common),
              "wm_lfss_mid_rz_fwd")
    else:
        check(lib.wm_lfss_mid_fwd(_ptr(y4), 4, B * D * L, _ptr(z), _ptr(tok), int(tok_nchw), *common), "wm_lfss_mid_fwd")
    f = rnd(f)
    out = torch.empty((B, C, H, W) if out_nchw else (B, L, C), device=dev)
    if C == 32 and W % 32 == 0 and ops._FUSE_OUT_CONV:
        check(lib.wm_lfss_out_conv_fwd(_ptr(f), _ptr(w(ff.conv2.weight)), None if ff.conv2.bias is None else _ptr(w(ff.conv2.bias)),
                                       _ptr(tok1), _ptr(w(ff.conv3.weight)), _ptr(w(ff.conv3.bias)), _ptr(w(blk.skip_scale2)),
                                       _ptr(out), int(out_nchw), B, H, W, C, WM_F32, st), "wm_lfss_out_conv_fwd")
        return out
    fc = rnd(ops.dwconv3x3(f, ff.conv2.weight, ff.conv2.bias, "none"))
    check(lib.wm_lfss_out_fwd(_ptr(fc), _ptr(tok1), _ptr(w(ff.conv3.weight)), _ptr(w(ff.conv3.bias)), _ptr(w(blk.skip_scale2)),
                              _ptr(out), int(out_nchw), B, L, C, WM_F32, st), "wm_lfss_out_fwd")
    return out


def random_block(C, d_state, seed):
    torch.manual_seed(seed)
    blk = arch.LFSSBlock(C, d_state=d_state, expand=2.0).eval().to(DEV)
    with torch.no_grad():
        for p in blk.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return blk


def block_forward(x, hw, blk, tok_nchw, out_nchw, plane_dtype):
    prev = wm.ops.set_plane_dtype(plane_dtype)
    try:
        return wm.ops.lfss_block_forward(x, hw, blk, tok_nchw=tok_nchw, out_nchw=out_nchw)
    finally:
        wm.ops.set_plane_dtype(prev)


@pytest.mark.parametrize("B,H,W,N", [(1, 9, 64, 16), (2, 1, 96, 16), (2, 3, 128, 32),      # W % 32 == 0
                                     (1, 7, 36, 16), (2, 5, 44, 32), (2, 1, 40, 16)])       # W % 4 == 0, W % 32 != 0
@pytest.mark.parametrize("rz", [True, False], ids=["rz", "stored_z"])
@pytest.mark.parametrize("fuse", [True, False], ids=["fused_out", "unfused_out"])
@pytest.mark.parametrize("layout", [(False, False), (True, False), (True, True)], ids=["tok-tok", "nchw-tok", "nchw-nchw"])
def test_lfss_block_bf16_mode_is_the_emulated_block(B, H, W, N, rz, fuse, layout):
    """ops.lfss_block_forward with bf16 planes is bit-equal to emulated_bf16_block.  W % 4 == 0 with W % 32 != 0 (and
    ops._FUSE_OUT_CONV = False) takes dwconv3x3<bf16> + lfss_out_mfma_kernel<bf16_t>; most L = H*W here leave the last
    group of 64 positions ragged; H = 1; d_state 16 and 32."""
    blk = random_block(32, N, seed=H * W + N)
    tok_nchw, out_nchw = layout
    x = torch.randn((B, 32, H, W) if tok_nchw else (B, H * W, 32), generator=gen(B + H + W)).to(DEV)
    prev = (wm.ops._RECOMPUTE_Z, wm.ops._FUSE_OUT_CONV)
    wm.ops._RECOMPUTE_Z, wm.ops._FUSE_OUT_CONV = rz, fuse
    try:
        with torch.no_grad():
            want = emulated_bf16_block(x, (H, W), blk, tok_nchw, out_nchw)
            got = block_forward(x, (H, W), blk, tok_nchw, out_nchw, torch.bfloat16)
    finally:
        wm.ops._RECOMPUTE_Z, wm.ops._FUSE_OUT_CONV = prev
    assert got.dtype == torch.float32
    assert_bits(got, want, f"bf16-mode block {B}x{H}x{W} d_state {N}")


@pytest.mark.parametrize("C,H,W", [(32, 6, 30), (32, 5, 7), (16, 8, 32), (8, 4, 64)])
def test_lfss_block_bf16_mode_falls_back_to_fp32_planes(C, H, W):
    """The mode stores bf16 planes only for C = 32 with W % 4 == 0; other blocks are bit-equal to the fp32 mode."""
    blk = random_block(C, 16, seed=C + W)
    x = torch.randn(2, H * W, C, generator=gen(C * W)).to(DEV)
    with torch.no_grad():
        for layout in ((False, False), (True, True)):
            xi = x.transpose(1, 2).reshape(2, C, H, W).contiguous() if layout[0] else x
            want = block_forward(xi, (H, W), blk, *layout, torch.float32)
            got = block_forward(xi, (H, W), blk, *layout, torch.bfloat16)
            assert_bits(got, want, f"C={C} {H}x{W} layout {layout}")


class EmulatedBf16Ops:
    """An operator backend (oracle/backend.py) that is wave_mamba_amd.ops with lfss_block_forward replaced by
    emulated_bf16_block; records the (H, W) of every block call."""

    def __init__(self):
        self.sizes = []

    def __getattr__(self, name):
        return getattr(wm.ops, name)

    def lfss_block_forward(self, tok, x_size, blk, tok_nchw=False, out_nchw=False):
        self.sizes.append(tuple(int(s) for s in x_size))
        return emulated_bf16_block(tok, x_size, blk, tok_nchw, out_nchw)


@pytest.mark.parametrize("hw", [(256, 256), (256, 288), (240, 288)])
def test_network_bf16_mode_is_the_emulated_network(hw):
    """The shipped config (wf 32, [1, 2, 4] / [1, 1, 2], ffn 2) in the bf16-storage mode is bit-equal to the fp32-plane
    network with every LFSSBlock replaced by its emulation.  The LFSS levels run at W/2, W/4 and W/8: at W = 288 at widths
    144, 72 and 36 (W % 4 == 0, W % 32 != 0: dwconv3x3<bf16> + lfss_out_mfma_kernel<bf16_t>), and at 240 x 288 two of those
    levels also end in a ragged group of 64 positions (L = 4320, 1080).  The record shows such levels occurred."""
    torch.manual_seed(0)
    net = wm.WaveMamba(in_chn=3, wf=32, n_l_blocks=[1, 2, 4], n_h_blocks=[1, 1, 2], ffn_scale=2.0).eval().to(DEV)
    img = torch.rand(1, 3, *hw, generator=gen(1234)).to(DEV)
    emu = EmulatedBf16Ops()
    assert wm.ops.get_plane_dtype() == torch.float32
    with torch.no_grad():
        with oracle_backend.ops_backend(emu):
            want = net(img)
        prev = wm.ops.set_plane_dtype(torch.bfloat16)
        try:
            got = net(img)
        finally:
            wm.ops.set_plane_dtype(prev)
    assert emu.sizes, "no LFSSBlock took the fused path"
    narrow = [(h, w) for h, w in emu.sizes if w % 4 == 0 and w % 32 != 0]
    if hw[1] % 256:                                # a level width W / 2^k that is not a multiple of 32
        assert narrow, emu.sizes
    if hw[0] == 240:
        assert any(h * w % 64 for h, w in narrow), emu.sizes
    assert_bits(got, want, f"network {hw}")
