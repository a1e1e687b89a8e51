"""Wide-range operands for the training convolutions and an a-priori, PER-ELEMENT error bound for them.

assert_close (conftest.py) divides by the whole tensor's norm and maximum, so an error confined to the quiet part of a tensor - one
image, one channel, a band of rows far below the largest element - does not move its figure: an fp16-split convolution that loses
the low term of every subnormal element measures the same 3e-7 as an honest one.  Here every output element is judged against a
bound computed from the OPERANDS alone (never from what the code under test gives):

    S1 = conv(|x|, |w|), SW = conv(1, |w|), SX = conv(|x|, 1)       (same zero padding), Xmax / Wmax: largest finite magnitudes

    fp16 form (conv2d.hip.h, conv2d_f16):  2^-19 S1 + 2^-38 (Xmax SW + Wmax SX)
        per product the two-term split leaves at most 3 * 2^-22 |w||x| (two residuals and the dropped lo * lo); to this comes
        2^-39 of the tensor's largest element times the other operand - half an fp16 subnormal step (2^-25) under a scale that puts
        the maximum in [2^14, 2^15) - with a factor 2 for the two roundings (hi, lo); 3 * 2^-22 -> 2^-19 is the allowance for the
        fp32 accumulation.
    bf16 form (conv2d.hip.h:13, conv_wgrad.hip.h):  2^-15 S1
        3 * 2^-18 per product, with the same kind of allowance; bf16 has fp32's exponent range, so no second term.
    a bias enters ONE fp32 sum v = conv + bias in the epilogue, rounded once: half a unit in the last place of v, at most
        2^-24 |v| <= 2^-24 (|bias| + S1).  (A kernel that adds the bias first and accumulates onto it rounds at the bias's
        magnitude with every product and does not fit this - nor does it deserve to, next to operands 2^-26 of the bias.)

The CPU emulation of the documented arithmetic (emulate_conv / emulate_wgrad) keeps the bound honest: tests/test_conv_range_cpu.py
shows that the documented form stays inside it and that a form which flushes fp16 subnormals, or leaves one of the three products
out, does not.
"""
import math

import torch
import torch.nn.functional as F


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def banded(shape, seed):
    """randn (B, C, H, W) with the last batch image at 2^-20 (B > 1), channel C // 3 of image 0 at 2^-12 and rows H // 3 .. 2H // 3 of
    image 0 at 2^-26: a few loud entries and a long quiet tail, as a gradient map has."""
    B, C, H, W = shape
    x = torch.randn(*shape, generator=_gen(seed))
    if B > 1:
        x[B - 1] *= 2.0 ** -20
    x[0, C // 3] *= 2.0 ** -12
    x[0, :, H // 3:2 * H // 3] *= 2.0 ** -26
    return x


def banded_weight(Cout, Cin, ks, seed):
    """randn / (ks sqrt(Cin)) with output channel 3 at 2^-18 and input channel 7 at 2^-9 (where they exist)."""
    w = torch.randn(Cout, Cin, ks, ks, generator=_gen(seed)) / (ks * math.sqrt(Cin))
    if Cout > 3:
        w[3] *= 2.0 ** -18
    if Cin > 7:
        w[:, 7] *= 2.0 ** -9
    return w


def _fin_abs64(t):
    a = t.detach().double().cpu().abs()
    return torch.where(torch.isfinite(a), a, torch.zeros_like(a))


def conv_ref64(x, w, ks, bias=None):
    """The float64 convolution (stride 1, zero padding ks // 2) on the CPU."""
    return F.conv2d(x.detach().double().cpu(), w.detach().double().cpu(), None if bias is None else bias.detach().double().cpu(),
                    padding=ks // 2)


def dgrad_weight(w):
    """The input-gradient convolution's weight of a forward (Cout, Cin, ks, ks) weight: transposed, rotated by 180 degrees."""
    return w.transpose(0, 1).flip(2, 3).contiguous()


def conv_bound(x, w, ks, form, bias=None):
    """float64 (B, Cout, H, W): the error bound per output element of y = conv(x, w) (+ bias) in `form` ("f16" | "bf16"), from the
    operands alone; non-finite elements of x count as absent (Xmax is taken over the finite ones).  The input gradient of a forward
    weight is conv_bound(gy, dgrad_weight(w), ...): the roles of Cin and Cout exchanged."""
    ax, aw = _fin_abs64(x), _fin_abs64(w)
    s1 = F.conv2d(ax, aw, padding=ks // 2)
    if form == "bf16":
        bound = 2.0 ** -15 * s1
    elif form == "f16":
        sw = F.conv2d(torch.ones_like(ax), aw, padding=ks // 2)
        sx = F.conv2d(ax, torch.ones_like(aw), padding=ks // 2)
        bound = 2.0 ** -19 * s1 + 2.0 ** -38 * (float(ax.max()) * sw + float(aw.max()) * sx)
    else:
        raise ValueError(form)
    if bias is not None:
        bound = bound + 2.0 ** -24 * (bias.detach().double().cpu().abs().view(1, -1, 1, 1) + s1)
    return bound


def wgrad_ref64(gy, x, ks):
    """float64 dW (Cout, Cin, ks, ks) of a stride-1 'same' convolution from gy (B, Cout, H, W) and x (B, Cin, H, W), on the CPU."""
    return _wgrad(gy.detach().double().cpu(), x.detach().double().cpu(), ks)


def _wgrad(gy, x, ks):
    w = torch.zeros(gy.shape[1], x.shape[1], ks, ks, dtype=x.dtype, requires_grad=True)
    dw, = torch.autograd.grad(F.conv2d(x, w, None, padding=ks // 2), w, gy)
    return dw


def wgrad_bound(gy, x, ks, form="bf16"):
    """The weight-gradient analogue, per entry of dW: 2^-15 S1w with S1w = wgrad(|gy|, |x|) (conv2d_wgrad is the bf16 form)."""
    if form != "bf16":
        raise ValueError(form)
    return 2.0 ** -15 * _wgrad(_fin_abs64(gy), _fin_abs64(x), ks)


def worst_ratio(got, ref64, bound):
    """(worst |got - ref| / bound over EVERY element, its index); a non-finite `got` where the reference is finite counts as inf,
    a zero bound admits only an exact result."""
    got, ref64, bound = got.detach().double().cpu(), ref64.detach().double().cpu(), bound.detach().double().cpu()
    assert got.shape == ref64.shape == bound.shape, f"shapes {tuple(got.shape)} / {tuple(ref64.shape)} / {tuple(bound.shape)}"
    err = (got - ref64).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)                 # 0 / 0 -> 0, e / 0 -> inf
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf")))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    flat = int(ratio.argmax())
    return float(ratio.flatten()[flat]), tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape))


def assert_within(got, ref64, bound, what):
    """Every element of `got` within `bound` of `ref64`; none is left out.  -> the worst ratio (for the record)."""
    r, idx = worst_ratio(got, ref64, bound)
    if not r <= 1.0:
        g, t, b = (float(v.detach().double().cpu()[idx]) for v in (got, ref64, bound))
        n_bad = int((((got.detach().double().cpu() - ref64.double().cpu()).abs() > bound.double().cpu())
                     | ~torch.isfinite(got.detach().cpu())).sum())
        raise AssertionError(f"{what}: worst error / bound {r:.3g} at {idx} (got {g!r}, float64 {t!r}, bound {b:.3e}); "
                             f"{n_bad} of {got.numel()} elements exceed the bound")
    return r


# ------------------------------------------------------------------------------------------------
# the documented arithmetic, emulated on the CPU
# ------------------------------------------------------------------------------------------------
def pow2_scale(amax):
    """cv_pow2_scale: the power of two that puts amax in [2^14, 2^15)."""
    if not (amax > 0.0) or not (amax < 3.0e38):
        return 1.0
    _, e = math.frexp(amax)
    return math.ldexp(1.0, max(-100, min(100, 15 - e)))


def _split(v, dtype, flush):
    """v (fp32) -> (hi, lo) as fp32 holding `dtype` values; flush: fp16 values below 2^-14 (subnormals) become zero."""
    def rnd(t):
        r = t.to(dtype).float()
        return torch.where(r.abs() < 2.0 ** -14, torch.zeros_like(r), r) if flush else r
    hi = rnd(v)
    return hi, rnd(v - hi)


PRODUCTS = ("hi*hi", "hi*lo", "lo*hi")                   # (weight part) * (input part), the kernels' order (cv_mma3)


def emulate_conv(x, w, ks, form="f16", flush=False, drop=None):
    """conv2d_f16 / the bf16 form as documented, in fp32 on the CPU: both operands split into two terms (under the per-tensor
    power-of-two scales for fp16), three fp32 convolutions w_hi x_hi + w_hi x_lo + w_lo x_hi, the result times 1 / (s_x s_w).
    flush: every fp16 value below 2^-14 is zero (a conversion or a matrix instruction that flushes subnormals); drop: one of
    PRODUCTS is left out."""
    x, w = x.float(), w.float()
    f16 = form == "f16"
    sx = pow2_scale(float(_fin_abs64(x).max())) if f16 else 1.0
    sw = pow2_scale(float(_fin_abs64(w).max())) if f16 else 1.0
    dt = torch.float16 if f16 else torch.bfloat16
    xh, xl = _split(x * sx, dt, flush and f16)
    wh, wl = _split(w * sw, dt, flush and f16)
    acc = None
    for name, (wp, xp) in zip(PRODUCTS, ((wh, xh), (wh, xl), (wl, xh))):
        if name == drop:
            continue
        t = F.conv2d(xp, wp, padding=ks // 2)
        acc = t if acc is None else acc + t
    return acc * (1.0 / (sx * sw))


def emulate_wgrad(gy, x, ks, drop=None):
    """conv2d_wgrad as documented (conv_wgrad.hip.h): bf16 split of both operands, gy_hi x_hi + gy_hi x_lo + gy_lo x_hi in fp32."""
    gh, gl = _split(gy.float(), torch.bfloat16, False)
    xh, xl = _split(x.float(), torch.bfloat16, False)
    acc = None
    for name, (gp, xp) in zip(PRODUCTS, ((gh, xh), (gh, xl), (gl, xh))):
        if name == drop:
            continue
        t = _wgrad(gp, xp, ks)
        acc = t if acc is None else acc + t
    return acc


def quiet_outputs(shape):
    """bool (B, 1, H, W): outputs of a banded(shape) map that lie in its quiet regions - the last image, and the rows of image 0
    strictly inside the 2^-26 band (every tap of a 3x3 window in the band)."""
    B, _, H, W = shape
    q = torch.zeros(B, 1, H, W, dtype=torch.bool)
    if B > 1:
        q[B - 1] = True
    q[0, :, H // 3 + 1:2 * H // 3 - 1] = True
    return q
