"""Shared by tests/test_fft_loss_cpu.py and tests/test_fft_loss_gpu.py (not collected): the reference composition of FFTLoss
(basicsr/losses/losses.py:300-313), its float64 truth, and input pairs whose spectrum of pred - target has no weak bin.

Why the construction matters: the gradient of the loss is a sum of SIGNS, one per spectrum bin.  A bin whose sign is decided by
rounding moves the whole gradient by 2 / sqrt(number of bins) (3.9e-3 at 512 x 512), whichever code is right.  So a gradient test
uses inputs whose every bin is far from zero and ASSERTS that (`margin`); it never tolerates or skips on a weak bin.

Bars (the project's own, tests/test_ssim_loss_cpu.py:18-23), e_ref = the error of `reference` in fp32 on the CPU against `truth`:
    value     relative error <= 2 e_ref if e_ref > 5e-6 else 1e-5
    gradient  max |g - truth| / max |truth| <= min(max(1e-4, 2 e_ref), 5e-4)"""
import torch
import torch.nn.functional as F

from conftest import rel_err

FLAT_SEED = 7
FLAT_SHAPES = [(2, 3, 16, 16), (1, 1, 16, 32), (1, 1, 32, 16), (1, 2, 64, 128), (1, 2, 128, 64), (1, 1, 256, 16), (1, 1, 16, 256),
               (1, 2, 512, 512), (1, 1, 1024, 16), (1, 1, 16, 1024)]
RANDN_CASES = [((2, 3, 16, 16), 0), ((1, 2, 16, 64), 0), ((1, 2, 64, 16), 2), ((2, 3, 32, 32), 2)]


def value_bar(e_ref):
    return 2.0 * e_ref if e_ref > 5e-6 else 1e-5


def grad_bar(e_ref):
    return min(max(1e-4, 2.0 * e_ref), 5e-4)


def reference(pred, target):
    """FFTLoss.forward at loss_weight 1, as the reference composes it, in the tensors' dtype."""
    pf, tf = torch.fft.rfft2(pred), torch.fft.rfft2(target)
    return F.l1_loss(torch.stack([pf.real, pf.imag], dim=-1), torch.stack([tf.real, tf.imag], dim=-1))


def truth(pred, target):
    """(value as a float, d/dpred, d/dtarget) of the reference composition in float64 on the CPU."""
    p = pred.detach().cpu().double().requires_grad_(True)
    t = target.detach().cpu().double().requires_grad_(True)
    v = reference(p, t)
    gp, gt = torch.autograd.grad(v, (p, t))
    return float(v.detach()), gp, gt


def _self_conjugate(H, W):
    return [(k1, k2) for k1 in (0, H // 2) for k2 in (0, W // 2)]


def flat_pair(B, C, H, W, seed, amp=0.05):
    """(pred, target) in fp32 on the CPU whose difference has a flat-magnitude spectrum: real and imaginary part of every bin of the
    half spectrum +-U(0.5, 1.5); the columns k2 = 0 and W / 2 made Hermitian (Y[H - k1] = conj Y[k1], the four self-conjugate bins
    real) so that the half spectrum IS that of a real image; d = irfft2(Y) scaled to standard deviation amp; target = rand,
    pred = target + d (added in float64, rounded once)."""
    g = torch.Generator().manual_seed(seed)
    K = W // 2 + 1

    def part():
        mag = 0.5 + torch.rand(B, C, H, K, generator=g, dtype=torch.float64)
        return mag * (torch.randint(0, 2, (B, C, H, K), generator=g).double() * 2 - 1)
    y = torch.complex(part(), part())
    mirror = (-torch.arange(H)) % H
    upper = (torch.arange(H) > H // 2).view(1, 1, H)
    for k2 in (0, W // 2):
        col = y[:, :, :, k2]
        col = torch.where(upper, torch.conj(col[:, :, mirror]), col)
        for k1 in (0, H // 2):
            col[:, :, k1] = col[:, :, k1].real + 0j
        y[:, :, :, k2] = col
    d = torch.fft.irfft2(y, s=(H, W))
    d = d * (amp / d.std())
    target = torch.rand(B, C, H, W, generator=g)
    return (target.double() + d).float(), target


def randn_pair(shape, seed):
    """pred, then target, drawn from one generator."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g), torch.randn(shape, generator=g)


def margin(pred, target):
    """The smallest |Re| or |Im| over the float64 spectrum of pred - target (the imaginary part of the four self-conjugate bins
    left out: it is zero by construction and its sign has no derivative), divided by the largest |Y|."""
    y = torch.fft.rfft2(pred.detach().cpu().double() - target.detach().cpu().double())
    H, W = pred.shape[2:]
    im = y.imag.abs().clone()
    for k1, k2 in _self_conjugate(H, W):
        im[:, :, k1, k2] = float("inf")
    return float(torch.minimum(y.real.abs().min(), im.min()) / y.abs().max())


_CASES = {}


def case(kind, shape, seed):
    """One input pair with everything the tests compare against, computed once and shared (callers do not modify it):
    {pred, target (fp32, CPU), margin, value, gpred, gtarget (float64 truth), e_value, e_grad (the fp32 reference's errors)}."""
    key = (kind, tuple(shape), seed)
    if key not in _CASES:
        pred, target = flat_pair(*shape, seed=seed) if kind == "flat" else randn_pair(shape, seed)
        value, gp, gt = truth(pred, target)
        p32 = pred.clone().requires_grad_(True)
        v32 = reference(p32, target)
        g32, = torch.autograd.grad(v32, p32)
        _CASES[key] = dict(pred=pred, target=target, margin=margin(pred, target), value=value, gpred=gp, gtarget=gt,
                           e_value=abs(float(v32.detach()) - value) / abs(value), e_grad=rel_err(g32, gp)[1])
    return _CASES[key]


def all_cases():
    return [("flat", s, FLAT_SEED) for s in FLAT_SHAPES] + [("randn", s, seed) for s, seed in RANDN_CASES]


def case_id(c):
    return f"{c[0]}-{'x'.join(map(str, c[1]))}-s{c[2]}"


def check_margin(c):
    kind, d = c[0], case(*c)
    need = 0.1 if kind == "flat" else 1e-4
    assert d["margin"] >= need, f"{case_id(c)}: the weakest bin is {d['margin']:.3e} of the largest (needs {need}): not a gradient test"


def check_value_and_grad(c, value, gpred, what):
    """A value (python float) and a d/dpred against the float64 truth of case c, at the bars above; prints the measured errors."""
    d = case(*c)
    check_margin(c)
    ev = abs(value - d["value"]) / abs(d["value"])
    eg = rel_err(gpred, d["gpred"])[1]
    print(f"{what} {case_id(c)}: value rel err {ev:.2e} (reference fp32 {d['e_value']:.2e}, bar {value_bar(d['e_value']):.1e}); "
          f"gradient max rel err {eg:.2e} (reference fp32 {d['e_grad']:.2e}, bar {grad_bar(d['e_grad']):.1e}); margin {d['margin']:.3f}")
    assert ev <= value_bar(d["e_value"]), f"{what} {case_id(c)}: value {value} vs {d['value']}"
    assert eg <= grad_bar(d["e_grad"]), f"{what} {case_id(c)}: gradient max rel err {eg:.3e}"
