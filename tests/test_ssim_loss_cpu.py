"""The SSIM training loss (trainer.ssim_loss = 1 - cal_ssim.SSIM(), femasr_model.py:29 / :172, pixel_ssim_opt of
train_wavemamba_uhdll.yml:99-100) without a GPU: the plain-PyTorch statement against the reference's float64 values and gradients
(tests/golden/ssim_loss.npz, made by tests/golden/make_golden_ssim_loss.py), and the trainer's `ssim_weight` plumbing.

Bars: |SSIM - SSIM_f64| <= 1e-5 (2 x the reference's own float32 error where that exceeds 5e-6); gradients per tensor, l2- and
max-abs-relative to the float64 truth, <= truth_bar(err of the reference's float32) - the project's bar of test_gpu_parity.py."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_err
import wave_mamba_amd as wm
from wave_mamba_amd import cpu_twin, trainer


def truth_bar(err_ref):
    return min(max(1e-4, 2.0 * err_ref), 5e-4)


def value_bar(err_ref):
    return 2.0 * err_ref if err_ref > 5e-6 else 1e-5


_CACHE = {}


def ssim_golden():
    """{case: {field: tensor}} of tests/golden/ssim_loss.npz (`equal` cases hold gt alone: pred is gt)."""
    if not _CACHE:
        with np.load(os.path.join(GOLDEN, "ssim_loss.npz")) as z:
            for key in z.files:
                if key == "cases":
                    continue
                case, field = key.split(".")
                _CACHE.setdefault(case, {})[field] = torch.from_numpy(z[key])
        for case, d in _CACHE.items():
            d.setdefault("pred", d["gt"].clone())
    return _CACHE


def check_case(case, d, value, g_pred, g_gt, noise_max=None):
    """An SSIM value (python float) and its two gradients against the golden case, at the issue's bars."""
    err32 = d["err32"].tolist()
    v = abs(value - float(d["ssim64"]))
    print(f"{case}: value err {v:.2e} (reference fp32 {err32[0]:.2e})")
    if case.startswith("equal"):
        assert abs(1.0 - value) <= 1e-6
        for g in (g_pred, g_gt):
            assert bool(torch.isfinite(g).all())
            print(f"{case}: max|g| {float(g.abs().max()):.2e} against 1e-4 x {noise_max:.2e}")
            assert float(g.abs().max()) <= 1e-4 * noise_max
        return
    assert v <= value_bar(err32[0]), f"{case}: SSIM {value} vs {float(d['ssim64'])}"
    for name, g, t, e in (("pred", g_pred, d["gpred64"], err32[1:3]), ("gt", g_gt, d["ggt64"], err32[3:5])):
        l2, mx = rel_err(g, t)
        print(f"{case}: d/d{name} l2 {l2:.2e} (bar {truth_bar(e[0]):.1e})  max {mx:.2e} (bar {truth_bar(e[1]):.1e})")
        assert l2 <= truth_bar(e[0]) and mx <= truth_bar(e[1]), f"{case}: d/d{name} l2 {l2:.3e} max {mx:.3e}"


def noise_max_of(cases, case):
    """max |d SSIM / d pred| of the `noise` case of the same shape: what the `equal` gradient is held against."""
    return float(cases["noise_" + case.split("_")[1]]["gpred64"].abs().max())


def test_golden_has_every_shape_and_kind():
    cases = ssim_golden()
    shapes = {tuple(d["gt"].shape) for d in cases.values()}
    assert shapes == {(1, 1, 5, 7), (1, 2, 1, 30), (1, 3, 11, 11), (2, 3, 33, 47), (2, 3, 40, 130)}
    assert {c.split("_")[0] for c in cases} == {"noise", "smooth", "flat", "dark", "unclamped", "equal"}
    assert os.path.getsize(os.path.join(GOLDEN, "ssim_loss.npz")) < 1_000_000


def test_window_is_the_references_float32_window():
    """cal_ssim.gaussian(11, 1.5) in float32, tap for tap: the values the HIP library holds as constants (haar_image.hip)."""
    want = [float.fromhex(h) for h in ("0x1.0d956cp-10", "0x1.f1fe02p-8", "0x1.26eb18p-5", "0x1.bff0fep-4", "0x1.b43c3ep-3", "0x1.10656p-2")]
    g = cpu_twin.ssim_window_1d()
    assert g.dtype == torch.float32 and g.tolist() == want + want[-2::-1]


@pytest.mark.parametrize("case", sorted(ssim_golden()))
def test_ssim_loss_on_cpu_tensors_matches_the_float64_reference(case):
    cases = ssim_golden()
    d = cases[case]
    pred, gt = d["pred"].clone().requires_grad_(True), d["gt"].clone().requires_grad_(True)
    loss = trainer.ssim_loss(pred, gt)
    loss.backward()
    check_case(case, d, 1.0 - float(loss.detach()), -pred.grad, -gt.grad, noise_max_of(cases, case) if case.startswith("equal") else None)
    # the loss is 1 - SSIM, in the inputs' dtype.  float64 inputs are held to the same value bar, not to rounding: the reference
    # filters with float32(g_i g_j), 121 separately rounded products, the row and column passes with g_i and g_j - on the flat
    # 40 x 130 case that alone is 6e-7 of the value
    l32 = trainer.ssim_loss(d["pred"], d["gt"])
    l64 = trainer.ssim_loss(d["pred"].double(), d["gt"].double())
    assert l32.dtype == torch.float32 and l32.dim() == 0 and l64.dtype == torch.float64
    assert abs(float(l64) - (1.0 - float(d["ssim64"]))) <= value_bar(d["err32"].tolist()[0])


def test_ssim_loss_refuses_what_is_not_a_pair_of_image_batches():
    a = torch.rand(1, 3, 8, 8)
    with pytest.raises(RuntimeError):
        trainer.ssim_loss(a, torch.rand(1, 3, 8, 9))
    with pytest.raises(RuntimeError):
        trainer.ssim_loss(a[0], a[0])
    with pytest.raises(RuntimeError):
        trainer.ssim_loss(a[:0], a[:0])
    with pytest.raises(RuntimeError):
        wm.ops.ssim_mean(a, a)                                   # CPU tensors never reach the HIP path


def test_losses_arity_with_and_without_an_ssim_weight():
    g = torch.Generator().manual_seed(1)
    out, gt = torch.rand(1, 3, 16, 20, generator=g), torch.rand(1, 3, 16, 20, generator=g)
    two = trainer.losses(out, gt)
    assert isinstance(two, tuple) and len(two) == 2
    l_pix, l_freq = trainer.losses(out, gt, fft_weight=0.1)     # every existing caller unpacks two
    three = trainer.losses(out, gt, ssim_weight=0.25)
    assert len(three) == 3
    assert torch.equal(three[0], l_pix) and torch.equal(three[1], l_freq)
    assert torch.equal(three[2], 0.25 * trainer.ssim_loss(out, gt))
    assert float(trainer.losses(out, gt, ssim_weight=0.0)[2]) == 0.0      # a weight of 0 is still a third term


def test_train_step_with_an_ssim_weight_reports_l_ssim_and_leaves_the_other_terms():
    cfg = dict(in_chn=3, wf=8, n_l_blocks=[1, 1, 1], n_h_blocks=[1, 1, 1], ffn_scale=2.0)
    g = torch.Generator().manual_seed(7)
    lq, gt = torch.rand(1, 3, 32, 32, generator=g), torch.rand(1, 3, 32, 32, generator=g)

    def run(weight):
        torch.manual_seed(0)
        net = wm.WaveMamba(**cfg).train()
        opt = trainer.make_optimizer(net)
        with torch.no_grad():
            first_out = net(lq)
        return [trainer.train_step(net, opt, lq, gt, ssim_weight=weight) for _ in range(2)], first_out, net
    plain, out0, net_p = run(None)
    with_ssim, out1, net_s = run(0.25)
    assert torch.equal(out0, out1)
    assert set(plain[0]) == {"l_pix", "l_freq"} and set(with_ssim[0]) == {"l_pix", "l_freq", "l_ssim"}
    assert with_ssim[0]["l_pix"] == plain[0]["l_pix"] and with_ssim[0]["l_freq"] == plain[0]["l_freq"]
    assert with_ssim[0]["l_ssim"] == pytest.approx(0.25 * float(trainer.ssim_loss(out0.double(), gt.double())), abs=1e-6)
    assert all(isinstance(v, float) for d in with_ssim for v in d.values())
    # the third term reached the weights: step 2 differs from the two-term run
    assert with_ssim[1]["l_pix"] != plain[1]["l_pix"]
    assert any(not torch.equal(p, q) for p, q in zip(net_p.parameters(), net_s.parameters()))


def test_library_op_on_cpu_tensors_is_the_twin():
    import wave_mamba_amd.torch_ops as tops
    assert "ssim_mean" in tops.OPS and "ssim_mean_backward" in tops.OPS
    d = ssim_golden()["noise_1x3x11x11"]
    a, b = d["pred"].clone().requires_grad_(True), d["gt"].clone().requires_grad_(True)
    s = torch.ops.wavemamba_hip.ssim_mean(a, b)
    s.backward()
    a2, b2 = d["pred"].clone().requires_grad_(True), d["gt"].clone().requires_grad_(True)
    s2 = cpu_twin.ssim_mean(a2, b2)
    s2.backward()
    assert torch.equal(s.detach(), s2.detach()) and torch.equal(a.grad, a2.grad) and torch.equal(b.grad, b2.grad)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x = torch.empty(2, 3, 16, 24, device="cuda")
        out = torch.ops.wavemamba_hip.ssim_mean(x, x)
        assert out.shape == () and out.dtype == torch.float32
        ga, gb = torch.ops.wavemamba_hip.ssim_mean_backward(x, x, out, True, False)
        assert tuple(ga.shape) == (2, 3, 16, 24) and tuple(gb.shape) == (0,)


def test_abi_has_the_ssim_entry_points():
    lib = wm._lib.load()
    assert wm._lib.ABI_VERSION == 34 and lib.wm_abi_version() == 34
    th, tw = wm.ops.SSIM_TILE_H, wm.ops.SSIM_TILE_W
    assert lib.wm_ssim_workspace_bytes(24, 512, 512) == 24 * ((512 + th - 1) // th) * ((512 + tw - 1) // tw) * 8
    assert lib.wm_ssim_workspace_bytes(70000, 1, 1) == 70000 * 8          # planes fold into the grid: no 65,535 limit
    assert lib.wm_ssim_workspace_bytes(0, 8, 8) == 0 and lib.wm_ssim_workspace_bytes(1, 0, 8) == 0
    assert lib.wm_ssim_workspace_bytes(1 << 40, 8, 8) == 0                # more tiles than a grid holds
    # 256 threads a tile and fewer than 2^32 threads a launch: 2^24 - 1 tiles at the most
    assert lib.wm_ssim_workspace_bytes((1 << 24) - 1, 1, 1) == ((1 << 24) - 1) * 8 and lib.wm_ssim_workspace_bytes(1 << 24, 1, 1) == 0
    assert lib.wm_ssim_workspace_bytes(1 << 22, th + 1, tw + 1) == 0 and lib.wm_ssim_workspace_bytes((1 << 22) - 1, th + 1, tw + 1) > 0
    p = (1 << 20)
    assert lib.wm_ssim_mean_fwd(None, None, None, None, None, None, None, None, 0, 0, 8, 8, None) == wm._lib.WM_EINVAL
    assert lib.wm_ssim_mean_fwd(None, None, None, None, None, None, None, None, 0, 1, 8, 8, None) == wm._lib.WM_ENULL
    assert lib.wm_ssim_mean_fwd(p, p, p, None, None, None, None, p, 0, 1 << 40, 8, 8, None) == wm._lib.WM_EUNSUPPORTED
    assert lib.wm_ssim_mean_fwd(p, p, p, None, None, None, None, p + 4, 8, 1, 8, 8, None) == wm._lib.WM_EALIGN
    assert lib.wm_ssim_mean_fwd(p, p, p, None, None, None, None, p, 7, 1, 8, 8, None) == wm._lib.WM_EWORKSPACE
    assert lib.wm_ssim_mean_fwd(p, p, p, p, None, None, None, p, 8, 1, 8, 8, None) == wm._lib.WM_ENULL      # p1 without q, r
    assert lib.wm_ssim_mean_bwd(p, p, p, p, p, p, None, 1, 8, 8, None) == wm._lib.WM_ENULL
    assert lib.wm_ssim_mean_bwd(p, p, p, p, p, p, p, 1, 8, 0, None) == wm._lib.WM_EINVAL
