"""The FFT training loss (FFTLoss, basicsr/losses/losses.py:300-313; fft_opt of train_wavemamba_uhdll.yml:102-104) without a GPU:
the plain-PyTorch statement of the difference-first form (cpu_twin.fft_l1_mean) against the float64 truth, the library's host-only
entry points, the backend switch and its plumbing through trainer and recipe, and the torch.library ops under the CPU key.
Cases and bars: tests/fft_loss_cases.py."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import yaml

from conftest import GOLDEN, ROOT
import fft_loss_cases as fc
import wave_mamba_amd as wm
from wave_mamba_amd import _lib, cpu_twin, recipe, trainer

YAML = os.path.join(GOLDEN, "train_wavemamba_uhdll.yml")


@pytest.mark.parametrize("c", fc.all_cases(), ids=fc.case_id)
def test_twin_fp32_against_float64(c):
    d = fc.case(*c)
    p = d["pred"].clone().requires_grad_(True)
    v = cpu_twin.fft_l1_mean(p, d["target"])
    assert v.dtype == torch.float32 and v.dim() == 0
    g, = torch.autograd.grad(v, p)
    fc.check_value_and_grad(c, float(v), g, "twin fp32")


@pytest.mark.parametrize("c", [("flat", (1, 2, 64, 128), fc.FLAT_SEED), ("randn", (2, 3, 32, 32), 2), ("randn", (1, 2, 24, 40), 0)],
                         ids=fc.case_id)
def test_twin_float64_is_the_reference_composition(c):
    """Linearity: in float64 the difference-first form and the reference's two transforms agree to rounding - any H and W."""
    pred, target = fc.randn_pair(c[1], c[2]) if c[0] == "randn" else fc.flat_pair(*c[1], seed=c[2])
    p, t = pred.double().requires_grad_(True), target.double().requires_grad_(True)
    v = cpu_twin.fft_l1_mean(p, t)
    assert v.dtype == torch.float64
    gp, gt = torch.autograd.grad(v, (p, t))
    want, wp, wt = fc.truth(pred, target)
    assert abs(float(v) - want) <= 1e-12 * abs(want)
    assert float((gp - wp).abs().max()) <= 1e-12 * float(wp.abs().max())
    assert float((gt - wt).abs().max()) <= 1e-12 * float(wt.abs().max())
    assert torch.equal(gt, -gp)


def test_twin_takes_16_bit_inputs_and_refuses_bad_shapes():
    pred, target = fc.randn_pair((1, 2, 16, 16), 0)
    v = cpu_twin.fft_l1_mean(pred.bfloat16(), target.bfloat16())
    assert v.dtype == torch.bfloat16
    want = cpu_twin.fft_l1_mean(pred.bfloat16().float(), target.bfloat16().float())
    assert abs(float(v) - float(want)) <= 2 ** -8 * float(want)
    with pytest.raises(RuntimeError, match="fft_l1_mean"):
        cpu_twin.fft_l1_mean(pred[0], target[0])
    with pytest.raises(RuntimeError, match="fft_l1_mean"):
        cpu_twin.fft_l1_mean(pred, target[:, :1])


# ---- the library, host-only calls -----------------------------------------------------------------------------------------------------
SIZES = {8: 0, 16: 1, 24: 0, 512: 1, 1024: 1, 2048: 0, 0: 0, -1: 0}


def test_supported_is_exactly_the_powers_of_two_from_16_to_1024():
    lib = _lib.load()
    assert lib.wm_abi_version() == 34
    for h, oh in SIZES.items():
        for w, ow in SIZES.items():
            assert lib.wm_fft_l1_supported(h, w) == (oh & ow), (h, w)
            assert wm.ops.fft_l1_supported(h, w) == bool(oh & ow)
    for n in range(-2, 1100):
        assert lib.wm_fft_l1_supported(n, 16) == int(n in (16, 32, 64, 128, 256, 512, 1024)), n


def test_size_functions():
    lib = _lib.load()
    for h, oh in SIZES.items():
        for w, ow in SIZES.items():
            rec, ws = lib.wm_fft_l1_record_bytes(3, h, w), lib.wm_fft_l1_workspace_bytes(3, h, w)
            assert (rec > 0) == (ws > 0) == bool(oh & ow), (h, w, rec, ws)
    for planes in (0, -1, 1 << 40):                                  # nothing to do; more planes than a launch holds
        assert lib.wm_fft_l1_record_bytes(planes, 64, 64) == 0 and lib.wm_fft_l1_workspace_bytes(planes, 64, 64) == 0
    rec = [lib.wm_fft_l1_record_bytes(p, 64, 128) for p in (1, 2, 3, 7, 24, 1000)]
    ws = [lib.wm_fft_l1_workspace_bytes(p, 64, 128) for p in (1, 2, 3, 7, 24, 1000)]
    assert rec == sorted(rec) and len(set(rec)) == len(rec) and ws == sorted(ws) and len(set(ws)) == len(ws)
    assert rec[0] >= 64 * 65                                         # at least a sign pair per bin of the half spectrum


def test_null_pointers_short_workspace_and_unsupported_shapes_answer_with_the_library_s_codes():
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    p = (base + 255) & ~255                                          # an aligned, non-null address; nothing is launched with it
    big = lib.wm_fft_l1_workspace_bytes(1, 16, 16)
    fwd, bwd = lib.wm_fft_l1_mean_fwd, lib.wm_fft_l1_mean_bwd
    assert fwd(None, p, p, None, p, big, 1, 16, 16, None) == _lib.WM_ENULL
    assert fwd(p, None, p, None, p, big, 1, 16, 16, None) == _lib.WM_ENULL
    assert fwd(p, p, None, None, p, big, 1, 16, 16, None) == _lib.WM_ENULL
    assert fwd(p, p, p, None, None, big, 1, 16, 16, None) == _lib.WM_ENULL
    assert fwd(p, p, p, None, p, big - 1, 1, 16, 16, None) == _lib.WM_EWORKSPACE
    assert fwd(p + 4, p, p, None, p, big, 1, 16, 16, None) == _lib.WM_EALIGN
    assert bwd(None, p, p, None, p, big, 1, 16, 16, None) == _lib.WM_ENULL
    assert bwd(p, None, p, None, p, big, 1, 16, 16, None) == _lib.WM_ENULL
    assert bwd(p, p, None, None, p, big, 1, 16, 16, None) == _lib.WM_ENULL          # neither gradient wanted
    assert bwd(p, p, p, None, None, big, 1, 16, 16, None) == _lib.WM_ENULL
    assert bwd(p, p, p, None, p, big - 1, 1, 16, 16, None) == _lib.WM_EWORKSPACE
    for h, w in ((24, 16), (16, 8), (2048, 16), (16, 0), (-1, 16)):
        assert fwd(p, p, p, None, p, 1 << 30, 1, h, w, None) == _lib.WM_EUNSUPPORTED
        assert bwd(p, p, p, None, p, 1 << 30, 1, h, w, None) == _lib.WM_EUNSUPPORTED
    assert fwd(p, p, p, None, p, 1 << 30, 1 << 40, 16, 16, None) == _lib.WM_EUNSUPPORTED
    assert fwd(p, p, p, None, p, 1 << 30, 0, 16, 16, None) == _lib.WM_EINVAL
    for name in ("wm_fft_l1_supported", "wm_fft_l1_record_bytes", "wm_fft_l1_workspace_bytes", "wm_fft_l1_mean_fwd", "wm_fft_l1_mean_bwd"):
        assert name in _lib.SIGNATURES


# ---- the switch ---------------------------------------------------------------------------------------------------------------------------
def test_switch_defaults_to_torch_and_returns_the_previous_backend():
    assert wm.fft_loss_backend() == "torch" or os.environ.get("WM_FFT_LOSS") == "hip"
    first = wm.fft_loss_backend()
    try:
        assert wm.set_fft_loss("hip") == first and wm.fft_loss_backend() == "hip"
        assert wm.set_fft_loss("torch") == "hip" and wm.fft_loss_backend() == "torch"
        assert wm.ops.set_fft_loss is wm.set_fft_loss and wm.ops.fft_loss_backend is wm.fft_loss_backend
        with pytest.raises(ValueError, match="set_fft_loss"):
            wm.set_fft_loss("rocfft")
        assert wm.fft_loss_backend() == "torch"
    finally:
        wm.set_fft_loss(first)


def test_environment_sets_the_initial_backend_in_a_fresh_process():
    def run(value):
        env = {k: v for k, v in os.environ.items() if k != "WM_FFT_LOSS"}
        if value is not None:
            env["WM_FFT_LOSS"] = value
        return subprocess.run([sys.executable, "-c", "import wave_mamba_amd as wm; print(wm.fft_loss_backend())"], cwd=ROOT, env=env,
                              capture_output=True, text=True, timeout=300)
    assert run(None).stdout.strip() == "torch"
    assert run("hip").stdout.strip() == "hip"
    bad = run("rocfft")
    assert bad.returncode != 0 and "WM_FFT_LOSS" in bad.stderr


def test_cpu_tensors_take_the_default_path_whatever_the_backend():
    pred, target = fc.randn_pair((2, 3, 32, 32), 2)

    def both(fn):
        p = pred.clone().requires_grad_(True)
        v = fn(p)
        v = v if isinstance(v, torch.Tensor) else v[1]
        g, = torch.autograd.grad(v, p)
        return v.detach(), g
    v0, g0 = both(lambda p: trainer.fft_l1(p, target))
    v1, g1 = both(lambda p: trainer.fft_l1(p, target, backend="hip"))
    assert torch.equal(v0, v1) and torch.equal(g0, g1)
    assert torch.equal(v0, fc.reference(pred, target))
    l0, l1 = trainer.losses(pred, target), trainer.losses(pred, target, fft_backend="hip")
    assert len(l0) == len(l1) == 2 and all(torch.equal(a, b) for a, b in zip(l0, l1))
    l3 = trainer.losses(pred, target, ssim_weight=0.25, fft_backend="hip")
    assert all(torch.equal(a, b) for a, b in zip(trainer.losses(pred, target, ssim_weight=0.25), l3))
    prev = wm.set_fft_loss("hip")
    try:
        v2, g2 = both(lambda p: trainer.fft_l1(p, target))
    finally:
        wm.set_fft_loss(prev)
    assert torch.equal(v0, v2) and torch.equal(g0, g2)
    with pytest.raises(ValueError, match="backend"):
        trainer.fft_l1(pred, target, backend="rocfft")


def test_recipe_key():
    opt, _ = recipe.load_options(YAML)
    assert "backend" not in opt["train"]["fft_opt"] and recipe.fft_backend_option(opt) is None
    for value in ("hip", "torch"):
        opt["train"]["fft_opt"]["backend"] = value
        got, _ = recipe.load_options(yaml.safe_dump(opt) + "\n")
        assert recipe.fft_backend_option(got) == value
    opt["train"]["fft_opt"]["backend"] = "rocfft"
    with pytest.raises(ValueError, match="train.fft_opt.backend"):
        recipe.load_options(yaml.safe_dump(opt) + "\n")


# ---- torch.library ops under the CPU key ------------------------------------------------------------------------------------------------
def test_torch_library_ops_on_cpu_tensors_are_the_twin():
    import wave_mamba_amd.torch_ops as tops
    assert "fft_l1_mean" in tops.OPS and "fft_l1_mean_backward" in tops.OPS
    pred, target = fc.flat_pair(1, 2, 32, 64, seed=fc.FLAT_SEED)
    p, t = pred.clone().requires_grad_(True), target.clone().requires_grad_(True)
    v = torch.ops.wavemamba_hip.fft_l1_mean(p, t)
    assert v.dtype == torch.float32 and v.dim() == 0
    (3.0 * v).backward()
    p2, t2 = pred.clone().requires_grad_(True), target.clone().requires_grad_(True)
    w = cpu_twin.fft_l1_mean(p2, t2)
    (3.0 * w).backward()
    assert torch.equal(v.detach(), w.detach()) and torch.equal(p.grad, p2.grad) and torch.equal(t.grad, t2.grad)
    p3 = pred.clone().requires_grad_(True)
    torch.ops.wavemamba_hip.fft_l1_mean(p3, target).backward()                  # one side only
    assert p3.grad.shape == pred.shape


def test_fake_implementations_give_shapes_and_dtypes():
    import wave_mamba_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        a, b = torch.empty(2, 3, 64, 64), torch.empty(2, 3, 64, 64, dtype=torch.bfloat16)
        v = torch.ops.wavemamba_hip.fft_l1_mean(a, b)
        assert v.shape == () and v.dtype == torch.float32
        g = torch.empty((), dtype=torch.float32)
        ga, gb = torch.ops.wavemamba_hip.fft_l1_mean_backward(a, b, g, True, True)
        assert ga.shape == a.shape and gb.shape == b.shape and ga.dtype == gb.dtype == torch.float32
        ga, gb = torch.ops.wavemamba_hip.fft_l1_mean_backward(a, b, g, True, False)
        assert ga.shape == a.shape and gb.shape == (0,)
        with pytest.raises(RuntimeError, match="fft_l1_mean"):
            torch.ops.wavemamba_hip.fft_l1_mean(a, b[:, :1])
