"""CPU: the deterministic training mode's host surface - the switch itself, and ops.channel_gather on CPU tensors, which is plain
torch.gather (ordered there already) bit for bit, forward and backward."""
import os
import subprocess
import sys

import torch

from conftest import ROOT
import wave_mamba_amd as wm


def test_set_deterministic_returns_the_previous_value_and_round_trips():
    assert wm.set_deterministic is wm.ops.set_deterministic and wm.is_deterministic is wm.ops.is_deterministic
    first = wm.is_deterministic()
    assert isinstance(first, bool)
    try:
        assert wm.set_deterministic(True) is first and wm.is_deterministic() is True
        assert wm.set_deterministic(False) is True and wm.is_deterministic() is False
        assert wm.set_deterministic(1) is False and wm.is_deterministic() is True          # any truth value, stored as a bool
    finally:
        wm.set_deterministic(first)
    assert wm.is_deterministic() is first


def test_the_initial_mode_comes_from_the_environment():
    """WM_DETERMINISTIC is read at import, like WM_TRAIN_CONV: 1 switches the mode on in a fresh interpreter, absent or 0 leaves it
    off, anything else is refused."""
    def run(value):
        env = {k: v for k, v in os.environ.items() if k != "WM_DETERMINISTIC"}
        if value is not None:
            env["WM_DETERMINISTIC"] = value
        return subprocess.run([sys.executable, "-c", "import wave_mamba_amd as wm; print(wm.is_deterministic())"], cwd=ROOT, env=env,
                              capture_output=True, text=True)
    assert run("1").stdout.strip() == "True"
    assert run("0").stdout.strip() == "False"
    assert run(None).stdout.strip() == "False"
    bad = run("yes")
    assert bad.returncode != 0 and "WM_DETERMINISTIC" in bad.stderr


def _cases():
    g = torch.Generator().manual_seed(4)
    # (B, C, H, W) maps as _cat_gathered sees them and (B, C, HW) maps as nearest_candidate_maps does; indices with repeated
    # destinations and destinations that receive nothing; int32 (match_index) and int64 (topk) indices
    yield torch.randn(3, 8, 5, 7, generator=g), torch.tensor([[0, 0, 3, 7, 3, 0], [1, 2, 3, 4, 5, 6], [7, 7, 7, 7, 7, 7]])
    yield torch.randn(2, 6, 35, generator=g), torch.tensor([[5, 5, 0, 1], [2, 2, 2, 3]], dtype=torch.int32)
    yield torch.randn(1, 4, 9, generator=g), torch.zeros(1, 0, dtype=torch.int64)


def test_channel_gather_on_cpu_tensors_is_torch_gather_bit_for_bit():
    for mode in (False, True):                                   # CPU tensors take torch.gather whatever the mode is
        prev = wm.set_deterministic(mode)
        try:
            for x, idx in _cases():
                full = idx.long().reshape(idx.shape + (1,) * (x.dim() - 2)).expand(-1, -1, *x.shape[2:])
                xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
                got, want = wm.ops.channel_gather(xa, idx), torch.gather(xb, 1, full)
                assert got.shape == want.shape and torch.equal(got, want)
                gy = torch.randn(want.shape, generator=torch.Generator().manual_seed(1))
                got.backward(gy); want.backward(gy)
                assert torch.equal(xa.grad, xb.grad)
        finally:
            wm.set_deterministic(prev)


def test_the_arch_gathers_are_unchanged_on_the_cpu():
    """_cat_gathered / nearest_candidate_maps with the mode on and CPU tensors: the same tensors as with it off."""
    from wave_mamba_amd.archs import wavemamba_arch as arch
    g = torch.Generator().manual_seed(9)
    x, x2 = torch.randn(2, 8, 6, 5, generator=g), torch.randn(2, 8, 6, 5, generator=g)
    idx = torch.randint(0, 8, (2, 8), generator=g)
    off = arch._cat_gathered(x, x2, idx)
    prev = wm.set_deterministic(True)
    try:
        on = arch._cat_gathered(x, x2, idx)
    finally:
        wm.set_deterministic(prev)
    assert torch.equal(on, off)
