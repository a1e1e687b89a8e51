"""CPU: the arch file's grad rule under PARTIAL freezing.  A forward-only operator writes into fresh memory and its result carries
no graph, so a call site that takes one while something flowing into it wants a gradient drops that gradient silently: the
forward stays right and nothing raises.  An HFEBlock in float64 runs here under a stand-in backend that has the four operators
CMTAttention's fold goes through - `gram`, `attn_fold` and `conv2d` forward-only (torch code under no_grad, the way a launch into
torch.empty behaves), `gram_train` under autograd - and under the empty backend (the plain PyTorch path): outputs and gradients
must agree, and no gradient the plain path has may be missing.  (The real HIP operators: tests/test_partial_grad_gpu.py.)"""
import pytest
import torch
import torch.nn.functional as F

from oracle import backend as oracle_backend
from wave_mamba_amd.archs import wavemamba_arch as arch

BAR = 1e-12         # both sides are float64 and differ only in association


class StandIn:
    """`gram`, `gram_train`, `attn_fold`, `conv2d` with wave_mamba_amd.ops's signatures, as torch code on any device and dtype."""

    @staticmethod
    def gram_supported(x, y):
        return x.shape == y.shape

    @staticmethod
    def gram_train(x, y):
        return x @ y.transpose(1, 2), (x * x).sum(2), (y * y).sum(2)

    @staticmethod
    @torch.no_grad()
    def gram(x, y):
        return StandIn.gram_train(x, y)

    @staticmethod
    def attn_fold_supported(x, w_po, heads):
        return x.shape[1] % heads == 0

    @staticmethod
    @torch.no_grad()
    def attn_fold(G, nq, nk, temperature, w_po, batch, heads):
        C = w_po.shape[0]
        scale = nq.clamp_min(1e-24).sqrt().unsqueeze(2) * nk.clamp_min(1e-24).sqrt().unsqueeze(1)
        attn = (G / scale).reshape(batch, heads, C // heads, C // heads)
        attn = (attn * temperature.reshape(1, heads, 1, 1)).softmax(dim=-1)
        return w_po.reshape(C, C) @ torch.stack([torch.block_diag(*a) for a in attn], 0)

    @staticmethod
    def conv2d_supported(x, weight, x2=None):
        return True

    @staticmethod
    @torch.no_grad()
    def conv2d(x, weight, bias=None, x2=None, x2_index=None, gate=None, residual=None, dynamic_weight=False):
        if x2 is not None and x2_index is not None:
            x2 = torch.gather(x2, 1, x2_index.long()[:, :, None, None].expand(-1, -1, x2.shape[2], x2.shape[3]))
        if x2 is not None:
            x = torch.cat([x, x2], 1)
        y = F.conv2d(x, weight, bias, padding=weight.shape[2] // 2)
        if gate is not None:
            y = y * torch.sigmoid(gate)
        return y if residual is None else y + residual


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


CASES = {                                               # name -> (is this parameter trainable?, do the inputs want gradients?)
    "all_frozen_input_grad": (lambda n: False, True),
    "attn_frozen": (lambda n: not n.startswith("attn."), True),
    "attn_frozen_inputs_plain": (lambda n: not n.startswith("attn."), False),
    "attn_alone_trainable": (lambda n: n.startswith("attn."), True),
    "attn_alone_trainable_inputs_plain": (lambda n: n.startswith("attn."), False),
}


def run(blk, x, per, backend):
    """One forward and backward -> (y, {name: gradient or None}) with 'x' and 'perception' among the names."""
    leaves = dict(blk.named_parameters(), x=x, perception=per)
    for t in leaves.values():
        t.grad = None
    with oracle_backend.ops_backend(backend):
        y = blk(x, per)
        assert y.requires_grad, "the block's output carries no graph"
        (y * torch.linspace(0.5, 1.5, y.numel(), dtype=y.dtype).view_as(y)).sum().backward()
    return y.detach(), {k: None if t.grad is None else t.grad.clone() for k, t in leaves.items()}


@pytest.mark.parametrize("case", list(CASES))
def test_hfe_block_gradients_survive_partial_freezing(case):
    trainable, input_grad = CASES[case]
    torch.manual_seed(7)
    blk = arch.HFEBlock(32, match_factor=1, ffn_expansion_factor=1).double()
    with torch.no_grad():                               # off the initial ones / zeros, so that every gradient is a general one
        for n, p in blk.named_parameters():
            if p.dim() <= 1 or n.endswith("temperature"):
                p.add_(0.3 * torch.randn_like(p))
    for n, p in blk.named_parameters():
        p.requires_grad_(trainable(n))
    g = torch.Generator().manual_seed(11)
    x = torch.randn(1, 32, 12, 20, generator=g, dtype=torch.float64).requires_grad_(input_grad)
    per = torch.randn(1, 32, 12, 20, generator=g, dtype=torch.float64).requires_grad_(input_grad)
    y_want, want = run(blk, x, per, type("Plain", (), {})())
    y_got, got = run(blk, x, per, StandIn())
    assert rel(y_got, y_want) <= BAR, f"{case}: forward differs by {rel(y_got, y_want):.3e}"
    assert any(v is not None for v in want.values())
    missing = [k for k, v in want.items() if v is not None and got[k] is None]
    assert not missing, f"{case}: no gradient reached {missing} (the plain path gives them one)"
    for k, v in want.items():
        if v is None:
            assert got[k] is None, f"{case}: {k} is frozen and got a gradient"
        else:
            assert rel(got[k], v) <= BAR, f"{case}: gradient of {k} off by {rel(got[k], v):.3e} (|g| max {float(v.abs().max()):.3e})"
