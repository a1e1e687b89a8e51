"""The arch file's dispatch, characterised: which operator of wave_mamba_amd.ops each module of a small WaveMamba calls, in
call order, against the lists recorded on the commit named in tests/golden/arch_dispatch.json (make_golden_dispatch.py); and
the two textual facts that keep the dispatch in one place (one lookup helper, one grad rule)."""
import ast
import importlib.util
import json
import os

import pytest
import torch

from conftest import GOLDEN, ROOT, assert_close
from oracle import backend as oracle_backend
import wave_mamba_amd as wm
from wave_mamba_amd.archs import wavemamba_arch as arch

DEV = "cuda:0"
TOL = 1e-4          # the per-tensor gradient bar (TOL of tests/test_gpu_parity.py)


def _recorder_module():
    spec = importlib.util.spec_from_file_location("make_golden_dispatch", os.path.join(GOLDEN, "make_golden_dispatch.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["eval_two_streams", "eval_one_stream", "train", "frozen_input_grad"])
def test_dispatch_matches_recorded_lists(mode):
    """The ordered operator calls of one forward (+ backward) equal the recorded ones: a rewrite of the dispatch conditions
    sends every module of this model where it went before."""
    gd = _recorder_module()
    with open(os.path.join(GOLDEN, "arch_dispatch.json")) as f:
        want = json.load(f)[mode]
    rec = gd.Recorder(wm.ops)
    with oracle_backend.ops_backend(rec):
        gd.run_mode(mode)
    diff = next((i for i, (a, b) in enumerate(zip(rec.calls, want)) if a != b), min(len(rec.calls), len(want)))
    assert rec.calls == want, (f"{mode}: {len(rec.calls)} calls against {len(want)} recorded; first difference at call {diff}: "
                               f"{rec.calls[diff:diff + 3]} against {want[diff:diff + 3]}")


@pytest.mark.gpu
def test_paconv_gate_bias_alone_trainable_gets_its_gradient():
    """An HFEBlock whose only trainable parameter is the bias of PAConv's gate convolution (k2), inputs without grad: the
    block must record a graph through the gate (the forward-only conv2d_gated kernel cannot serve it), and the bias's
    gradient on the HIP backend matches the plain PyTorch path's.
    (On 4cb310b PAConv's own grad test listed x, x2, k3.weight and k2.weight but not k2.bias: the block took conv2d_gated,
    its output carried no graph and backward() raised "element 0 of tensors does not require grad and does not have a grad_fn".)"""
    torch.manual_seed(3)
    blk = arch.HFEBlock(32, match_factor=1, ffn_expansion_factor=1).to(DEV)
    x = torch.randn(1, 32, 40, 56, device=DEV)
    per = torch.randn(1, 32, 40, 56, device=DEV)
    for p in blk.parameters():
        p.requires_grad_(False)
    bias = blk.ffn.matching_transformation.paconv.k2.bias.requires_grad_(True)
    blk(x, per).sum().backward()
    got, bias.grad = bias.grad, None
    with oracle_backend.ops_backend(type("Plain", (), {})()):                 # a backend without any helper
        blk(x, per).sum().backward()
    print(f"k2.bias gradient: |g| max {float(bias.grad.abs().max()):.3e}, HIP vs plain rel max "
          f"{float((got - bias.grad).abs().max() / bias.grad.abs().max()):.3e}")
    assert_close(got, bias.grad, TOL, "PAConv k2.bias gradient")


def test_one_lookup_helper_and_one_grad_rule():
    """Two facts about wavemamba_arch.py's syntax tree: `hasattr` is called nowhere outside the lookup helper `_op`, and
    `requires_grad` / `is_grad_enabled` are named only inside `_needs_grad`."""
    path = os.path.join(ROOT, "wave_mamba_amd", "archs", "wavemamba_arch.py")
    with open(path) as f:
        tree = ast.parse(f.read())
    found = {"hasattr": set(), "grad": set()}

    def walk(node, owner):
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and owner is None:
            owner = node.name                                              # the top-level function or class a node lies in
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "hasattr":
            found["hasattr"].add(owner)
        if isinstance(node, ast.Attribute) and node.attr in ("requires_grad", "is_grad_enabled"):
            found["grad"].add(owner)
        for child in ast.iter_child_nodes(node):
            walk(child, owner)
    walk(tree, None)
    assert found["hasattr"] <= {"_op"}, f"hasattr() called in {sorted(map(str, found['hasattr']))}"
    assert found["grad"] == {"_needs_grad"}, f"grad mode / requires_grad asked in {sorted(map(str, found['grad']))}"
