"""GPU: gradients when only PART of the network is trainable.  The arch file chooses per call site between a forward-only HIP
kernel (its result is fresh memory without a graph) and an autograd path; a site that asks too little of `_needs_grad` drops a
gradient silently - the forward stays right and nothing raises.  Three parts:

  A  a graph-drop detector around wave_mamba_amd.ops (no list of forward-only operators: an operator call whose arguments want a
     gradient and whose floating-point results carry none IS a drop; a site that means to cut the graph detaches first), run over
     freeze patterns of HFEBlock, an LFSSBlock stack, SKFF and a small WaveMamba, with the shipped size floors and with the
     `_FUSE_*_MIN_POSITIONS` floors at 0 (the fused forward-only forms become candidates on small maps);
  B  HFEBlock gradient VALUES under freeze patterns against the same block in float64 on the CPU, judged by the suite's criterion
     (truth_bar of tests/test_gpu_parity.py) against the plain fp32 PyTorch path's own error;
  C  the wf = 8 model under freeze patterns against the goldens it already has (a parameter's gradient does not depend on which other
     parameters are marked trainable), and the input gradient against tests/golden/train_grads_wf8_input.npz.

The CPU twin of the rule: tests/test_partial_grad_cpu.py."""
import contextlib
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, assert_close, rel_err
from oracle import backend as oracle_backend
from test_arch_cpu import grad_golden_case
from test_gpu_parity import truth_bar
import wave_mamba_amd as wm
from wave_mamba_amd import ops
from wave_mamba_amd.archs import wavemamba_arch as arch

gpu = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 32, 8, 32), (2, 32, 9, 21)]
FLOORS = ["shipped_floors", "floors_at_0"]


# ------------------------------------------------------------------------------------------------
# A: the detector
# ------------------------------------------------------------------------------------------------
class GraphDropped(AssertionError):
    pass


def tensors_of(v):
    """The tensors an argument or a result stands for: itself, the tensors inside a tuple or list, the parameters of a module
    (lfss_block_forward takes the block)."""
    if isinstance(v, torch.Tensor):
        yield v
    elif isinstance(v, (tuple, list)):
        for e in v:
            yield from tensors_of(e)
    elif isinstance(v, torch.nn.Module):
        yield from v.parameters()


class Detector:
    """An operator set with every call checked: attribute lookups go to `ops`, the `_supported` predicates come back as they are,
    any other callable wrapped.  The wrapped call fails when grad mode is on, some argument requires grad and no floating-point
    tensor it returns does."""

    def __init__(self, ops):
        self._ops, self.calls = ops, []

    def __getattr__(self, name):
        v = getattr(self._ops, name)
        if not callable(v) or name.endswith("_supported"):
            return v

        def checked(*args, **kwargs):
            out = v(*args, **kwargs)
            self.calls.append(name)
            if torch.is_grad_enabled():
                wants = [i for i, a in [*enumerate(args), *kwargs.items()] if any(t.requires_grad for t in tensors_of(a))]
                if wants and not any(t.requires_grad for t in tensors_of(out) if t.is_floating_point()):
                    raise GraphDropped(f"operator {name} dropped the graph of argument {wants[0]}")
            return out
        return checked


def test_detector_on_a_stand_in_operator_set():
    """The detector itself, on the CPU: it names the operator and the argument, looks inside lists and modules, leaves predicates
    and no_grad calls alone, and lets a call through whose argument was detached by the caller."""
    class Fake:
        keep = staticmethod(lambda a, b=None: a * 2)
        drop = staticmethod(lambda a, b=None, residual=None: a.detach() * 2)
        drop_of_list = staticmethod(lambda feats: feats[0].detach() + feats[1].detach())
        index = staticmethod(lambda a: a.argmax(1))
        pair = staticmethod(lambda a: (a.detach(), a + 1))
        of_block = staticmethod(lambda a, blk: a.detach() + blk.weight.detach().sum())
        drop_supported = staticmethod(lambda a: a.detach())
        flag = True
    det = Detector(Fake)
    x, plain = torch.ones(2, 3, requires_grad=True), torch.ones(2, 3)
    lin = torch.nn.Linear(3, 3)
    assert det.keep(x).requires_grad and det.pair(x)[1].requires_grad and det.flag is True
    assert not det.drop(plain).requires_grad and not det.drop(x.detach()).requires_grad and not det.drop_supported(x).requires_grad
    det.index(x.detach())
    with torch.no_grad():
        det.drop(x)
    for call, message in [(lambda: det.drop(x), "operator drop dropped the graph of argument 0"),
                          (lambda: det.drop(plain, x), "operator drop dropped the graph of argument 1"),
                          (lambda: det.drop(plain, residual=x), "operator drop dropped the graph of argument residual"),
                          (lambda: det.drop_of_list([plain, x]), "operator drop_of_list dropped the graph of argument 0"),
                          (lambda: det.index(x), "operator index dropped the graph of argument 0"),
                          (lambda: det.of_block(plain, lin), "operator of_block dropped the graph of argument 1")]:
        with pytest.raises(GraphDropped, match=message + "$"):
            call()
    assert det.calls.count("drop") == 6 and "drop_supported" not in det.calls


def lower_the_floors(monkeypatch):
    """Every `_FUSE_*_MIN_POSITIONS` floor of ops.py to 0 (tests/test_hfe_heads.py's form); the `_supported` predicates stay."""
    names = [n for n in vars(ops) if n.startswith("_FUSE_") and n.endswith("_MIN_POSITIONS")]
    assert len(names) >= 6, names
    for n in names:
        v = getattr(ops, n)
        monkeypatch.setattr(ops, n, {k: 0 for k in v} if isinstance(v, dict) else 0)


def prefixes(mod, depth=1):
    """The names of `mod`'s sub-modules down to `depth` levels that hold parameters."""
    return [n for n, m in mod.named_modules() if n and n.count(".") < depth and any(True for _ in m.parameters())]


def under(prefix, name):
    return name == prefix or name.startswith(prefix + ".")


def block_patterns(mod, depth=1):
    """-> [(label, trainable parameter names, do the inputs require grad)]: everything frozen and the inputs wanting gradients; each
    sub-module alone frozen and alone trainable (both ways with and without input gradients); each single parameter alone
    trainable, inputs plain."""
    names = [n for n, _ in mod.named_parameters()]
    out = [("all frozen, inputs want gradients", set(), True)]
    for pre in prefixes(mod, depth):
        inside = {n for n in names if under(pre, n)}
        for ig in (False, True):
            out.append((f"{pre} alone frozen, inputs {'want gradients' if ig else 'plain'}", set(names) - inside, ig))
            out.append((f"{pre} alone trainable, inputs {'want gradients' if ig else 'plain'}", inside, ig))
    out += [(f"{n} alone trainable, inputs plain", {n}, False) for n in names]
    return out


def run_patterns(mod, call, inputs, patterns):
    """Forward and backward of `call(*inputs)` under the detector for every pattern (its input flag: one for all inputs, or one per
    input) -> the list of failures: a dropped graph, an output without a graph, a trainable leaf without a gradient, a frozen one
    with a gradient."""
    failures = []
    params = dict(mod.named_parameters())
    for label, trainable, input_grad in patterns:
        for n, p in params.items():
            p.requires_grad_(n in trainable)
            p.grad = None
        flags = input_grad if isinstance(input_grad, tuple) else (input_grad,) * len(inputs)
        ins = [t.detach().clone().requires_grad_(f) for t, f in zip(inputs, flags)]
        det = Detector(wm.ops)
        try:
            with oracle_backend.ops_backend(det):
                y = call(*ins)
                if not y.requires_grad:
                    raise GraphDropped("the output carries no graph")
                y.sum().backward()
        except GraphDropped as e:
            failures.append(f"{label}: {e}")
            continue
        leaves = {**{n: (p, n in trainable) for n, p in params.items()},
                  **{f"input {i}": (t, t.requires_grad) for i, t in enumerate(ins)}}
        lost = [n for n, (t, want) in leaves.items() if want and t.grad is None]
        extra = [n for n, (t, want) in leaves.items() if not want and t.grad is not None]
        if lost or extra:
            failures.append(f"{label}: no gradient reached {lost}; frozen but given a gradient: {extra}")
    torch.cuda.synchronize()
    return failures


def report(what, patterns, failures):
    print(f"{what}: {len(patterns)} freeze patterns, {len(failures)} failures")
    assert not failures, f"{what}: {len(failures)} of {len(patterns)} freeze patterns fail:\n  " + "\n  ".join(failures[:12])


def maps(shape, n, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(shape, generator=g).to(DEV) for _ in range(n)]


@gpu
@pytest.mark.parametrize("floors", FLOORS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_no_operator_drops_a_graph_hfe_block(monkeypatch, shape, floors):
    torch.manual_seed(1)
    blk = arch.HFEBlock(32, match_factor=1, ffn_expansion_factor=1).to(DEV)
    if floors == "floors_at_0":
        lower_the_floors(monkeypatch)
    patterns = block_patterns(blk) + [("all frozen, perception alone wants a gradient", set(), (False, True))]
    failures = run_patterns(blk, blk, maps(shape, 2, 21), patterns)
    report(f"HFEBlock {shape} {floors}", patterns, failures)


@gpu
@pytest.mark.parametrize("floors", FLOORS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_no_operator_drops_a_graph_lfss_stack(monkeypatch, shape, floors):
    """Two blocks, so that a stack with one frozen and one trainable block occurs (the sub-modules down to two levels: the blocks
    and each block's own)."""
    torch.manual_seed(2)
    stack = torch.nn.Sequential(arch.LFSSBlock(32), arch.LFSSBlock(32)).to(DEV)
    if floors == "floors_at_0":
        lower_the_floors(monkeypatch)
    patterns = block_patterns(stack, depth=2)
    failures = run_patterns(stack, lambda x: arch._run_lfss_stack(stack, x), maps(shape, 1, 22), patterns)
    report(f"LFSSBlock stack {shape} {floors}", patterns, failures)


@gpu
@pytest.mark.parametrize("floors", FLOORS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_no_operator_drops_a_graph_skff(monkeypatch, shape, floors):
    torch.manual_seed(3)
    skff = arch.SKFF(32).to(DEV)
    if floors == "floors_at_0":
        lower_the_floors(monkeypatch)
    patterns = block_patterns(skff)
    failures = run_patterns(skff, lambda *feats: skff(list(feats)), maps(shape, 3, 23), patterns)
    report(f"SKFF {shape} {floors}", patterns, failures)


# ------------------------------------------------------------------------------------------------
# the model's freeze patterns (parts A and C)
# ------------------------------------------------------------------------------------------------
def of_type(net, *types):
    """The parameter names inside every sub-module of one of `types`."""
    return {f"{n}.{k}" for n, m in net.named_modules() if isinstance(m, types) for k, _ in m.named_parameters()}


def having(net, *parts):
    """The parameter names with a path component that starts with one of `parts`."""
    return {n for n, _ in net.named_parameters() if any(c.startswith(parts) for c in n.split("."))}


def model_pattern(net, pattern):
    """-> (the trainable parameter names, does the input want a gradient)."""
    names = {n for n, _ in net.named_parameters()}
    attn = of_type(net, arch.CMTAttention)
    norms = of_type(net, arch.LayerNorm2d, torch.nn.LayerNorm)
    trainable = {
        "attention_frozen": names - attn,
        "attention_alone_trainable": attn,
        "hfe_side_frozen": names - having(net, "h_blk", "h_fusion", "h_out_conv"),
        "lfss_side_frozen": names - having(net, "l_blk", "l_conv"),
        "encoder_frozen": names - having(net, "ps_down", "conv_01", "down_group"),
        "decoder_frozen": names - having(net, "up_group", "last"),
        "norms_alone_trainable": norms,
        "one_d_alone_trainable": {n for n, p in net.named_parameters() if p.dim() == 1},
        "all_frozen_input_grad": set(),
    }[pattern]
    assert pattern == "all_frozen_input_grad" or (trainable and trainable < names), pattern
    return trainable, pattern == "all_frozen_input_grad"


MODEL_PATTERNS = ["attention_frozen", "attention_alone_trainable", "hfe_side_frozen", "lfss_side_frozen", "encoder_frozen",
                  "decoder_frozen", "norms_alone_trainable", "one_d_alone_trainable", "all_frozen_input_grad"]


@gpu
@pytest.mark.parametrize("floors", FLOORS)
def test_no_operator_drops_a_graph_model(monkeypatch, floors):
    torch.manual_seed(0)
    net = wm.WaveMamba(in_chn=3, wf=8, n_l_blocks=[1, 1, 2], n_h_blocks=[1, 1, 1], ffn_scale=2.0).train().to(DEV)
    if floors == "floors_at_0":
        lower_the_floors(monkeypatch)
    patterns = [(p, *model_pattern(net, p)) for p in MODEL_PATTERNS]
    lq = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1234)).to(DEV)
    failures = run_patterns(net, net, [lq], patterns)
    report(f"WaveMamba wf = 8 {floors}", patterns, failures)


# ------------------------------------------------------------------------------------------------
# B: HFEBlock gradient values against float64
# ------------------------------------------------------------------------------------------------
HFE_CASES = {(1, 32, 8, 32): 4, (2, 32, 9, 21): 5}      # shape -> the seed of block and inputs (see hfe_reference: the argmin gap)
MIN_GAP = 5e-4                                          # hundreds of times the fp32 Gram form's ~1e-6 relative error in d^2


@contextlib.contextmanager
def matching_spy(log):
    """Every channel matching of the block noted: (maps, candidates, the indices chosen), in call order."""
    real = arch.nearest_candidate_index

    def spy(maps, candidates, num_matches):
        idx = real(maps, candidates, num_matches)
        log.append((maps.detach(), candidates.detach(), idx.detach().cpu().long()))
        return idx
    arch.nearest_candidate_index = spy
    try:
        yield
    finally:
        arch.nearest_candidate_index = real


def hfe_case(shape):
    seed = HFE_CASES[shape]
    torch.manual_seed(seed)
    blk = arch.HFEBlock(32, match_factor=1, ffn_expansion_factor=1)
    g = torch.Generator().manual_seed(seed)
    x, per = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    dy = torch.randn(shape, generator=g)                # the cotangent of the output
    return blk, x, per, dy


def hfe_grads(blk, x, per, dy, trainable, input_grad, backend):
    """One forward and backward of `blk` on `backend` (None: the HIP operators) -> ({name: gradient or None}, y, matching indices)."""
    for n, p in blk.named_parameters():
        p.requires_grad_(trainable(n))
        p.grad = None
    x, per = x.detach().clone().requires_grad_(input_grad), per.detach().clone().requires_grad_(input_grad)
    log = []
    with matching_spy(log), oracle_backend.ops_backend(backend):
        y = blk(x, per)
        (y * dy).sum().backward()
    grads = {n: p.grad for n, p in blk.named_parameters()}
    grads.update(x=x.grad, perception=per.grad)
    return grads, y.detach(), log


@functools.lru_cache(maxsize=None)
def hfe_reference(shape):
    """Once per shape, shared and left unchanged: the truth (the block as .double() on the CPU under the empty backend, everything
    trainable), the matching indices of that run, and e_ref per tensor - the error of the plain fp32 path (the same block on the GPU
    under the empty backend).  Channel matching is an argmin: on the float64 run the relative gap between the nearest and the
    second-nearest distance must be at least MIN_GAP for every channel at both matching sites, or the comparison means nothing."""
    blk, x, per, dy = hfe_case(shape)
    plain = type("Plain", (), {})()
    truth, y, log = hfe_grads(blk.double(), x.double(), per.double(), dy.double(), lambda n: True, True, plain)
    assert len(log) == 2
    for site, (m, c, _) in enumerate(log):
        near = torch.cdist(m, c).topk(2, largest=False).values
        gap = float(((near[..., 1] - near[..., 0]) / near[..., 0]).min())
        print(f"HFEBlock {shape}: matching site {site}: minimum relative gap nearest / second-nearest {gap:.2e}")
        assert gap >= MIN_GAP, f"matching site {site}: gap {gap:.2e} below {MIN_GAP:g}"
    blk32 = hfe_case(shape)[0].to(DEV)
    ref, y32, log32 = hfe_grads(blk32, x.to(DEV), per.to(DEV), dy.to(DEV), lambda n: True, True, plain)
    assert all(torch.equal(a[2], b[2]) for a, b in zip(log, log32)), "the plain fp32 path matches other channels than float64"
    e_ref = {k: max(rel_err(ref[k], truth[k])) for k in truth}
    e_ref["y"] = max(rel_err(y32, y))
    return truth, y, [entry[2] for entry in log], e_ref


HFE_PATTERNS = {
    "all_frozen": lambda n: False,
    "attn_frozen": lambda n: not under("attn", n),
    "attn_alone_trainable": lambda n: under("attn", n),
    "ffn_frozen": lambda n: not under("ffn", n),
    "norm1_alone_trainable": lambda n: under("norm1", n),
    "norm2_alone_trainable": lambda n: under("norm2", n),
    "LayerNorm_alone_trainable": lambda n: under("LayerNorm", n),
    "temperature_alone_trainable": lambda n: n == "attn.temperature",
}
# (pattern, do the inputs want gradients, deterministic mode): all frozen needs the input gradients; the first two patterns run
# in the deterministic mode (the channel_gather path) as well
HFE_RUNS = [(p, ig, False) for p in HFE_PATTERNS for ig in (True, False) if (p, ig) != ("all_frozen", False)] + \
           [("all_frozen", True, True), ("attn_frozen", True, True), ("attn_frozen", False, True)]


@gpu
@pytest.mark.parametrize("pattern,input_grad,deterministic", HFE_RUNS,
                         ids=[f"{p}-{'input_grad' if ig else 'inputs_plain'}{'-deterministic' if d else ''}" for p, ig, d in HFE_RUNS])
@pytest.mark.parametrize("shape", list(HFE_CASES), ids=str)
def test_hfe_block_gradient_values_under_partial_freezing(shape, pattern, input_grad, deterministic):
    """max(rel_err(got, truth)) <= truth_bar(e_ref) for every gradient the pattern asks for (x.grad and perception.grad among
    them), None for every frozen leaf, the same channels matched as in float64."""
    truth, y_truth, idx_truth, e_ref = hfe_reference(shape)
    blk, x, per, dy = hfe_case(shape)
    prev = ops.set_deterministic(deterministic)
    try:
        got, y, log = hfe_grads(blk.to(DEV), x.to(DEV), per.to(DEV), dy.to(DEV), HFE_PATTERNS[pattern], input_grad, None)
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(prev)
    assert [entry[2].tolist() for entry in log] == [i.tolist() for i in idx_truth], "the HIP path matches other channels than float64"
    tag = f"HFEBlock {shape} {pattern}, inputs {'want gradients' if input_grad else 'plain'}{', deterministic' if deterministic else ''}"
    e_y = max(rel_err(y, y_truth))
    print(f"{tag}: y e_got {e_y:.3e} e_ref {e_ref['y']:.3e}")
    bad = [] if e_y <= truth_bar(e_ref["y"]) else [("y", e_y, e_ref["y"])]
    worst = (0.0, 0.0, None)
    for k, t in truth.items():
        wanted = input_grad if k in ("x", "perception") else HFE_PATTERNS[pattern](k)
        if not wanted:
            assert got[k] is None, f"{k} is frozen and got a gradient"
            continue
        assert got[k] is not None, f"no gradient reached {k}"
        assert torch.isfinite(got[k]).all(), k
        e_got = max(rel_err(got[k], t))
        print(f"{tag}: {k} e_got {e_got:.3e} e_ref {e_ref[k]:.3e}")
        worst = max(worst, (e_got, e_ref[k], k))
        if e_got > truth_bar(e_ref[k]):
            bad.append((k, e_got, e_ref[k]))
    print("%s: worst gradient error vs float64 truth: e_got %.3e (e_ref %.3e) %s" % (tag, *worst))
    assert not bad, "off the float64 truth (name, build, plain fp32 path): " + "; ".join("%s %.3e %.3e" % b for b in bad)


# ------------------------------------------------------------------------------------------------
# C: the model against the goldens it already has
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_truth():
    """{name: (float64 truth, the reference's fp32 gradient)} with 'lq' for the input (make_golden_grads.py, make_golden_input_grad.py)."""
    g = np.load(os.path.join(GOLDEN, "train_grads_wf8.npz"))
    t = np.load(os.path.join(GOLDEN, "train_grads_wf8_f64.npz"))
    i = np.load(os.path.join(GOLDEN, "train_grads_wf8_input.npz"))
    out = {k[2:]: (torch.from_numpy(t[k]), torch.from_numpy(g["g." + k[2:]]).double()) for k in t.files if k.startswith("t.")}
    out["lq"] = (torch.from_numpy(i["t.lq"]), torch.from_numpy(i["g.lq"]).double())
    return out


@gpu
@pytest.mark.parametrize("pattern", MODEL_PATTERNS)
def test_model_gradients_under_partial_freezing(pattern):
    """The step of test_training_step_per_parameter_gradients_on_gpu with part of the model frozen: every trainable parameter's
    gradient present, finite and within truth_bar of the float64 truth, every frozen parameter's None, the prediction unchanged."""
    net, g = grad_golden_case()
    truth = model_truth()
    net = net.to(DEV)
    trainable, input_grad = model_pattern(net, pattern)
    for n, p in net.named_parameters():
        p.requires_grad_(n in trainable)
    lq = torch.from_numpy(g["lq"]).to(DEV).requires_grad_(input_grad)
    pred = net(lq)
    l_pix, l_fft = wm.trainer.losses(pred, torch.from_numpy(g["gt"]).to(DEV))
    (l_pix + l_fft).backward()
    torch.cuda.synchronize()
    assert abs(float(l_pix.detach()) - g["losses"][0]) < 1e-6
    assert_close(pred.detach(), torch.from_numpy(g["pred"]), 1e-5, "prediction")
    leaves = dict(net.named_parameters(), lq=lq)
    assert set(leaves) == set(truth)
    bad, worst = [], (0.0, 0.0, None)
    for k, p in leaves.items():
        if not (input_grad if k == "lq" else k in trainable):
            assert p.grad is None, f"{k} is frozen and got a gradient"
            continue
        assert p.grad is not None, f"no gradient reached {k}"
        assert torch.isfinite(p.grad).all(), k
        e_got = max(rel_err(p.grad.detach().cpu().double(), truth[k][0]))
        e_ref = max(rel_err(truth[k][1], truth[k][0]))
        worst = max(worst, (e_got, e_ref, k))
        if e_got > truth_bar(e_ref):
            bad.append((e_got, e_ref, k))
    print("%s: %d gradient tensors, worst error vs float64 truth: e_got %.3e (e_ref %.3e) %s"
          % (pattern, len(trainable) + input_grad, *worst))
    assert not bad, "gradients off the float64 truth (build, reference fp32, name): " + \
        "; ".join("%.3e %.3e %s" % b for b in sorted(bad, reverse=True)[:8])
