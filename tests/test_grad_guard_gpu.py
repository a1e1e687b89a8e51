"""GPU: the guarded optimizer step - wm_grad_guard against cpu_twin.grad_guard on the kernel cases of tests/grad_guard_cases.py,
the contract of torch's fused AdamW that the guard relies on (found_inf, grad_scale), a captured guard + AdamW graph, whole
captured training steps of the wf = 8 network (GraphedTrainStep, a one-rank GraphedDDPTrainStep in both collective modes) and
recipe.Trainer with the train.grad_guard block.

The bar for the norm is 2 ulp of fp32: the squares are exact in double, <= 2^21 double additions contribute < 2e-10 relative, the
rounding to fp32 <= 0.5 ulp, and the second ulp is the device's double sqrt.  found_inf and grad_scale must be exactly what the
formula gives from the kernel's OWN fp32 norm.  Nothing here provokes a fault: the poison is a non-finite GRADIENT VALUE (a tensor
hook multiplies one parameter's gradient by a device scalar); the forward and every index the network computes stay finite."""
import copy
import json
import os
import socket
from datetime import timedelta

import numpy as np
import pytest
import torch

import wave_mamba_amd as wm
from wave_mamba_amd import cpu_twin, ops, recipe, trainer
import grad_guard_cases as cases
from test_recipe_cpu import TRAIN_SHAPES, make_store, small_opt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL = dict(in_chn=3, wf=8, n_l_blocks=[1, 1, 1], n_h_blocks=[1, 1, 1], ffn_scale=2.0)       # tests/test_deterministic_gpu.py


# ---- the kernel against the twin ---------------------------------------------------------------------------------------------------
def _check(tensors, max_norm=None, record=None, **kw):
    """ops.grad_guard on device views of `tensors` (CPU) against the twin; -> the record as a list of floats."""
    rec, skipped = ops.grad_guard(tensors, max_norm, record=record, **kw)
    want = cpu_twin.grad_guard(tensors, max_norm)
    got = rec.cpu()
    print(f"norm {float(got[0])!r} twin {float(want[0])!r}  found_inf {float(got[1])} / {float(want[1])}  "
          f"grad_scale {float(got[2])!r} / {float(want[2])!r}")
    assert float(got[1]) == float(want[1]) and float(got[3]) == 0.0
    if np.isfinite(float(want[0])):
        assert cases.norm_within_2ulp(float(got[0]), float(want[0])), (float(got[0]), float(want[0]))
    else:
        assert not np.isfinite(float(got[0]))
    assert np.float32(float(got[2])) == cases.expected_scale(float(got[0]), float(got[1]), max_norm)
    return got.tolist()


@pytest.mark.parametrize("offset", cases.OFFSETS)
def test_lengths_at_every_offset(offset):
    for n in cases.LENGTHS:
        view = cases.at_offset(cases.randn(n, 10 + n), offset, DEV)
        table, n_rows = ops.grad_guard_table([view])
        assert n_rows == (n + cases.CHUNK - 1) // cases.CHUNK and table.shape == (n_rows, 2)
        assert n == 0 or (int(table[0, 0]) == view.data_ptr() and int(table[:, 1].sum()) == n and int(table[:, 1].max()) <= cases.CHUNK)
        _check([view])


def test_a_row_of_count_zero_and_a_row_longer_than_a_chunk():
    """Rows written by hand: count = 0 is allowed (between two real rows), and a count above CHUNK is summed by its one workgroup."""
    a, b = cases.at_offset(cases.randn(37, 1), 3, DEV), cases.at_offset(cases.randn(3 * cases.CHUNK + 1, 2), 2, DEV)
    table = torch.tensor([[a.data_ptr(), a.numel()], [a.data_ptr(), 0], [b.data_ptr(), b.numel()]], dtype=torch.int64, device=DEV)
    rec, _ = ops.grad_guard((table, 3), 1e-3)
    want = cpu_twin.grad_guard([a, b], 1e-3)
    assert cases.norm_within_2ulp(float(rec[0]), float(want[0])) and float(rec[1]) == 0.0
    assert np.float32(float(rec[2])) == cases.expected_scale(float(rec[0]), 0.0, 1e-3)


def test_many_tensors_and_the_empty_list():
    tensors = [t.to(DEV) for t in cases.many()]
    table, n_rows = ops.grad_guard_table(tensors)
    assert n_rows == sum((n + cases.CHUNK - 1) // cases.CHUNK for n in cases.MANY_SIZES) > cases.MANY
    _check(tensors, 1.0)
    rec, skipped = ops.grad_guard([], 1.0, record=torch.full((4,), float("nan"), device=DEV))
    assert rec.tolist() == [0.0, 0.0, 1.0, 0.0] and int(skipped) == 0


@pytest.mark.parametrize("name", sorted(cases.value_cases()))
def test_values(name):
    tensors, finite, norm_finite = cases.value_cases()[name]
    got = _check([cases.at_offset(t, 1, DEV) for t in tensors], 1.0)
    assert got[1] == (0.0 if finite and norm_finite else 1.0) and got[0] > 0.0


@pytest.mark.parametrize("kind", sorted(cases.NONFINITE))
def test_nonfinite_elements(kind):
    bits = cases.NONFINITE[kind]
    for place in cases.POISON_PLACES:
        got = _check([cases.at_offset(cases.poisoned(bits, place), cases.POISON_OFFSET, DEV)], 1e-3)
        assert got[1:] == [1.0, 1.0, 0.0], (kind, place)
    one = cases.at_offset(cases.bits_scalar(bits), 2, DEV)
    assert int(one.view(torch.int32)[0]) & 0xffffffff == bits                              # the bit pattern reached the device
    assert _check([one], 1e-3)[1:] == [1.0, 1.0, 0.0]
    tensors = cases.many()
    tensors[-1] = tensors[-1].clone()
    tensors[-1].view(torch.int32)[-1] = cases.bits_scalar(bits).view(torch.int32)[0]
    assert _check([t.to(DEV) for t in tensors], 1e-3)[1:] == [1.0, 1.0, 0.0]


def test_clipping():
    t = [cases.at_offset(cases.randn(2 * cases.CHUNK + 3, 1), 1, DEV)]
    small = [cases.at_offset(cases.randn(5, 2, 1e-3), 3, DEV)]
    for tensors in (t, small):
        norm = float(ops.grad_guard(tensors)[0][0])
        assert _check(tensors, 1e-3)[2] > 1.0
        assert 1.0 <= _check(tensors, norm)[2] < 1.0 + 1e-2
        assert _check(tensors, 1e9)[2] == 1.0
        assert _check(tensors, None)[2] == 1.0
    assert _check(small, float(ops.grad_guard(small)[0][0]))[2] > 1.0


def test_reproducible_whatever_the_workspace_and_the_record_held():
    tensors = [t.to(DEV) for t in cases.many(seed=5)]
    pair = ops.grad_guard_table(tensors)
    first, _ = ops.grad_guard(pair, 1e-3)
    again, _ = ops.grad_guard(pair, 1e-3)
    assert torch.equal(first, again)
    nbytes = wm._lib.load().wm_grad_guard_workspace_bytes(pair[1])
    dirty = torch.full((nbytes + 64,), 0xFF, dtype=torch.uint8, device=DEV)               # every double a NaN, every flag set
    rec, _ = ops.grad_guard(pair, 1e-3, record=torch.full((4,), float("nan"), device=DEV), workspace=dirty)
    assert torch.equal(rec, first) and float(rec[1]) == 0.0
    with pytest.raises(RuntimeError, match="workspace"):
        ops.grad_guard(pair, 1e-3, workspace=dirty[:nbytes - 16])
    record, skipped = torch.empty(4, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    x = cases.at_offset(cases.randn(100, 1), 1, DEV)
    pair = ops.grad_guard_table([x])
    for value, want in ((1.0, 0), (float("nan"), 1), (float("inf"), 2), (2.0, 2)):
        x[50] = value
        ops.grad_guard(pair, None, record, skipped)
        assert int(skipped) == want and float(record[1]) == (0.0 if np.isfinite(value) else 1.0)


# ---- the fused AdamW's contract ----------------------------------------------------------------------------------------------------
def _five(seed, capturable=False):
    g = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(n, generator=g).to(DEV)) for n in (1, 5, 64, 257, 1030)]
    lr = torch.tensor(1e-2, device=DEV) if capturable else 1e-2
    opt = torch.optim.AdamW(params, lr=lr, weight_decay=1e-3, betas=(0.9, 0.99), fused=True, capturable=capturable)
    return params, opt


def _opt_state(params, opt):
    return [p.detach().clone() for p in params] + [opt.state[p][k].clone() for p in params for k in ("exp_avg", "exp_avg_sq", "step")]


@pytest.mark.parametrize("capturable", [False, True])
def test_fused_adamw_honours_found_inf_and_grad_scale(capturable):
    """What GradGuard.attach relies on: found_inf = 1 leaves params, both moments and `step` bit-equal; grad_scale = s from zero
    state gives exp_avg = (1 - beta1) g / s to 1e-6 relative of float64 (six fp32 roundings at 2^-24 each)."""
    params, opt = _five(0, capturable)
    g = torch.Generator().manual_seed(1)
    grads = [torch.randn(p.shape, generator=g) for p in params]
    for p, gr in zip(params, grads):
        p.grad = gr.to(DEV)
    opt.step()
    before = _opt_state(params, opt)
    opt.found_inf = torch.ones((), device=DEV)
    opt.step()
    assert all(torch.equal(a, b) for a, b in zip(before, _opt_state(params, opt))), "found_inf = 1 did not leave the state alone"
    opt.found_inf.zero_()
    opt.step()
    assert not torch.equal(before[0], params[0].detach()) and float(opt.state[params[0]]["step"]) == 2.0
    params, opt = _five(0, capturable)
    s = 3.7
    opt.grad_scale = torch.tensor(s, device=DEV)
    for p, gr in zip(params, grads):
        p.grad = gr.to(DEV)
    opt.step()
    for p, gr in zip(params, grads):
        want = 0.1 * gr.double() / float(np.float32(s))
        got = opt.state[p]["exp_avg"].cpu().double()
        assert float(((got - want).abs() / want.abs()).max()) <= 1e-6
        assert float(((p.grad.cpu().double() - gr.double() / float(np.float32(s))).abs() / gr.double().abs()).max()) <= 1e-6


# ---- a captured guard + AdamW graph ------------------------------------------------------------------------------------------------
class _CapturedGuardedAdamW:
    """Six static gradient tensors, the guard's launch and optimizer.step() in one graph; the optimizer's state starts at zero."""
    LENGTHS = (1, 3, 5, cases.CHUNK - 1, cases.CHUNK + 1, 2 * cases.CHUNK + 3)

    def __init__(self, max_norm, skip_nonfinite=True):
        g = torch.Generator().manual_seed(0)
        self.params = [torch.nn.Parameter(torch.randn(n, generator=g).to(DEV)) for n in self.LENGTHS]
        self.grads = [cases.at_offset(torch.zeros(n), k % 4, DEV) for k, n in enumerate(self.LENGTHS)]
        self.opt = torch.optim.AdamW(self.params, lr=torch.tensor(1e-2, device=DEV), weight_decay=1e-3, betas=(0.9, 0.99), fused=True,
                                     capturable=True)
        self.guard = trainer.GradGuard(max_norm=max_norm, skip_nonfinite=skip_nonfinite).attach(self.opt)
        for p, gr in zip(self.params, self.grads):
            p.grad = gr
        start = [p.detach().clone() for p in self.params]
        self.table = table = ops.grad_guard_table(self.grads)       # the graph replays a launch on the table's address
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):                               # one eager step: the optimizer's state exists before the capture
            self.guard.run(self.grads, table=table)
            self.opt.step()
        torch.cuda.current_stream(DEV).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.guard.run(self.grads, table=table)
            self.opt.step()
        with torch.no_grad():
            for p, s0 in zip(self.params, start):
                p.copy_(s0)
            for st in self.opt.state.values():
                for v in st.values():
                    v.zero_()
        self.guard.set_skipped(0)

    def replay(self, grads):
        for mine, new in zip(self.grads, grads):
            mine.copy_(new)
        self.graph.replay()
        return _opt_state(self.params, self.opt)


def test_captured_guard_and_adamw_skip_clip_and_continue():
    g = torch.Generator().manual_seed(2)
    small = [torch.randn(n, generator=g) * 1e-3 for n in _CapturedGuardedAdamW.LENGTHS]              # norm ~ 0.13: below max_norm
    last = [torch.randn(n, generator=g) * 1e-3 for n in _CapturedGuardedAdamW.LENGTHS]
    large = [torch.randn(n, generator=g) for n in _CapturedGuardedAdamW.LENGTHS]                     # norm ~ 130: clipped
    bad = [t.clone() for t in small]
    bad[3][-1] = float("inf")
    run, twin = _CapturedGuardedAdamW(1.0), _CapturedGuardedAdamW(1.0)
    s1 = run.replay(small)
    assert float(run.guard.found_inf) == 0.0 and float(run.guard.grad_scale) == 1.0 and int(run.guard.skipped) == 0
    assert cases.norm_within_2ulp(float(run.guard.norm), float(cpu_twin.grad_guard(small)[0]))
    s2 = run.replay(bad)
    assert all(torch.equal(a, b) for a, b in zip(s1, s2)), "the replay with an inf gradient moved a weight, a moment or a step counter"
    assert float(run.guard.found_inf) == 1.0 and float(run.guard.grad_scale) == 1.0 and int(run.guard.skipped) == 1
    run.replay(large)
    norm, scale = float(run.guard.norm), float(run.guard.grad_scale)
    assert cases.norm_within_2ulp(norm, float(cpu_twin.grad_guard(large)[0])) and float(run.guard.found_inf) == 0.0
    assert np.float32(scale) == cases.expected_scale(norm, 0.0, 1.0) and scale > 100.0
    for mine, new in zip(run.grads, large):                         # the optimizer's kernel left g / grad_scale in p.grad
        assert float(((mine.cpu().double() - new.double() / scale).abs()).max()) <= 1e-6 * float(new.abs().max()) / scale
    s4 = run.replay(last)
    twin.replay(small)
    twin.replay(large)
    t3 = twin.replay(last)
    assert all(torch.equal(a, b) for a, b in zip(s4, t3)), "after the skipped replay the run is not the twin's that never saw it"
    assert int(run.guard.skipped) == 1 and int(twin.guard.skipped) == 0 and float(run.opt.state[run.params[0]]["step"]) == 3.0


def _counter_arguments(fn):
    """What reached wm_grad_guard's `skipped` argument in the launches made inside fn()."""
    seen, real = [], ops._launch

    def spying(dev, name, *args, **kw):
        if name == "wm_grad_guard":
            seen.append(args[4])
        return real(dev, name, *args, **kw)
    ops._launch = spying
    try:
        fn()
    finally:
        ops._launch = real
    return seen


def test_a_guard_that_does_not_skip_clips_and_counts_nothing():
    """GradGuard(max_norm=M, skip_nonfinite=False), eagerly (train_step) and captured: NULL reaches the entry point in place of the
    counter, which stays 0; optimizer.found_inf is not set while grad_scale is; clipping applies; a step with an inf gradient is
    flagged in the record and TAKEN (that is what the option says)."""
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(4, 3, 3, padding=1)).to(DEV)
    opt = trainer.make_optimizer(net)
    g = torch.Generator().manual_seed(3)
    lq, gt = torch.rand(2, 3, 16, 16, generator=g).to(DEV), torch.rand(2, 3, 16, 16, generator=g).to(DEV)
    guard = trainer.GradGuard(max_norm=1e-4, skip_nonfinite=False)
    seen = _counter_arguments(lambda: trainer.train_step(net, opt, lq, gt, as_float=False, guard=guard))
    assert seen == [None]
    assert getattr(opt, "found_inf", None) is None and opt.grad_scale.data_ptr() == guard.grad_scale.data_ptr()
    norm, scale = float(guard.norm), float(guard.grad_scale)
    assert norm > 1e-4 and np.float32(scale) == cases.expected_scale(norm, 0.0, 1e-4) > 1.0 and int(guard.skipped) == 0
    clipped = cpu_twin.grad_guard([p.grad for p in net.parameters()])                   # the kernel left g / grad_scale in p.grad
    assert abs(float(clipped[0]) * scale - norm) <= 1e-5 * norm
    assert float(opt.state[net[0].weight]["step"]) == 1.0

    large = [torch.randn(n, generator=g) for n in _CapturedGuardedAdamW.LENGTHS]
    bad = [t.clone() for t in large]
    bad[2][1] = float("inf")
    made = []
    assert _counter_arguments(lambda: made.append(_CapturedGuardedAdamW(1.0, skip_nonfinite=False))) == [None, None]
    run = made[0]
    assert getattr(run.opt, "found_inf", None) is None and run.opt.grad_scale.data_ptr() == run.guard.grad_scale.data_ptr()
    run.replay(large)
    assert float(run.guard.found_inf) == 0.0 and float(run.guard.grad_scale) > 100.0 and int(run.guard.skipped) == 0
    for mine, new in zip(run.grads, large):
        assert float((mine.cpu().double() - new.double() / float(run.guard.grad_scale)).abs().max()) <= 1e-6 * float(new.abs().max())
    run.replay(bad)
    assert run.guard.record.tolist()[1:] == [1.0, 1.0, 0.0] and int(run.guard.skipped) == 0
    assert float(run.opt.state[run.params[0]]["step"]) == 2.0, "a guard that does not skip withheld a step"


# ---- whole captured steps ------------------------------------------------------------------------------------------------------------
def _batches():
    g = torch.Generator().manual_seed(11)
    return torch.rand(3, 2, 3, 64, 64, generator=g).to(DEV), torch.rand(3, 2, 3, 64, 64, generator=g).to(DEV)


class _Step:
    """A captured step of the wf = 8 network from seed 0 whose constructor's warm-up is undone (weights back in place, AdamW's state
    zeroed, the counter at 0): every run starts from the same weights and zero moments.  kind: "single" (GraphedTrainStep),
    "split" / "captured" (GraphedDDPTrainStep over an initialised one-rank group)."""

    def __init__(self, kind, guard, lq, gt, spy=None):
        torch.manual_seed(0)
        self.net = wm.WaveMamba(**SMALL).train().to(DEV)
        self.poison = torch.ones((), device=DEV)
        self.net.restoration_network.last.weight.register_hook(lambda grad: grad * self.poison)
        self.opt = trainer.make_optimizer(self.net, capturable=True)
        self.params = [p for g in self.opt.param_groups for p in g["params"]]
        self.guard = guard
        start = [p.detach().clone() for p in self.net.parameters()]
        real = ops._launch
        if spy is not None:
            def spying(dev, name, *args, **kw):
                spy.append(name)
                return real(dev, name, *args, **kw)
            ops._launch = spying
        try:
            if kind == "single":
                self.step = trainer.GraphedTrainStep(self.net, self.opt, lq, gt, guard=guard)
            else:
                self.step = trainer.GraphedDDPTrainStep(self.net, self.opt, lq, gt, collective=kind, guard=guard)
        finally:
            ops._launch = real
        with torch.no_grad():
            for p, s0 in zip(self.net.parameters(), start):
                p.copy_(s0)
            for st in self.opt.state.values():
                for v in st.values():
                    v.zero_()
        if guard is not None:
            guard.set_skipped(0)

    def __call__(self, lq, gt, poison=1.0):
        self.poison.fill_(poison)
        self.step(lq, gt)
        torch.cuda.synchronize()
        return [p.detach().cpu() for p in self.params] + [self.opt.state[p][k].cpu() for p in self.params for k in ("exp_avg", "exp_avg_sq", "step")]

    def grads(self):
        if hasattr(self.step, "flat"):
            nl = len(self.step.losses) if not isinstance(self.step, trainer.GraphedTrainStep) else 0
            return self.step.flat[:self.step.flat.numel() - nl].cpu()
        return torch.cat([p.grad.reshape(-1) for p in self.params]).cpu()


def _whole_step(kind):
    """The runs of one step form -> plain CPU values (this also runs inside a spawned worker, for the forms that need a group)."""
    lq, gt = _batches()
    out, launched_plain, launched_guarded = {}, [], []
    plain = _Step(kind, None, lq[0], gt[0], spy=launched_plain)
    p1 = plain(lq[0], gt[0])
    out["plain_grads_1"] = plain.grads()
    out["plain"] = [p1, plain(lq[2], gt[2]), plain(lq[1], gt[1])]
    neutral = _Step(kind, trainer.GradGuard(), lq[0], gt[0], spy=launched_guarded)
    n1 = neutral(lq[0], gt[0])
    out["norm_1"] = float(neutral.guard.norm)
    out["neutral"] = [n1, neutral(lq[2], gt[2]), neutral(lq[1], gt[1])]
    out["neutral_skipped"] = int(neutral.guard.skipped)
    out["launched_plain"], out["launched_guarded"] = launched_plain.count("wm_grad_guard"), launched_guarded.count("wm_grad_guard")
    del plain, neutral
    poisoned = _Step(kind, trainer.GradGuard(), lq[0], gt[0])
    out["poisoned"] = [poisoned(lq[0], gt[0]), poisoned(lq[1], gt[1], float("inf"))]
    out["poisoned_record_2"] = poisoned.guard.record.tolist()
    out["poisoned"].append(poisoned(lq[2], gt[2]))
    out["poisoned_skipped"], out["poisoned_record_3"] = int(poisoned.guard.skipped), poisoned.guard.record.tolist()
    del poisoned
    clipped = _Step(kind, trainer.GradGuard(max_norm=0.5 * out["norm_1"]), lq[0], gt[0])
    out["clipped"] = clipped(lq[0], gt[0])
    out["clipped_record"] = clipped.guard.record.tolist()
    out["n_params"] = len(clipped.params)
    return out


def _ddp_worker(rank, port, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    torch.cuda.set_device(0)
    wm.set_deterministic(True)
    dist.init_process_group("nccl", device_id=torch.device("cuda", 0), rank=0, world_size=1, timeout=timedelta(seconds=120))
    try:
        torch.save({kind: _whole_step(kind) for kind in ("split", "captured")}, os.path.join(out_dir, "ddp.pt"))
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def whole(tmp_path_factory):
    """kind -> _whole_step(kind): the single-process form here, the two one-rank RCCL forms in one spawned worker."""
    import torch.multiprocessing as mp
    prev = wm.set_deterministic(True)
    try:
        res = {"single": _whole_step("single")}
    finally:
        wm.set_deterministic(prev)
    out = tmp_path_factory.mktemp("grad_guard_ddp")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_ddp_worker, args=(port, str(out)), nprocs=1, join=True)
    res.update(torch.load(out / "ddp.pt", weights_only=False))
    return res


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


KINDS = ["single", "split", "captured"]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kind", KINDS)
def test_whole_step_neutral_guard_changes_nothing(whole, kind):
    """(a) guard=GradGuard() on finite data: three steps end on torch.equal weights and moments; without a guard no wm_grad_guard
    is launched (and with one, the warm-up steps and the capture launch it)."""
    r = whole[kind]
    for s in range(3):
        assert _equal(r["plain"][s], r["neutral"][s]), f"step {s + 1}: the guarded run differs from the unguarded one"
    assert not _equal(r["plain"][0], r["plain"][1])
    assert r["launched_plain"] == 0 and r["launched_guarded"] >= 1 and r["neutral_skipped"] == 0 and r["norm_1"] > 0.0


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kind", KINDS)
def test_whole_step_skips_the_poisoned_step_and_continues(whole, kind):
    """(b) poison 1 / inf / 1: the second replay leaves weights, moments and step counters torch.equal, the third equals the second
    step of the run that never saw it (the neutral run: batches 0, 2), skipped == 1."""
    r = whole[kind]
    assert _equal(r["poisoned"][0], r["neutral"][0])
    assert _equal(r["poisoned"][1], r["poisoned"][0]), "the poisoned replay moved a weight, a moment or a step counter"
    assert r["poisoned_record_2"][1:] == [1.0, 1.0, 0.0]
    assert _equal(r["poisoned"][2], r["neutral"][1]), "the replay after the skipped one is not the unpoisoned run's second step"
    assert r["poisoned_skipped"] == 1 and r["poisoned_record_3"][1] == 0.0
    n = r["n_params"]
    assert {float(v) for v in r["poisoned"][2][n + 2::3]} == {2.0}                # AdamW's own counters: two steps taken


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kind", KINDS)
def test_whole_step_clipping_agrees_with_the_unclipped_norm(whole, kind):
    """(c) max_norm = half the first step's norm: guard.norm is the twin's norm of the UNGUARDED run's gradients (2 ulp), and
    exp_avg after the first step - linear in the gradient - is the unclipped run's divided by grad_scale, to 1e-6 relative,
    element by element (three fp32 roundings at 2^-24 apart: g / s and its product with 1 - beta1 on one side, the product alone
    on the other).  Entries below 1e-30 are left out: zeros have no relative error, and within 2^24 of the smallest normal fp32
    number a rounding is no longer 2^-24 of the value.  (Weights are not compared: Adam's first update is scale-invariant.)"""
    r = whole[kind]
    norm, found, scale, _ = r["clipped_record"]
    want = float(cpu_twin.grad_guard([r["plain_grads_1"]])[0])
    print(f"{kind}: guard.norm {norm!r}, twin of the unguarded gradients {want!r}, grad_scale {scale!r}")
    assert cases.norm_within_2ulp(norm, want) and cases.norm_within_2ulp(r["norm_1"], want) and found == 0.0
    assert np.float32(scale) == cases.expected_scale(norm, 0.0, 0.5 * r["norm_1"]) and 1.9 < scale < 2.1
    n = r["n_params"]
    for k in range(n):
        clipped, plain = r["clipped"][n + 3 * k].double(), r["plain"][0][n + 3 * k].double() / scale
        keep = plain.abs() >= 1e-30
        assert bool(keep.any()) or float(plain.abs().max()) == 0.0, k
        if bool(keep.any()):
            worst = float(((clipped - plain).abs() / plain.abs())[keep].max())
            assert worst <= 1e-6, (k, worst)
        assert float(clipped[~keep].abs().max() if bool((~keep).any()) else 0.0) < 1e-30, k


# ---- the recipe ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
def test_recipe_logs_the_norm_and_resumes_exactly(tmp_path):
    """recipe.Trainer, graphed, 6 iterations with the block: every log line carries grad_norm > 0 and skipped_steps == 0, and a run
    resumed from iteration 3 reproduces iterations 4-6 bit for bit."""
    prev = wm.set_deterministic(True)
    try:
        opt = small_opt(total_iter=6, print_freq=1, save_checkpoint_freq=3)
        opt["train"]["grad_guard"] = {"max_norm": 1.0, "skip_nonfinite": True}
        runs = {}
        for name in ("whole", "resumed"):
            if name == "resumed":
                opt = copy.deepcopy(opt)
                opt["path"]["resume_state"] = str(tmp_path / "whole" / "training_states" / "3.state")
            t = recipe.Trainer(opt, make_store(DEV, TRAIN_SHAPES, 1), graphed=True, out_dir=str(tmp_path / name))
            weights = []
            t.run(on_iter=lambda it, epoch, lrs, rows, losses: weights.append((it, [p.detach().clone() for p in t.net.parameters()])))
            assert isinstance(t._gstep, trainer.GraphedTrainStep) and t._gstep.guard is t.guard
            runs[name] = (t, weights, [json.loads(l) for l in open(tmp_path / name / "train.log")])
    finally:
        wm.set_deterministic(prev)
    t, weights, lines = runs["whole"]
    lines = [l for l in lines if "l_pix" in l]
    assert [l["iter"] for l in lines] == [1, 2, 3, 4, 5, 6]
    print("grad_norm per iteration:", [l["grad_norm"] for l in lines])
    assert all(l["grad_norm"] > 0.0 and np.isfinite(l["grad_norm"]) and l["skipped_steps"] == 0 for l in lines)
    assert {float(st["step"]) for st in t.optimizer.state.values()} == {6.0}                 # the guarded warm-up steps were undone
    assert torch.load(tmp_path / "whole" / "training_states" / "3.state", weights_only=True)["recipe"]["skipped_steps"] == 0
    t2, weights2, lines2 = runs["resumed"]
    assert [it for it, _ in weights2] == [4, 5, 6]
    for (it, a), (_, b) in zip(weights[3:], weights2):
        assert _equal(a, b), f"iteration {it}: the resumed run differs"
    assert [l["grad_norm"] for l in lines2 if "l_pix" in l] == [l["grad_norm"] for l in lines[3:]]
