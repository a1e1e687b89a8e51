"""CPU: the guarded optimizer step without a GPU - the two entry points' host-side refusals, cpu_twin.grad_guard against numpy
float64, train_step(..., guard=) and the gloo GraphedDDPTrainStep(capture=False, guard=) skipping a poisoned step, and the recipe's
train.grad_guard block (options, state round trip, log line).  The kernel itself: tests/test_grad_guard_gpu.py."""
import copy
import json
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import wave_mamba_amd as wm
from wave_mamba_amd import _lib, cpu_twin, ops, recipe, trainer
import grad_guard_cases as cases
from test_ddp_gloo import CFG, free_port
from test_recipe_cpu import TRAIN_SHAPES, make_store, small_opt


# ---- 1. the C ABI, by host arithmetic --------------------------------------------------------------------------------------------
def test_entry_points_refuse_before_any_launch():
    """Negative n_rows -> WM_EINVAL first; then a NULL record, table and workspace -> WM_ENULL; a short workspace ->
    WM_EWORKSPACE; odd pointers -> WM_EALIGN.  (The pointers are never dereferenced on the host: small integers stand in.)"""
    lib = _lib.load()
    N, P = None, 4096
    assert lib.wm_abi_version() == _lib.ABI_VERSION == 34
    assert lib.wm_grad_guard(N, -1, 1.0, N, N, N, 0, N) == _lib.WM_EINVAL
    assert lib.wm_grad_guard(P, -1, 1.0, P, P, P, 1 << 20, N) == _lib.WM_EINVAL
    assert lib.wm_grad_guard(N, 0, 1.0, N, N, N, 0, N) == _lib.WM_ENULL                  # the record is written even for no rows
    assert lib.wm_grad_guard(N, 3, 1.0, N, N, N, 0, N) == _lib.WM_ENULL
    assert lib.wm_grad_guard(N, 3, 1.0, P, P, P, 1 << 20, N) == _lib.WM_ENULL            # table
    assert lib.wm_grad_guard(P, 3, 1.0, P, P, N, 1 << 20, N) == _lib.WM_ENULL            # workspace
    need = lib.wm_grad_guard_workspace_bytes(3)
    assert lib.wm_grad_guard(P, 3, 1.0, P, P, P, need - 1, N) == _lib.WM_EWORKSPACE
    assert lib.wm_grad_guard(P, 3, 1.0, P, P, P, 0, N) == _lib.WM_EWORKSPACE
    assert lib.wm_grad_guard(P, 1 << 31, 1.0, P, P, P, 1 << 40, N) == _lib.WM_EUNSUPPORTED
    assert lib.wm_grad_guard(P + 4, 3, 1.0, P, P, P, need, N) == _lib.WM_EALIGN
    assert lib.wm_grad_guard(P, 3, 1.0, P + 2, P, P, need, N) == _lib.WM_EALIGN
    assert lib.wm_grad_guard(P, 3, 1.0, P, P + 4, P, need, N) == _lib.WM_EALIGN


def test_workspace_bytes_is_zero_for_no_rows_and_monotone():
    lib = _lib.load()
    assert lib.wm_grad_guard_workspace_bytes(0) == 0 and lib.wm_grad_guard_workspace_bytes(-5) == 0
    sizes = [lib.wm_grad_guard_workspace_bytes(n) for n in (1, 2, 3, 369, 1000, 1 << 20)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
    assert "wm_grad_guard" in _lib.SIGNATURES and "wm_grad_guard_workspace_bytes" in _lib.SIGNATURES
    assert ops.GRAD_GUARD_CHUNK >= 4 and ops.GRAD_GUARD_CHUNK % 4 == 0


def test_operator_layer_refuses_what_is_not_a_dense_fp32_cuda_tensor():
    with pytest.raises(ValueError, match="contiguous float32 CUDA"):
        ops.grad_guard_table([torch.zeros(4)])
    with pytest.raises(ValueError, match="contiguous float32 CUDA"):
        ops.grad_guard([torch.zeros(4, dtype=torch.float64)])


# ---- 2. the twin against numpy float64 ---------------------------------------------------------------------------------------------
def _check_twin(tensors, max_norm=None):
    rec = cpu_twin.grad_guard(tensors, max_norm)
    norm, found, scale = cases.numpy_record(tensors, max_norm)
    assert rec.dtype == torch.float32 and rec.shape == (4,) and float(rec[3]) == 0.0
    assert float(rec[1]) == found
    if np.isfinite(norm):
        assert cases.norm_within_2ulp(float(rec[0]), norm), (float(rec[0]), float(norm))
    else:
        assert not np.isfinite(float(rec[0]))
    assert np.float32(float(rec[2])) == cases.expected_scale(float(rec[0]), found, max_norm) and (found == 0.0 or float(rec[2]) == 1.0)
    return rec


@pytest.mark.parametrize("offset", cases.OFFSETS)
def test_twin_lengths_and_offsets(offset):
    for n in cases.LENGTHS:
        _check_twin([cases.at_offset(cases.randn(n, 10 + n), offset)])


def test_twin_many_tensors_empty_list_and_values():
    _check_twin(cases.many())
    assert cpu_twin.grad_guard([]).tolist() == [0.0, 0.0, 1.0, 0.0]
    assert cpu_twin.grad_guard([], 1.0).tolist() == [0.0, 0.0, 1.0, 0.0]
    for name, (tensors, finite, norm_finite) in cases.value_cases().items():
        rec = _check_twin(tensors, 1.0)
        assert float(rec[1]) == (0.0 if finite and norm_finite else 1.0), name
        assert float(rec[0]) > 0.0, name                                              # 1e19 and 1e-30 neither overflow nor vanish


@pytest.mark.parametrize("kind", sorted(cases.NONFINITE))
def test_twin_nonfinite_elements(kind):
    bits = cases.NONFINITE[kind]
    for place in cases.POISON_PLACES:
        rec = _check_twin([cases.at_offset(cases.poisoned(bits, place), cases.POISON_OFFSET)], 1e-3)
        assert rec[1:].tolist() == [1.0, 1.0, 0.0], (kind, place)
    assert cpu_twin.grad_guard([cases.bits_scalar(bits)], 1e-3)[1:].tolist() == [1.0, 1.0, 0.0]
    tensors = cases.many()
    tensors[-1] = tensors[-1].clone()
    tensors[-1].view(torch.int32)[-1] = cases.bits_scalar(bits).view(torch.int32)[0]
    assert _check_twin(tensors, 1e-3)[1:].tolist() == [1.0, 1.0, 0.0]


def test_twin_clipping():
    t = [cases.randn(2 * cases.CHUNK + 3, 1)]
    norm = float(cpu_twin.grad_guard(t)[0])
    assert float(_check_twin(t, 1e-3)[2]) > 1.0
    assert 1.0 <= float(_check_twin(t, norm)[2]) < 1.0 + 1e-5                             # (norm + 1e-6) / norm: 1 at this norm (~90)
    small = [cases.randn(5, 2, 1e-3)]
    assert float(_check_twin(small, float(cpu_twin.grad_guard(small)[0]))[2]) > 1.0           # ... and above 1 at a norm of ~2e-3
    assert float(_check_twin(t, 1e9)[2]) == 1.0


# ---- 3. train_step on the CPU --------------------------------------------------------------------------------------------------------
def _small_net(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(4, 4, 3, padding=1),
                               torch.nn.ReLU(), torch.nn.Conv2d(4, 3, 3, padding=1))


def _snapshot(net, optimizer):
    state = [v.clone() for st in optimizer.state.values() for v in st.values() if isinstance(v, torch.Tensor)]
    return [p.detach().clone() for p in net.parameters()] + state


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_train_step_skips_the_poisoned_step_and_continues():
    """poison 1 / inf / 1 through a tensor hook on one parameter's gradient: the second step leaves weights and optimizer state
    torch.equal, the third equals the second step of a run that never saw the poisoned step, skipped == 1; the loss dict keeps
    its keys."""
    g = torch.Generator().manual_seed(3)
    lq, gt = torch.rand(3, 2, 3, 16, 16, generator=g), torch.rand(3, 2, 3, 16, 16, generator=g)
    net, twin = _small_net(), _small_net()
    poison = torch.ones(())
    net[2].weight.register_hook(lambda grad: grad * poison)
    opt, opt_twin = trainer.make_optimizer(net), trainer.make_optimizer(twin)
    guard, guard_twin = trainer.GradGuard(), trainer.GradGuard()
    keys = set(trainer.train_step(net, opt, lq[0], gt[0], guard=guard))
    assert keys == {"l_pix", "l_freq"} and int(guard.skipped) == 0 and float(guard.found_inf) == 0.0 and float(guard.norm) > 0.0
    before = _snapshot(net, opt)
    poison.fill_(float("inf"))
    assert set(trainer.train_step(net, opt, lq[1], gt[1], guard=guard)) == keys
    assert _same(_snapshot(net, opt), before), "the poisoned step moved a weight or a moment"
    assert int(guard.skipped) == 1 and float(guard.found_inf) == 1.0 and float(guard.grad_scale) == 1.0
    poison.fill_(1.0)
    trainer.train_step(net, opt, lq[2], gt[2], guard=guard)
    trainer.train_step(twin, opt_twin, lq[0], gt[0], guard=guard_twin)
    trainer.train_step(twin, opt_twin, lq[2], gt[2], guard=guard_twin)
    assert _same(_snapshot(net, opt), _snapshot(twin, opt_twin)), "the step after the skipped one is not the twin run's second step"
    assert int(guard.skipped) == 1 and int(guard_twin.skipped) == 0 and float(guard.found_inf) == 0.0
    assert getattr(opt, "found_inf", None) is None and getattr(opt, "grad_scale", None) is None     # the non-fused AdamW takes neither


def test_train_step_without_a_guard_and_with_a_neutral_one_agree_and_clipping_divides():
    g = torch.Generator().manual_seed(4)
    lq, gt = torch.rand(2, 3, 16, 16, generator=g), torch.rand(2, 3, 16, 16, generator=g)
    nets = [_small_net() for _ in range(3)]
    opts = [trainer.make_optimizer(n) for n in nets]
    trainer.train_step(nets[0], opts[0], lq, gt)
    trainer.train_step(nets[1], opts[1], lq, gt, guard=trainer.GradGuard())
    assert _same(_snapshot(nets[0], opts[0]), _snapshot(nets[1], opts[1]))
    unclipped = [p.grad.clone() for p in nets[0].parameters()]
    norm = float(cpu_twin.grad_guard(unclipped)[0])
    guard = trainer.GradGuard(max_norm=0.5 * norm)
    trainer.train_step(nets[2], opts[2], lq, gt, guard=guard)
    assert float(guard.norm) == norm and float(guard.grad_scale) == cases.expected_scale(norm, 0.0, 0.5 * norm) > 1.9
    for p, want in zip(nets[2].parameters(), unclipped):
        assert torch.equal(p.grad, want / float(guard.grad_scale))
    for bad in (0.0, -1.0, float("inf"), float("nan"), "1", True):
        with pytest.raises(ValueError, match="max_norm"):
            trainer.GradGuard(max_norm=bad)


# ---- 4. gloo, world 2 ------------------------------------------------------------------------------------------------------------------
def _gloo_worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    import wave_mamba_amd as wm
    from oracle import oracle
    from oracle import backend as oracle_backend
    oracle.set_num_threads(2)
    oracle_backend.set_ops_backend(oracle)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        g = torch.Generator().manual_seed(77)
        lq, gt = torch.rand(3, 2, 3, 32, 32, generator=g), torch.rand(3, 2, 3, 32, 32, generator=g)      # [step][image]
        shard = slice(rank, rank + 1)
        torch.manual_seed(0)
        net = wm.WaveMamba(**CFG).train()
        poison = torch.ones(())
        if rank == 1:                                               # only rank 1 is poisoned: the REDUCED gradients decide
            net.restoration_network.last.weight.register_hook(lambda grad: grad * poison)
        opt = wm.trainer.make_optimizer(net)
        guard = wm.trainer.GradGuard(max_norm=1e9)
        step = wm.trainer.GraphedDDPTrainStep(net, opt, lq[0, shard], gt[0, shard], capture=False, guard=guard)
        rec = []
        for s, value in enumerate((1.0, float("inf"), 1.0)):
            poison.fill_(value)
            losses = step(lq[s, shard], gt[s, shard])
            rec.append({"keys": sorted(losses), "skipped": int(guard.skipped), "found_inf": float(guard.found_inf),
                        "norm": float(guard.norm), "w": [p.detach().clone() for p in net.parameters()],
                        "steps": sorted({float(st["step"]) for st in opt.state.values()})})
        torch.save(rec, os.path.join(out_dir, f"guard{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_gloo_both_ranks_skip_when_one_is_poisoned(tmp_path):
    mp.spawn(_gloo_worker, args=(2, free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"guard{r}.pt") for r in range(2))
    for s in range(3):
        assert r0[s]["keys"] == r1[s]["keys"] == ["l_freq", "l_pix"]
        assert _same(r0[s]["w"], r1[s]["w"]), f"step {s}: the ranks' weights differ"
        assert r0[s]["skipped"] == r1[s]["skipped"] == (0 if s == 0 else 1)
        assert r0[s]["found_inf"] == r1[s]["found_inf"] == (1.0 if s == 1 else 0.0)
    assert r0[0]["norm"] == r1[0]["norm"] > 0.0
    assert _same(r0[1]["w"], r0[0]["w"]) and r0[1]["steps"] == r0[0]["steps"] == [1.0], "the poisoned step was taken"
    assert not _same(r0[2]["w"], r0[1]["w"]) and r0[2]["steps"] == [2.0]


# ---- 5. the recipe ---------------------------------------------------------------------------------------------------------------------
def _guarded_opt(block, **kw):
    opt = small_opt(**kw)
    opt["train"]["grad_guard"] = block
    return opt


def test_check_options_accepts_and_refuses_the_block():
    for block in ({"max_norm": 1.0, "skip_nonfinite": True}, {"max_norm": None}, {"max_norm": 3}, {"skip_nonfinite": False}, {}):
        recipe.check_options(_guarded_opt(block))
    assert recipe.guard_options(small_opt()) is None
    assert recipe.guard_options(_guarded_opt({"max_norm": 2})) == {"max_norm": 2.0, "skip_nonfinite": True}
    assert recipe.guard_options(_guarded_opt({"max_norm": None, "skip_nonfinite": False})) == {"max_norm": None, "skip_nonfinite": False}
    text = "train:\n  grad_guard:\n    max_norm: 1.0        # or ~ : no clipping\n    skip_nonfinite: true\n"
    import yaml
    assert recipe.guard_options(yaml.safe_load(text)) == {"max_norm": 1.0, "skip_nonfinite": True}
    for block, key in (({"max_norm": 0}, "max_norm"), ({"max_norm": -1.0}, "max_norm"), ({"max_norm": "big"}, "max_norm"),
                       ({"max_norm": True}, "max_norm"), ({"max_norm": float("inf")}, "max_norm"), ({"max_norm": float("nan")}, "max_norm"),
                       ({"clip": 1.0}, "clip"), ({"skip_nonfinite": "yes"}, "skip_nonfinite"), ([1.0], "not a mapping")):
        with pytest.raises(ValueError, match=r"train\.grad_guard.*" + key):
            recipe.check_options(_guarded_opt(block))


def _stub_step(lq, gt):
    return {"l_pix": torch.tensor(0.5)}


def test_log_line_has_the_two_keys_only_with_the_block(tmp_path):
    for name, opt in (("plain", small_opt(total_iter=4, print_freq=2)),
                      ("guarded", _guarded_opt({"max_norm": 1.0}, total_iter=4, print_freq=2))):
        t = recipe.Trainer(opt, make_store("cpu", TRAIN_SHAPES, 1), out_dir=str(tmp_path / name), step_fn=_stub_step)
        assert (t.guard is not None) == (name == "guarded")
        t.run()
        lines = [json.loads(l) for l in open(tmp_path / name / "train.log")]
        lines = [l for l in lines if "l_pix" in l]
        assert len(lines) == 2
        for l in lines:
            assert set(l) == {"iter", "epoch", "lrs", "l_pix"} | ({"grad_norm", "skipped_steps"} if name == "guarded" else set())
        if name == "guarded":
            assert lines[-1]["skipped_steps"] == 0 and isinstance(lines[-1]["grad_norm"], float)


def test_state_round_trip_keeps_skipped_steps_and_a_state_without_it_resumes_at_zero(tmp_path):
    opt = _guarded_opt({"max_norm": 1.0}, total_iter=4, save_checkpoint_freq=2)
    t = recipe.Trainer(opt, make_store("cpu", TRAIN_SHAPES, 1), out_dir=str(tmp_path / "a"), step_fn=_stub_step)
    t.guard.set_skipped(7)
    t.run(max_iters=2)
    path = str(tmp_path / "a" / "training_states" / "2.state")
    state = torch.load(path, weights_only=True)
    assert state["recipe"]["skipped_steps"] == 7 and state["recipe"]["batch"] == 2
    opt2 = copy.deepcopy(opt)
    opt2["path"]["resume_state"] = path
    t2 = recipe.Trainer(opt2, make_store("cpu", TRAIN_SHAPES, 1), out_dir=str(tmp_path / "b"), step_fn=_stub_step)
    assert int(t2.guard.skipped) == 7 and t2.current_iter == 2
    # a state without the key (an unguarded run's), and one shaped like the reference's (no "recipe" entry at all)
    for drop in ("key", "recipe"):
        older = copy.deepcopy(state)
        if drop == "key":
            del older["recipe"]["skipped_steps"]
        else:
            del older["recipe"]
        os.makedirs(tmp_path / drop / "training_states")
        os.makedirs(tmp_path / drop / "models")
        torch.save(older, tmp_path / drop / "training_states" / "2.state")
        torch.save(torch.load(tmp_path / "a" / "models" / "net_g_2.pth", weights_only=True), tmp_path / drop / "models" / "net_g_2.pth")
        opt3 = copy.deepcopy(opt)
        opt3["path"]["resume_state"] = str(tmp_path / drop / "training_states" / "2.state")
        t3 = recipe.Trainer(opt3, make_store("cpu", TRAIN_SHAPES, 1), out_dir=str(tmp_path / ("c" + drop)), step_fn=_stub_step)
        assert int(t3.guard.skipped) == 0 and t3.current_iter == 2
    # and an unguarded run writes no such key
    plain = recipe.Trainer(small_opt(total_iter=2, save_checkpoint_freq=2), make_store("cpu", TRAIN_SHAPES, 1),
                           out_dir=str(tmp_path / "p"), step_fn=_stub_step)
    plain.run()
    assert "skipped_steps" not in torch.load(tmp_path / "p" / "training_states" / "2.state", weights_only=True)["recipe"]
