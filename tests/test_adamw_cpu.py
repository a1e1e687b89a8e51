"""CPU: the table-driven AdamW step and the weights' moving average without a GPU - cpu_twin.adamw_step and trainer.HipAdamW on CPU
tensors against torch.optim.AdamW bit for bit, the checkpoint format, the average's arithmetic, the skipped step, the reference's
golden optimizer step, wm_adamw_step's host-side refusals, and the recipe with train.ema_decay (options, files, validation on the
averaged weights, exact resume, gloo world 2).  The kernel itself: tests/test_adamw_gpu.py."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import wave_mamba_amd as wm
from wave_mamba_amd import _lib, cpu_twin, ops, recipe, trainer
import adamw_cases as cases
from test_checkpoint import _net_with_golden_grads
from test_ddp_gloo import free_port
from test_recipe_cpu import TRAIN_SHAPES, VAL_SHAPES, make_store, small_opt


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


# ---- 1. the twin and the optimizer class on CPU tensors ----------------------------------------------------------------------------
def _twin_run(steps):
    params = cases.start()
    m, v = [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]
    emas = [p.clone() for p in params]
    for s in range(steps):
        cpu_twin.adamw_step(params, cases.grads(s), m, v, cases.HYPER["lr"], s, cases.HYPER["betas"], cases.HYPER["eps"],
                            cases.HYPER["weight_decay"], emas, cases.EMA_DECAY)
    return {"param": params, "exp_avg": m, "exp_avg_sq": v, "ema": emas}


@pytest.mark.parametrize("foreach", [False, True])
def test_twin_equals_torch_adamw_bit_for_bit(foreach):
    """20 steps over 1 .. 8193 floats with gradients from 1e-6 to 10: parameters and both moments torch.equal to torch.optim.AdamW."""
    twin = _twin_run(cases.STEPS)
    params = [p.clone().requires_grad_() for p in cases.start()]
    opt = torch.optim.AdamW(params, foreach=foreach, **cases.HYPER)
    for s in range(cases.STEPS):
        for p, g in zip(params, cases.grads(s)):
            p.grad = g
        opt.step()
    assert _same(twin["param"], [p.detach() for p in params])
    for k in ("exp_avg", "exp_avg_sq"):
        assert _same(twin[k], [opt.state[p][k] for p in params]), k
    ref = cases.reference()
    assert all(_same(twin[k], ref[k]) for k in cases.KINDS)                  # ... and the shared reference run is that run


def _hip_on_cpu(steps, ema=True, **kw):
    params = [p.clone().requires_grad_() for p in cases.start()]
    opt = trainer.HipAdamW(params, ema_decay=cases.EMA_DECAY if ema else None, **cases.HYPER, **kw)
    for s in range(steps):
        for p, g in zip(params, cases.grads(s)):
            p.grad = g
        opt.step()
    return params, opt


def test_hip_adamw_on_cpu_tensors_is_the_twin_and_the_average_follows_its_formula():
    params, opt = _hip_on_cpu(cases.STEPS)
    twin = _twin_run(cases.STEPS)
    assert _same([p.detach() for p in params], twin["param"])
    assert _same([opt.state[p]["exp_avg"] for p in params], twin["exp_avg"])
    assert _same([opt.state[p]["exp_avg_sq"] for p in params], twin["exp_avg_sq"])
    assert _same(opt._groups[0].e, twin["ema"])
    assert {float(opt.state[p]["step"]) for p in params} == {float(cases.STEPS)}
    # the average by hand, beside three more steps: e.mul_(d).add_(p, alpha=1 - d) on the NEW weights
    emas = [e.clone() for e in opt._groups[0].e]
    for s in range(3):
        for p, g in zip(params, cases.grads(s)):
            p.grad = g
        opt.step()
        for e, p in zip(emas, params):
            e.mul_(cases.EMA_DECAY).add_(p.detach(), alpha=1 - cases.EMA_DECAY)
    assert _same(opt._groups[0].e, emas) and not _same(emas, [p.detach() for p in params])
    # every slot of the arenas starts on a 16-byte boundary
    st = opt._groups[0]
    for views in (st.m, st.v, st.e):
        assert all((t.data_ptr() - views[0].data_ptr()) % 16 == 0 for t in views)


def test_two_param_groups_step_like_torchs():
    """More groups mean one step per group, each with its own lr, counter and arenas - against torch.optim.AdamW with the same groups."""
    def groups(ps):
        return [{"params": ps[:3]}, {"params": ps[3:], "lr": 1e-3, "weight_decay": 0.0}]
    mine, theirs = [p.clone().requires_grad_() for p in cases.start()], [p.clone().requires_grad_() for p in cases.start()]
    a, b = trainer.HipAdamW(groups(mine), **cases.HYPER), torch.optim.AdamW(groups(theirs), **cases.HYPER)
    assert len(a._groups) == 2 and [g["lr"] for g in a.param_groups] == [cases.HYPER["lr"], 1e-3]
    for s in range(3):
        for p, q, g in zip(mine, theirs, cases.grads(s)):
            p.grad, q.grad = g, g.clone()
        a.step()
        b.step()
    assert _same([p.detach() for p in mine], [p.detach() for p in theirs])
    assert _same([a.state[p]["exp_avg_sq"] for p in mine], [b.state[p]["exp_avg_sq"] for p in theirs])
    with pytest.raises(RuntimeError, match="fixed at construction"):
        a.add_param_group({"params": [torch.zeros(2, requires_grad=True)]})


def test_refusals_of_the_class_and_of_make_optimizer():
    p = [torch.zeros(3, requires_grad=True)]
    for kw in ({"amsgrad": True}, {"maximize": True}, {"ema_decay": 1.0}, {"ema_decay": -0.1}, {"betas": (1.0, 0.9)}):
        with pytest.raises(ValueError):
            trainer.HipAdamW(p, **kw)
    net = torch.nn.Linear(2, 2)
    with pytest.raises(ValueError, match="backend"):
        trainer.make_optimizer(net, backend="triton")
    with pytest.raises(ValueError, match="ema_decay"):
        trainer.make_optimizer(net, ema_decay=0.9)
    assert isinstance(trainer.make_optimizer(net, backend="hip", ema_decay=0.9), trainer.HipAdamW)
    assert type(trainer.make_optimizer(net)) is torch.optim.AdamW
    with pytest.raises(RuntimeError, match="ema_decay"):
        trainer.make_optimizer(net, backend="hip").swap_ema()


def test_state_dict_round_trips_through_torch_adamw_and_back():
    """HipAdamW -> torch.optim.AdamW -> HipAdamW: the keys are torch's, and the next step of all three is bit-equal.  Differing
    per-parameter `step` entries are refused; loading copies INTO the arenas."""
    params, opt = _hip_on_cpu(5)
    state = opt.state_dict()
    fresh = torch.optim.AdamW([torch.zeros(2, requires_grad=True)], **cases.HYPER).state_dict()
    assert set(state["param_groups"][0]) == set(fresh["param_groups"][0])
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in state["state"].values()) and len(state["state"]) == len(params)
    assert all(s["step"].data_ptr() != state["state"][0]["step"].data_ptr() for k, s in state["state"].items() if k)   # no aliasing
    p_t = [p.detach().clone().requires_grad_() for p in params]
    o_t = torch.optim.AdamW(p_t, lr=1.0)
    o_t.load_state_dict(state)
    p_h = [p.detach().clone().requires_grad_() for p in params]
    o_h = trainer.HipAdamW(p_h, lr=1.0, ema_decay=cases.EMA_DECAY)
    arenas = [o_h._groups[0].exp_avg.data_ptr(), o_h._groups[0].exp_avg_sq.data_ptr()]
    o_h.load_state_dict(copy.deepcopy(o_t.state_dict()))
    assert arenas == [o_h._groups[0].exp_avg.data_ptr(), o_h._groups[0].exp_avg_sq.data_ptr()]
    assert o_h.state[p_h[3]]["exp_avg"].data_ptr() == o_h._groups[0].m[3].data_ptr()
    assert o_h.param_groups[0]["lr"] == cases.HYPER["lr"] and o_h.param_groups[0]["betas"] == cases.HYPER["betas"]
    for ps, o in ((params, opt), (p_t, o_t), (p_h, o_h)):
        for p, g in zip(ps, cases.grads(5)):
            p.grad = g
        o.step()
    for ps, o in ((p_t, o_t), (p_h, o_h)):
        assert _same([p.detach() for p in ps], [p.detach() for p in params])
        for k in ("exp_avg", "exp_avg_sq", "step"):
            assert _same([o.state[p][k] for p in ps], [opt.state[p][k] for p in params]), k
    bad = copy.deepcopy(o_t.state_dict())
    bad["state"][2]["step"] = torch.tensor(9.0)
    with pytest.raises(ValueError, match="step"):
        o_h.load_state_dict(bad)
    assert "ema" not in state and not any("ema" in s for s in state["state"].values())


def test_average_bookkeeping_in_place():
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Conv2d(4, 2, 1))
    net[2].bias.requires_grad_(False)                                       # a frozen parameter and buffers: from the network
    opt = trainer.make_optimizer(net, backend="hip", ema_decay=0.5)
    for p in net.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    ema = opt.ema_state_dict(net)
    assert set(ema) == set(net.state_dict())
    assert torch.equal(ema["2.bias"], net[2].bias) and torch.equal(ema["1.running_var"], net[1].running_var)
    assert not torch.equal(ema["0.weight"], net[0].weight)
    weights = [p.detach().clone() for p in net.parameters()]
    ptrs = [p.data_ptr() for p in net.parameters()] + [e.data_ptr() for e in opt._groups[0].e]
    opt.swap_ema()
    assert torch.equal(net[0].weight, ema["0.weight"]) and torch.equal(opt._groups[0].e[0], weights[0])
    opt.swap_ema()
    assert _same([p.detach() for p in net.parameters()], weights) and torch.equal(opt.ema_state_dict(net)["0.weight"], ema["0.weight"])
    assert ptrs == [p.data_ptr() for p in net.parameters()] + [e.data_ptr() for e in opt._groups[0].e]
    opt.load_ema({"module.0.weight": torch.full_like(net[0].weight, 2.0)}, net)
    assert float(opt._groups[0].e[0].min()) == 2.0
    opt.reset_ema()
    assert _same(opt._groups[0].e, [p.detach() for p in net.parameters() if p.requires_grad])


def test_skipped_step_leaves_everything_bit_equal():
    """train_step on the CPU with a GradGuard and a HipAdamW: the poisoned step leaves weights, moments, counter and the average
    torch.equal and advances guard.skipped; the next one moves them."""
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(4, 3, 3, padding=1))
    poison = torch.ones(())
    net[2].weight.register_hook(lambda grad: grad * poison)
    opt = trainer.make_optimizer(net, backend="hip", ema_decay=0.9)
    guard = trainer.GradGuard(max_norm=1.0)
    g = torch.Generator().manual_seed(3)
    lq, gt = torch.rand(3, 2, 3, 16, 16, generator=g), torch.rand(3, 2, 3, 16, 16, generator=g)

    def snapshot():
        st = opt._groups[0]
        return [p.detach().clone() for p in net.parameters()] + [st.exp_avg.clone(), st.exp_avg_sq.clone(), st.ema.clone(), st.step.clone()]
    trainer.train_step(net, opt, lq[0], gt[0], guard=guard)
    before = snapshot()
    poison.fill_(float("inf"))
    trainer.train_step(net, opt, lq[1], gt[1], guard=guard)
    assert _same(snapshot(), before) and int(guard.skipped) == 1 and float(opt._groups[0].step) == 1.0
    poison.fill_(1.0)
    trainer.train_step(net, opt, lq[2], gt[2], guard=guard)
    assert not any(torch.equal(a, b) for a, b in zip(snapshot(), before)) and float(opt._groups[0].step) == 2.0


def check_optimizer_arithmetic_hip(device):
    """tests/test_checkpoint.py::check_optimizer_arithmetic with backend="hip": one step on the reference's own gradients against
    the reference's parameters after optimizer_g.step() (tests/golden/train_opt_wf8.npz) - at most 1e-6 relative per tensor."""
    net, g, o = _net_with_golden_grads(device)
    opt = trainer.make_optimizer(net, backend="hip")
    assert isinstance(opt, trainer.HipAdamW) and len(opt.param_groups) == 1
    assert len(opt.param_groups[0]["params"]) == len(list(net.parameters()))
    opt.step()
    worst = 0.0
    for k, p in net.named_parameters():
        ref = torch.from_numpy(o["p1." + k]).double()
        worst = max(worst, float((p.detach().cpu().double() - ref).norm() / ref.norm().clamp_min(1e-30)))
    print(f"HipAdamW on {device} against the reference's optimizer step: worst relative deviation {worst:.3e}")
    assert worst <= 1e-6, f"parameters after the optimizer step deviate by {worst:.3e}"
    return worst


def test_hip_backend_matches_reference_on_reference_gradients():
    check_optimizer_arithmetic_hip("cpu")


# ---- 2. the C ABI, by host arithmetic --------------------------------------------------------------------------------------------
def test_entry_point_refuses_before_any_launch():
    """A negative row count first, then an empty problem is WM_OK whatever else is NULL, then NULL table, hyper, lr or step.  (The
    device pointers are never dereferenced on the host: small integers stand in; hyper is real host memory.)"""
    import ctypes
    lib = _lib.load()
    N, P = None, 4096
    H = (ctypes.c_double * 5)(0.9, 0.99, 1e-8, 1e-3, 0.0)
    assert lib.wm_abi_version() == _lib.ABI_VERSION == 34 and "wm_adamw_step" in _lib.SIGNATURES
    assert lib.wm_adamw_step(N, -1, N, N, N, N, N, N) == _lib.WM_EINVAL
    assert lib.wm_adamw_step(P, -1, P, P, H, N, N, N) == _lib.WM_EINVAL
    assert lib.wm_adamw_step(N, 0, N, N, N, N, N, N) == _lib.WM_OK
    assert lib.wm_adamw_step(N, 3, P, P, H, N, N, N) == _lib.WM_ENULL            # table
    assert lib.wm_adamw_step(P, 3, N, P, H, N, N, N) == _lib.WM_ENULL            # lr
    assert lib.wm_adamw_step(P, 3, P, N, H, N, N, N) == _lib.WM_ENULL            # step
    assert lib.wm_adamw_step(P, 3, P, P, N, N, N, N) == _lib.WM_ENULL            # hyper
    assert lib.wm_adamw_step(P, 1 << 31, P, P, H, N, N, N) == _lib.WM_EUNSUPPORTED
    assert lib.wm_adamw_step(P + 4, 3, P, P, H, N, N, N) == _lib.WM_EALIGN
    assert lib.wm_adamw_step(P, 3, P + 2, P, H, N, N, N) == _lib.WM_EALIGN
    assert lib.wm_adamw_step(P, 3, P, P, H, P + 1, N, N) == _lib.WM_EALIGN
    for i, bad in ((0, 1.0), (1, -0.1), (2, -1e-8), (3, -1.0), (4, 1.0), (0, float("nan"))):
        h = (ctypes.c_double * 5)(0.9, 0.99, 1e-8, 1e-3, 0.0)
        h[i] = bad
        assert lib.wm_adamw_step(P, 3, P, P, h, N, N, N) == _lib.WM_EINVAL, (i, bad)
    assert ops.ADAMW_ROW_WORDS == 6
    with pytest.raises(ValueError, match="CUDA"):
        ops.adamw_table([torch.zeros(4)], [torch.zeros(4)], [torch.zeros(4)], [torch.zeros(4)])


# ---- 3. the recipe ---------------------------------------------------------------------------------------------------------------------
def _ema_opt(decay=0.9, **kw):
    opt = small_opt(**kw)
    opt["train"]["ema_decay"] = decay
    opt["train"]["optim_g"]["backend"] = "hip"
    opt["val"]["metrics"].pop("lpips")
    return opt


def test_options_are_refused_by_key():
    recipe.check_options(_ema_opt())
    assert recipe.optimizer_backend_options(small_opt()) == ("torch", None)
    assert recipe.optimizer_backend_options(_ema_opt(0.999)) == ("hip", 0.999)
    assert recipe.optimizer_backend_options(_ema_opt(0)) == ("hip", None)
    zero_torch = small_opt()
    zero_torch["train"]["ema_decay"] = 0
    assert recipe.optimizer_backend_options(zero_torch) == ("torch", None)
    for decay in (1.0, -0.5, 1.5, "0.9", True, float("nan")):
        with pytest.raises(ValueError, match=r"train\.ema_decay"):
            recipe.check_options(_ema_opt(decay))
    needs = _ema_opt()
    needs["train"]["optim_g"]["backend"] = "torch"
    with pytest.raises(ValueError, match=r"train\.ema_decay.*train\.optim_g\.backend: hip"):
        recipe.check_options(needs)
    del needs["train"]["optim_g"]["backend"]
    with pytest.raises(ValueError, match=r"train\.ema_decay.*train\.optim_g\.backend: hip"):
        recipe.check_options(needs)
    unknown = _ema_opt()
    unknown["train"]["optim_g"]["backend"] = "cuda"
    with pytest.raises(ValueError, match=r"train\.optim_g\.backend"):
        recipe.check_options(unknown)


def _emas(t):
    return [e.clone() for e in t.optimizer._groups[0].e]


@pytest.fixture(scope="module")
def ema_runs(tmp_path_factory):
    """Eager CPU runs of the wf = 8 recipe with train.ema_decay: six iterations straight (saving at 3, validating at the end), and
    a fresh Trainer resumed from iteration 3 that runs the last three."""
    out = tmp_path_factory.mktemp("ema_runs")
    opt = _ema_opt(total_iter=6, print_freq=1000, save_checkpoint_freq=3)
    straight = recipe.Trainer(opt, make_store("cpu", TRAIN_SHAPES * 2, 1), make_store("cpu", VAL_SHAPES[:1], 2), out_dir=str(out / "straight"))
    assert isinstance(straight.optimizer, trainer.HipAdamW) and _same(_emas(straight), [p.detach() for p in straight.net.parameters()])
    straight.run()
    opt2 = copy.deepcopy(opt)
    opt2["path"]["resume_state"] = str(out / "straight" / "training_states" / "3.state")
    resumed = recipe.Trainer(opt2, make_store("cpu", TRAIN_SHAPES * 2, 1), out_dir=str(out / "resumed"))
    at_resume = _emas(resumed)
    resumed.run()
    return out, straight, resumed, at_resume


@pytest.mark.timeout(900)
def test_recipe_with_ema_writes_both_keys_and_loads_the_averaged_weights(ema_runs):
    out, straight, resumed, _ = ema_runs
    for name in ("net_g_3.pth", "net_g_6.pth", "net_g_latest.pth", "net_g_best_6.pth"):
        blob = torch.load(out / "straight" / "models" / name, weights_only=True)
        assert {"params", "params_ema"} <= set(blob) and set(blob["params"]) == set(blob["params_ema"]), name
    a, b = wm.build_network(straight.opt["network_g"]), wm.build_network(straight.opt["network_g"])
    latest = str(out / "straight" / "models" / "net_g_latest.pth")
    assert trainer.load_network(a, latest) == ([], [], []) and trainer.load_network(b, latest, param_key="params_ema") == ([], [], [])
    assert _same([p.detach() for p in a.parameters()], [p.detach() for p in straight.net.parameters()])
    assert _same([p.detach() for p in b.parameters()], _emas(straight))
    assert not any(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()) if p.numel() > 1)
    # without the option the file is what it always was
    plain = recipe.Trainer(small_opt(total_iter=1), make_store("cpu", TRAIN_SHAPES, 1), out_dir=str(out / "plain"), step_fn=lambda lq, gt: {})
    plain.run()
    assert set(torch.load(out / "plain" / "models" / "net_g_latest.pth", weights_only=True)) == {"params", "iter", "epoch"}


@pytest.mark.timeout(900)
def test_validation_scores_the_averaged_weights_and_puts_the_weights_back(ema_runs):
    out, straight, _, _ = ema_runs
    weights, emas = [p.detach().clone() for p in straight.net.parameters()], _emas(straight)
    seen = {}
    real = straight.score

    def spying():
        seen["during"] = [p.detach().clone() for p in straight.net.parameters()]
        return real()
    straight.score = spying
    try:
        results = straight.validate(6, straight.epoch)
    finally:
        straight.score = real
    assert _same(seen["during"], emas), "validation did not score the averaged weights"
    assert _same([p.detach() for p in straight.net.parameters()], weights) and _same(_emas(straight), emas)
    other = wm.build_network(straight.opt["network_g"])
    trainer.load_network(other, str(out / "straight" / "models" / "net_g_latest.pth"), param_key="params_ema")
    scorer = recipe.Trainer(small_opt(), make_store("cpu", TRAIN_SHAPES, 1), make_store("cpu", VAL_SHAPES[:1], 2), net=other,
                            out_dir=str(out / "scorer"), step_fn=lambda lq, gt: {})
    assert scorer.score() == results


@pytest.mark.timeout(900)
def test_resume_continues_the_average_exactly(ema_runs):
    """3 + resume + 3 against 6 straight: the resumed Trainer starts from the file's params_ema, and the averages after iteration 6
    are bit-equal."""
    out, straight, resumed, at_resume = ema_runs
    saved = torch.load(out / "straight" / "models" / "net_g_3.pth", weights_only=True)
    names = [k for k, p in resumed.net.named_parameters() if p.requires_grad]
    assert _same(at_resume, [saved["params_ema"][k] for k in names])
    assert not _same(at_resume, [saved["params"][k] for k in names])
    assert resumed.current_iter == 6 and float(resumed.optimizer._groups[0].step) == 6.0
    assert _same([p.detach() for p in resumed.net.parameters()], [p.detach() for p in straight.net.parameters()])
    assert _same(_emas(resumed), _emas(straight))


def _gloo_worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(4)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        opt = _ema_opt(total_iter=3, print_freq=1000)
        t = recipe.Trainer(opt, make_store("cpu", TRAIN_SHAPES, 1), out_dir=os.path.join(out_dir, f"rank{rank}"))
        start = _emas(t)
        t.run()
        torch.save({"start": start, "ema": _emas(t), "w": [p.detach().clone() for p in t.net.parameters()],
                    "kind": (t.distributed, type(t._gstep).__name__, type(t.optimizer).__name__)}, os.path.join(out_dir, f"ema{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_gloo_world_two_holds_equal_averages(tmp_path):
    mp.spawn(_gloo_worker, args=(2, free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"ema{r}.pt") for r in range(2))
    assert r0["kind"] == r1["kind"] == (True, "GraphedDDPTrainStep", "HipAdamW")
    assert _same(r0["start"], r1["start"]), "the averages did not start from rank 0's broadcast weights"
    assert _same(r0["w"], r1["w"]) and _same(r0["ema"], r1["ema"])
    assert not _same(r0["ema"], r0["w"]) and not _same(r0["ema"], r0["start"])
    blob = torch.load(tmp_path / "rank0" / "models" / "net_g_latest.pth", weights_only=True)
    assert "params_ema" in blob and not os.path.exists(tmp_path / "rank1" / "models")
