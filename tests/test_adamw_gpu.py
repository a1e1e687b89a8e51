"""GPU: the table-driven AdamW step with the weights' moving average - wm_adamw_step against a float64 evaluation, held to torch's
own CPU error on the cases of tests/adamw_cases.py (aligned rows and gradient views one float off a 16-byte boundary, rows with and
without an average, an empty tensor, an empty table), the guard's two device scalars, the reference's golden optimizer step, and
whole captured steps: GraphedTrainStep and GraphedDDPTrainStep with trainer.HipAdamW against eager train_steps."""
import os
import socket
from datetime import timedelta

import pytest
import torch

import wave_mamba_amd as wm
from wave_mamba_amd import ops, schedulers, trainer
import adamw_cases as cases
from grad_guard_cases import at_offset
from test_adamw_cpu import check_optimizer_arithmetic_hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL = dict(in_chn=3, wf=8, n_l_blocks=[1, 1, 1], n_h_blocks=[1, 1, 1], ffn_scale=2.0)       # tests/test_deterministic_gpu.py
HAS_EMA = [i % 3 != 0 for i in range(len(cases.SIZES))]         # rows with an ema address and rows with 0 in one table
LAYOUTS = {"aligned": 0, "grad_off_one": 1}                     # floats between a gradient's start and a 16-byte boundary
N_ROWS = sum(-(-n // cases.CHUNK) for n in cases.SIZES)


class _Set:
    """The case's tensors on the device - with an empty tensor at the end, which gives no row - and one table over them."""

    def __init__(self, layout, state=None, first=0, found_inf=None, grad_scale=None):
        off = LAYOUTS[layout]
        state = state or {"param": cases.start(), "exp_avg": [torch.zeros(n) for n in cases.SIZES],
                          "exp_avg_sq": [torch.zeros(n) for n in cases.SIZES], "ema": cases.start()}
        empty = [torch.zeros(0)]
        self.p = [at_offset(t.float(), 0, DEV) for t in state["param"] + empty]
        self.g = [at_offset(torch.zeros(n), off, DEV) for n in cases.SIZES + [0]]
        self.m = [at_offset(t.float(), 0, DEV) for t in state["exp_avg"] + empty]
        self.v = [at_offset(t.float(), 0, DEV) for t in state["exp_avg_sq"] + empty]
        self.e = [at_offset(t.float(), 0, DEV) if has else None for t, has in zip(state["ema"] + empty, HAS_EMA + [True])]
        assert all(g.data_ptr() % 16 == 4 * off for g in self.g[:-1])
        self.table = ops.adamw_table(self.p, self.g, self.m, self.v, self.e)
        assert self.table[1] == N_ROWS and tuple(self.table[0].shape) == (N_ROWS, ops.ADAMW_ROW_WORDS)
        self.lr = torch.tensor(cases.HYPER["lr"], dtype=torch.float32, device=DEV)
        self.step = torch.tensor([float(first)], dtype=torch.float32, device=DEV)
        self.found_inf = None if found_inf is None else torch.tensor([found_inf], dtype=torch.float32, device=DEV)
        self.grad_scale = None if grad_scale is None else torch.tensor([grad_scale], dtype=torch.float32, device=DEV)
        self.first = first

    def run(self, steps):
        for s in range(self.first, self.first + steps):
            for dst, src in zip(self.g, cases.grads(s)):
                dst.copy_(src)
            ops.adamw_step(self.table, self.lr, self.step, cases.HYPER["betas"], cases.HYPER["eps"], cases.HYPER["weight_decay"],
                           cases.EMA_DECAY, self.found_inf, self.grad_scale)
        torch.cuda.synchronize()
        return self.result()

    def result(self):
        n = len(cases.SIZES)
        return {"param": [t.cpu() for t in self.p[:n]], "exp_avg": [t.cpu() for t in self.m[:n]],
                "exp_avg_sq": [t.cpu() for t in self.v[:n]], "ema": [t.cpu() for t, has in zip(self.e[:n], HAS_EMA) if has]}


def _with_ema_rows(run):
    """A reference run's averages, for the rows of _Set that keep one."""
    return {**run, "ema": [t for t, has in zip(run["ema"], HAS_EMA) if has]}


def _bits(tensors):
    return [t.clone().view(torch.int32) for t in tensors if t is not None]


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_twenty_steps_hold_torchs_own_error_against_float64(layout):
    """20 steps from one fp32 start, gradients from 1e-6 to 10, tensors of 1 .. 8193 floats: per tensor max |x - f64| / max |f64|,
    the worst per kind at most twice the same figure of torch's CPU AdamW (what the reference runs).
    Measured pairs (kernel, torch): profiles/adamw/README.md."""
    got = _Set(layout).run(cases.STEPS)
    f64 = _with_ema_rows(cases.reference(f64=True))
    ref = _with_ema_rows(cases.reference())
    assert cases.within_twice(cases.errors(got, f64), cases.errors(ref, f64), f"{layout}, 20 steps, ")
    same = {k: sum(torch.equal(a, b) for a, b in zip(got[k], ref[k])) for k in cases.KINDS}
    print(f"{layout}: tensors bit-equal to torch's CPU run, of {len(cases.SIZES)} ({sum(HAS_EMA)} averages): {same}")


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_one_step_from_a_mid_run_state_and_the_counter(layout):
    """One step at t = 7 from the fp32 state torch's run has after six, under the same bar; the counter goes from 6 to 7."""
    state = cases.reference(6)
    run = _Set(layout, state=state, first=6)
    got = run.run(1)
    f64 = _with_ema_rows(cases.torch_run(1, torch.float64, state=state, first=6))
    ref = _with_ema_rows(cases.torch_run(1, torch.float32, state=state, first=6))
    assert cases.within_twice(cases.errors(got, f64), cases.errors(ref, f64), f"{layout}, t = 7, ")
    assert float(run.step) == 7.0


def test_difference_to_torchs_fused_gpu_adamw_is_reported():
    """The same 20 steps through torch.optim.AdamW(fused=True) on the device: the worst difference per kind is printed, not
    judged - both are held to float64 (torch's fused kernel here, for the record)."""
    got = _Set("aligned").run(cases.STEPS)
    params = [p.to(DEV).requires_grad_() for p in cases.start()]
    opt = torch.optim.AdamW(params, fused=True, **cases.HYPER)
    for s in range(cases.STEPS):
        for p, g in zip(params, cases.grads(s)):
            p.grad = g.to(DEV)
        opt.step()
    fused = {"param": [p.detach().cpu() for p in params], "exp_avg": [opt.state[p]["exp_avg"].cpu() for p in params],
             "exp_avg_sq": [opt.state[p]["exp_avg_sq"].cpu() for p in params]}
    f64 = cases.reference(f64=True)
    for k in fused:
        print(f"{k}: kernel against torch's fused GPU AdamW {cases.error(got[k], [t.double() for t in fused[k]]):.3e}; "
              f"fused against float64 {cases.error(fused[k], f64[k]):.3e}, kernel against float64 {cases.error(got[k], f64[k]):.3e}")


def test_found_inf_leaves_all_five_buffers_and_the_counter_bit_equal():
    for layout in LAYOUTS:
        run = _Set(layout, found_inf=0.0)
        run.run(2)
        before = [_bits(ts) for ts in (run.p, run.g, run.m, run.v, run.e)] + [run.step.clone()]
        run.found_inf.fill_(1.0)
        run.first = 2
        for dst, src in zip(run.g, cases.grads(2)):
            dst.copy_(src)
        before[1] = _bits(run.g)
        ops.adamw_step(run.table, run.lr, run.step, cases.HYPER["betas"], cases.HYPER["eps"], cases.HYPER["weight_decay"],
                       cases.EMA_DECAY, run.found_inf, None)
        torch.cuda.synchronize()
        after = [_bits(ts) for ts in (run.p, run.g, run.m, run.v, run.e)] + [run.step.clone()]
        assert all(torch.equal(a, b) for x, y in zip(before[:5], after[:5]) for a, b in zip(x, y)), layout
        assert torch.equal(before[5], after[5]) and float(run.step) == 2.0
        run.found_inf.fill_(0.0)
        run.run(1)                                                   # ... and with the flag down the same launch steps again
        assert float(run.step) == 3.0 and not torch.equal(_bits(run.p)[-2], before[0][-2])


def test_grad_scale_divides_inside_the_kernel_and_leaves_the_gradients():
    """grad_scale = 2.5 against torch's step on pre-divided gradients, under the bar; the gradient buffers keep their bits."""
    state = cases.reference(6)
    for layout in LAYOUTS:
        run = _Set(layout, state=state, first=6, grad_scale=2.5)
        got = run.run(1)
        f64 = _with_ema_rows(cases.torch_run(1, torch.float64, state=state, first=6, divide=2.5))
        ref = _with_ema_rows(cases.torch_run(1, torch.float32, state=state, first=6, divide=2.5))
        assert cases.within_twice(cases.errors(got, f64), cases.errors(ref, f64), f"{layout}, grad_scale 2.5, ")
        assert all(torch.equal(g.cpu(), want) for g, want in zip(run.g, cases.grads(6)))
        plain = _with_ema_rows(cases.torch_run(1, torch.float32, state=state, first=6))
        assert cases.error(got["exp_avg"], [t.double() for t in plain["exp_avg"]]) > 1e-3      # (the division did happen)


def test_a_table_of_no_rows_is_a_no_op():
    table = ops.adamw_table([], [], [], [])
    assert table[1] == 0 and tuple(table[0].shape) == (0, ops.ADAMW_ROW_WORDS)
    only_empty = ops.adamw_table(*[[torch.zeros(0, device=DEV)] for _ in range(4)])
    assert only_empty[1] == 0
    lr, step = torch.tensor(1e-3, device=DEV), torch.zeros(1, device=DEV)
    ops.adamw_step(table, lr, step, (0.9, 0.99), 1e-8, 1e-3)
    assert float(step) == 0.0
    with pytest.raises(ValueError, match="float32"):
        ops.adamw_step(table, lr.double(), step, (0.9, 0.99), 1e-8, 1e-3)
    with pytest.raises(ValueError, match="another size"):
        ops.adamw_table([torch.zeros(4, device=DEV)], [torch.zeros(5, device=DEV)], [torch.zeros(4, device=DEV)], [torch.zeros(4, device=DEV)])


def test_hip_backend_matches_reference_on_reference_gradients_on_the_gpu():
    check_optimizer_arithmetic_hip(DEV)


def test_eager_table_follows_the_gradients_and_state_moves_between_backends():
    """HipAdamW eagerly on the device: the table is rebuilt when a gradient moved; its state loads into torch's fused AdamW and
    back, and the next step of both agrees under the accuracy bar's metric (1e-6: two fp32 implementations of one step)."""
    params = [p.to(DEV).requires_grad_() for p in cases.start()]
    opt = trainer.HipAdamW(params, ema_decay=cases.EMA_DECAY, **cases.HYPER)
    assert opt.param_groups[0]["lr"].is_cuda and opt.param_groups[0]["capturable"]
    for s in range(3):
        for p, g in zip(params, cases.grads(s)):
            p.grad = g.to(DEV)                                       # fresh tensors: new addresses
        opt.step()
    ref = cases.reference(3)
    assert cases.error([p.detach() for p in params], [t.double() for t in ref["param"]]) <= 1e-6
    assert cases.error(opt._groups[0].e, [t.double() for t in ref["ema"]]) <= 1e-6 and float(opt._groups[0].step) == 3.0
    twin_params = [p.detach().clone().requires_grad_() for p in params]
    fused = torch.optim.AdamW(twin_params, fused=True, capturable=True, lr=torch.tensor(1.0, device=DEV))
    fused.load_state_dict(opt.state_dict())
    back = trainer.HipAdamW([p.detach().clone().requires_grad_() for p in params], lr=1.0)
    back.load_state_dict(fused.state_dict())
    assert float(back.param_groups[0]["lr"]) == float(torch.tensor(cases.HYPER["lr"], dtype=torch.float32))
    for o in (opt, fused, back):
        for p, g in zip(o.param_groups[0]["params"], cases.grads(3)):
            p.grad = g.to(DEV)
        o.step()
    mine = [p.detach() for p in params]
    assert all(torch.equal(a, b.detach()) for a, b in zip(mine, back.param_groups[0]["params"]))
    assert cases.error(mine, [p.detach().cpu().double() for p in twin_params]) <= 1e-6


# ---- whole captured steps ------------------------------------------------------------------------------------------------------------
def _batches():
    g = torch.Generator().manual_seed(11)
    return torch.rand(3, 2, 3, 64, 64, generator=g).to(DEV), torch.rand(3, 2, 3, 64, 64, generator=g).to(DEV)


class _Step:
    """The wf = 8 network from seed 0 with a HipAdamW that keeps an average, and a GradGuard(max_norm=1.0).  kind: "eager"
    (train_step), "single" (GraphedTrainStep), "split" / "captured" (GraphedDDPTrainStep over a one-rank group), "ddp_eager"
    (its capture=False form).  A constructor's warm-up is undone: every run starts from the same weights, zero moments, the
    counter at 0 and the average at the weights."""

    def __init__(self, kind, lq, gt, guarded=True):
        torch.manual_seed(0)
        self.kind = kind
        self.net = wm.WaveMamba(**SMALL).train().to(DEV)
        self.opt = trainer.make_optimizer(self.net, backend="hip", ema_decay=0.9)
        self.guard = trainer.GradGuard(max_norm=1.0) if guarded else None
        start = [p.detach().clone() for p in self.net.parameters()]
        if kind == "single":
            self.step = trainer.GraphedTrainStep(self.net, self.opt, lq, gt, guard=self.guard)
        elif kind != "eager":
            self.step = trainer.GraphedDDPTrainStep(self.net, self.opt, lq, gt, guard=self.guard, capture=kind != "ddp_eager",
                                                    collective="captured" if kind == "captured" else "split")
        st = self.opt._groups[0]
        with torch.no_grad():
            for p, s0 in zip(self.net.parameters(), start):
                p.copy_(s0)
            for t in (st.exp_avg, st.exp_avg_sq, st.step):
                t.zero_()
        self.opt.reset_ema()
        if self.guard is not None:
            self.guard.attach(self.opt).set_skipped(0)

    def eager(self, lq, gt):
        trainer.train_step(self.net, self.opt, lq, gt, as_float=False, guard=self.guard)
        return self.state()

    def __call__(self, lq, gt):
        if self.kind == "eager":
            return self.eager(lq, gt)
        self.step(lq, gt)
        return self.state()

    def state(self):
        torch.cuda.synchronize()
        st = self.opt._groups[0]
        return [p.detach().cpu() for p in self.net.parameters()] + [t.cpu().clone() for t in (st.exp_avg, st.exp_avg_sq, st.ema, st.step)]


def _worst(a, b):
    return max(float((x.double() - y.double()).abs().max() / y.double().abs().max().clamp_min(1e-30)) for x, y in zip(a, b))


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _three(kind):
    lq, gt = _batches()
    run = _Step(kind, lq[0], gt[0])
    return [run(lq[i], gt[i]) for i in range(3)], run


@pytest.fixture(scope="module")
def single():
    """Everything the single-process captured-step tests need, computed once under the deterministic mode."""
    prev = wm.set_deterministic(True)
    try:
        lq, gt = _batches()
        out = {"eager": _three("eager")[0]}
        out["graph"], run = _three("single")
        out["graph_again"] = _three("single")[0]
        out["skipped_before"] = int(run.guard.skipped)
        # a scheduler's fill_ between replays: at lr = 0 a replay moves the moments and leaves every weight as it is
        schedulers.set_lr(run.opt, [0.0])
        out["lr0"] = run(lq[0], gt[0])
        schedulers.set_lr(run.opt, [5e-4])
        # an injected NaN batch
        out["nan"] = run(torch.full_like(lq[1], float("nan")), gt[1])
        out["nan_record"], out["nan_skipped"] = run.guard.record.tolist(), int(run.guard.skipped)
        # eager work on the same network and optimizer between replays (its gradients live elsewhere: another table)
        mixed = _Step("single", lq[0], gt[0])
        out["mixed"] = [mixed(lq[0], gt[0]), mixed.eager(lq[1], gt[1]), mixed(lq[2], gt[2])]
        out["aligned_views"] = all(p.grad.data_ptr() % 16 == 0 for p in run.net.parameters())
        # without a guard: the captured step still steps on its flat buffer (the table needs addresses before the capture)
        bare_eager, bare_graph = _Step("eager", lq[0], gt[0], guarded=False), _Step("single", lq[0], gt[0], guarded=False)
        out["bare"] = [[r(lq[i], gt[i]) for i in range(2)] for r in (bare_eager, bare_graph)]
        out["bare_flat"] = hasattr(bare_graph.step, "flat") and bare_graph.step.guard is None
    finally:
        wm.set_deterministic(prev)
    return out


@pytest.mark.timeout(600)
def test_three_replays_equal_three_eager_steps(single):
    """GraphedTrainStep with a HipAdamW, the average and a GradGuard(max_norm=1.0) against train_step from the same state.  The bar:
    in the deterministic mode the gradients of a replay are the eager step's bit for bit, and both sides run the same elementwise
    kernel on them (16-byte rows either way), so weights, moments, average and counter are torch.equal."""
    for s in range(3):
        print(f"step {s + 1}: worst relative difference replay / eager {_worst(single['graph'][s], single['eager'][s]):.3e}")
    for s in range(3):
        assert _equal(single["graph"][s], single["eager"][s]), f"step {s + 1}"
    assert float(single["graph"][2][-1]) == 3.0 and not _equal(single["graph"][0][:-1], single["graph"][1][:-1])
    assert not torch.equal(single["graph"][2][-2], single["graph"][1][-2]) and single["aligned_views"]     # the average moves too


@pytest.mark.timeout(600)
def test_captured_step_without_a_guard_equals_the_eager_one(single):
    eager, graph = single["bare"]
    assert single["bare_flat"] and all(_equal(a, b) for a, b in zip(eager, graph)) and float(graph[1][-1]) == 2.0


@pytest.mark.timeout(600)
def test_two_graphs_from_one_state_agree_bit_for_bit(single):
    for s in range(3):
        assert _equal(single["graph"][s], single["graph_again"][s]), f"step {s + 1}"


@pytest.mark.timeout(600)
def test_a_scheduler_fill_reaches_the_replayed_update(single):
    before, after = single["graph"][2], single["lr0"]
    n = len(before) - 4
    assert _equal(before[:n], after[:n]), "a replay at lr = 0 moved a weight: the captured launch did not read the lr tensor"
    assert not torch.equal(before[n], after[n]) and float(after[-1]) == 4.0


@pytest.mark.timeout(600)
def test_a_nan_batch_is_skipped_with_the_average_untouched(single):
    assert _equal(single["nan"], single["lr0"]), "the skipped replay moved a weight, a moment, the average or the counter"
    assert single["nan_record"][1] == 1.0 and single["nan_skipped"] == single["skipped_before"] + 1


@pytest.mark.timeout(600)
def test_eager_work_between_replays_does_no_harm(single):
    for s in range(3):
        assert _equal(single["mixed"][s], single["eager"][s]), f"step {s + 1}"


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
        out = {}
        for kind in ("ddp_eager", "split", "captured"):
            out[kind], run = _three(kind)
            out[kind + "_unaligned"] = sum(v.data_ptr() % 16 != 0 for v in run.step.views)
        torch.save(out, os.path.join(out_dir, "ddp.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_ddp_step_over_one_rank_runs_the_unaligned_rows(single, tmp_path):
    """GraphedDDPTrainStep with the backend, both collective modes, against its eager form and the single-process eager steps: its
    packed gradient views mostly start off a 16-byte boundary, and an elementwise update does not depend on the access width."""
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_ddp_worker, args=(port, str(tmp_path)), nprocs=1, join=True)
    r = torch.load(tmp_path / "ddp.pt", weights_only=False)
    for kind in ("split", "captured"):
        assert r[kind + "_unaligned"] > 0
        for s in range(3):
            print(f"{kind}, step {s + 1}: worst relative difference to the single-process eager step "
                  f"{_worst(r[kind][s], single['eager'][s]):.3e}")
            assert _equal(r[kind][s], r["ddp_eager"][s]), f"{kind}, step {s + 1}"
        assert float(r[kind][2][-1]) == 3.0


# ---- the recipe ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
def test_recipe_trains_validates_saves_and_resumes_with_the_average(tmp_path):
    """recipe.Trainer, graphed, train.ema_decay with backend hip: the constructor's warm-up leaves no trace in the average, the
    files carry params and params_ema, validation scores the averaged weights and puts the weights back, and a run resumed from
    iteration 3 ends on the uninterrupted run's weights and average bit for bit (deterministic mode)."""
    import copy
    from wave_mamba_amd import recipe
    from test_recipe_cpu import TRAIN_SHAPES, VAL_SHAPES, make_store, small_opt
    prev = wm.set_deterministic(True)
    try:
        opt = small_opt(total_iter=6, print_freq=1000, save_checkpoint_freq=3)
        opt["train"]["ema_decay"] = 0.9
        opt["train"]["optim_g"]["backend"] = "hip"
        opt["val"]["metrics"].pop("lpips")
        runs = {}
        for name in ("whole", "resumed"):
            if name == "resumed":
                opt = copy.deepcopy(opt)
                opt["path"]["resume_state"] = str(tmp_path / "whole" / "training_states" / "3.state")
            t = recipe.Trainer(opt, make_store(DEV, TRAIN_SHAPES * 2, 1), make_store(DEV, VAL_SHAPES[:1], 2), graphed=True,
                               out_dir=str(tmp_path / name))
            start = ([p.detach().clone() for p in t.net.parameters()], [e.clone() for e in t.optimizer._groups[0].e])
            first = []
            t.run(max_iters=1, on_iter=lambda it, epoch, lrs, rows, losses: first.append(
                ([p.detach().clone() for p in t.net.parameters()], [e.clone() for e in t.optimizer._groups[0].e])))
            result = t.run()
            assert isinstance(t._gstep, trainer.GraphedTrainStep) and isinstance(t.optimizer, trainer.HipAdamW)
            runs[name] = (t, start, first[0], result)
    finally:
        wm.set_deterministic(prev)
    t, start, first, result = runs["whole"]
    d = 0.9
    assert _equal(start[0], start[1])                                    # the average starts at the weights
    # ... and the first iteration is ONE step from there: d e0 + (1 - d) p1 in float64, to the kernel's two roundings (2^-23)
    d32, omd32 = float(torch.tensor(d, dtype=torch.float32)), float(torch.tensor(1 - d, dtype=torch.float32))   # the kernel's scalars
    want = [e0.cpu().double() * d32 + omd32 * p1.cpu().double() for e0, p1 in zip(start[1], first[0])]
    assert cases.error(first[1], want) <= 2.0 ** -23 and not _equal(first[0], start[0])
    assert float(t.optimizer._groups[0].step) == 6.0 and set(result["validation"]) == {"psnr", "ssim"}
    weights, emas = [p.detach().clone() for p in t.net.parameters()], [e.clone() for e in t.optimizer._groups[0].e]
    for name in ("net_g_3.pth", "net_g_latest.pth", "net_g_best_6.pth"):
        blob = torch.load(tmp_path / "whole" / "models" / name, weights_only=True)
        assert {"params", "params_ema"} <= set(blob), name
    averaged = wm.build_network(t.opt["network_g"]).to(DEV)
    trainer.load_network(averaged, str(tmp_path / "whole" / "models" / "net_g_latest.pth"), param_key="params_ema")
    assert _equal([p.detach() for p in averaged.parameters()], emas) and not _equal(emas, weights)
    scorer = recipe.Trainer(small_opt(), make_store(DEV, TRAIN_SHAPES, 1), make_store(DEV, VAL_SHAPES[:1], 2), net=averaged,
                            graphed=False, out_dir=str(tmp_path / "scorer"), step_fn=lambda lq, gt: {})
    scorer.metrics, scorer.val_freq = t.metrics, t.val_freq
    assert scorer.score() == result["validation"], "validation did not score the averaged weights"
    assert _equal([p.detach() for p in t.net.parameters()], weights)     # (score() of the other trainer touched nothing here)
    t2 = runs["resumed"][0]
    assert t2.current_iter == 6 and float(t2.optimizer._groups[0].step) == 6.0
    assert _equal([p.detach() for p in t2.net.parameters()], weights), "the resumed run's weights differ"
    assert _equal([e for e in t2.optimizer._groups[0].e], emas), "the resumed run's average differs"
