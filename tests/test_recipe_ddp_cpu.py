"""CPU, world 2 over gloo: recipe.Trainer in its distributed mode (trainer.GraphedDDPTrainStep in its eager form under the recipe's
loop) - lock step with the DistributedDataParallel loop, files on rank 0 only, sharded validation, exact resume, the refusals, the
step's `fft_weight` and the command line.  The settings of test_recipe_cpu.py: wf = 8, crops of 64, batch 3, CPU stores.  The two
workers are spawned once per module and save what the tests read."""
import contextlib
import copy
import io
import json
import os
import socket
from datetime import timedelta

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from wave_mamba_amd import recipe, schedulers, trainer
from wave_mamba_amd.data import PairedPatchBatcher
from test_recipe_cpu import TRAIN_SHAPES, VAL_SHAPES, make_store, small_opt

WORLD = 2
VAL3 = VAL_SHAPES + [(64, 80)]                   # three pairs over two ranks: uneven shards
CLI_ITERS = 2
F32 = 2.0 ** -24                                 # half a unit in the last place of a float32, relative


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def _weights(net):
    return [p.detach().clone() for p in net.parameters()]


def _loop_opt():
    return small_opt(total_iter=4, print_freq=2, save_checkpoint_freq=3)


def _resume_opt(total_iter=6):
    return small_opt(total_iter=total_iter, print_freq=1000)


class Seen:
    """What on_iter saw, per iteration: (iter, epoch), lrs, rows, the step's losses as floats, a copy of every weight."""

    def __init__(self, t):
        self.t, self.iters, self.lrs, self.rows, self.losses, self.weights = t, [], [], [], [], []

    def __call__(self, it, epoch, lrs, rows, losses):
        self.iters.append((it, epoch))
        self.lrs.append(lrs)
        self.rows.append(rows)
        self.losses.append({k: float(v) for k, v in losses.items()})
        self.weights.append(_weights(self.t.net))

    def record(self):
        return {"iters": self.iters, "lrs": self.lrs, "rows": self.rows, "losses": self.losses, "weights": self.weights}


def _hand_loop(rank, opt, store, iters):
    """The reference's loop under DistributedDataParallel, from the seeds Trainer uses: wrap_ddp + train_step, the sampler's shard of
    this rank, the batcher seeded seed + rank, the recipe's scheduler.  Also this rank's OWN l_pix of every iteration (a no_grad
    forward before the step) beside the reduced one train_step returns."""
    seed, tr = opt["manual_seed"], opt["train"]
    torch.manual_seed(seed + rank)
    net = recipe.build_network(opt["network_g"]).train()
    ddp = trainer.wrap_ddp(net)
    assert isinstance(ddp, torch.nn.parallel.DistributedDataParallel)
    optim = trainer.make_optimizer(ddp, lr=tr["optim_g"]["lr"], weight_decay=tr["optim_g"]["weight_decay"],
                                   betas=tuple(tr["optim_g"]["betas"]))
    schedulers.set_lr(optim, [tr["optim_g"]["lr"]])
    sched = schedulers.build_scheduler(optim, tr["scheduler"])
    sampler = recipe.EnlargedSampler(len(store), WORLD, rank)
    batcher = PairedPatchBatcher(store, gt_size=64, geometric_augs=True, seed=seed + rank)
    out = {"weights": [], "rows": [], "own_l_pix": [], "reduced": []}
    it, epoch = 0, 0
    while it < iters:
        sampler.set_epoch(epoch)
        for idx in sampler.batches(3):
            if it == iters:
                break
            it += 1
            schedulers.update_learning_rate([sched], [optim], it, -1)
            rows = batcher.draw(idx)
            lq, gt = batcher.form(rows=rows)
            with torch.no_grad():
                out["own_l_pix"].append(trainer.losses(net(lq), gt, fft_weight=0.1, ssim_weight=0.25)[0].clone())
            red = trainer.train_step(ddp, optim, lq, gt, as_float=False, ssim_weight=0.25, fft_weight=0.1)
            out["reduced"].append({k: float(v) for k, v in red.items()})      # the mean over ranks on rank 0 (reduce_loss_dict)
            out["rows"].append(rows)
            out["weights"].append(_weights(net))
        epoch += 1
    return out


def _worker(rank, world, ports, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    torch.set_num_threads(4)
    mine = os.path.join(out_dir, f"rank{rank}")
    res = {}

    # ---- the command line: main() creates and destroys its own group ----
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(ports[0]), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        code = recipe.main(["-opt", os.path.join(out_dir, "cli.yml"), "--train-pairs", os.path.join(out_dir, "pairs", "train"),
                            "--val-pairs", os.path.join(out_dir, "pairs", "val"), "--device", "cpu", "--dist-backend", "gloo",
                            "--out-dir", os.path.join(mine, "cli"), "--dist-timeout", "120"])
    res["cli"] = {"code": code, "stdout": text.getvalue(), "group_left": dist.is_initialized()}

    os.environ["MASTER_PORT"] = str(ports[1])
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
    try:
        store = make_store("cpu", TRAIN_SHAPES, 1)

        # ---- refusal against the group ----
        for name, kw in (("world", {"world": 3}), ("rank", {"rank": 1 - rank})):
            try:
                recipe.Trainer(_loop_opt(), store, out_dir=os.path.join(mine, "refused"), **kw)
                res[f"refused_{name}"] = None
            except ValueError as e:
                res[f"refused_{name}"] = str(e)

        # ---- four iterations of Trainer, and of the DistributedDataParallel loop ----
        t = recipe.Trainer(_loop_opt(), store, out_dir=os.path.join(mine, "loop"))
        seen = Seen(t)
        res["loop_mode"] = (t.distributed, t.rank, t.world, type(t._gstep).__name__)
        res["loop_result"] = t.run(on_iter=seen)
        res["loop"] = seen.record()
        res["loop_step"] = (type(t._gstep).__name__, t._gstep.capture)
        res["loop_adam_steps"] = sorted({float(st["step"]) for st in t.optimizer.state.values()})
        res["hand"] = _hand_loop(rank, _loop_opt(), store, 4)

        # ---- sharded validation on the trained weights, against the single-process score() of the same network ----
        res["val"] = {}
        for name, shapes in (("three", VAL3), ("one", VAL_SHAPES[:1])):
            val = make_store("cpu", shapes, 2)
            sharded = recipe.Trainer(_loop_opt(), store, val, out_dir=os.path.join(mine, "val"), net=t.net)
            single = recipe.Trainer(_loop_opt(), store, val, out_dir=os.path.join(mine, "val"), net=t.net, distributed=False)
            assert sharded.distributed and not single.distributed and sharded.net is single.net
            res["val"][name] = {"sharded": sharded.score(), "single": single.score()}

        # ---- exact resume: two batches per epoch and rank; 6 iterations straight, and 3 + save + 3 ----
        big = make_store("cpu", TRAIN_SHAPES * 2, 1)
        straight = recipe.Trainer(_resume_opt(), big, out_dir=os.path.join(mine, "straight"))
        s_seen = Seen(straight)
        straight.run(on_iter=s_seen)
        res["straight"] = s_seen.record()
        first = recipe.Trainer(_resume_opt(), big, out_dir=os.path.join(mine, "first"))
        first.run(max_iters=3)
        res["saved_at"] = (first.current_iter, first.epoch, first._pos)
        res["saved_rng"] = first.batcher.rng.getstate()
        first.save(first.epoch, first.current_iter)                  # a collective: both ranks call it, rank 0 writes
        dist.barrier()
        opt2 = _resume_opt()
        opt2["path"]["resume_state"] = os.path.join(out_dir, "rank0", "first", "training_states", "3.state")
        second = recipe.Trainer(opt2, big, out_dir=os.path.join(mine, "second"))
        res["resumed_at"] = (second.current_iter, second.epoch, second._pos)
        r_seen = Seen(second)
        second.run(on_iter=r_seen)
        res["resumed"] = r_seen.record()

        # ---- fft_weight of the data-parallel step: one step each from the same weights on the same batch ----
        lq, gt = PairedPatchBatcher(store, gt_size=64, seed=5 + rank).form([0, 1, 2])
        res["l_freq"] = {}
        for name, kw in (("default", {}), ("0.3", {"fft_weight": 0.3})):
            torch.manual_seed(0)
            net = recipe.build_network(_loop_opt()["network_g"]).train()
            step = trainer.GraphedDDPTrainStep(net, trainer.make_optimizer(net), lq, gt, capture=False, ssim_weight=0.25, **kw)
            res["l_freq"][name] = step()["l_freq"].clone()
        res["files"] = _files(mine)
        torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    import yaml
    out = tmp_path_factory.mktemp("recipe_ddp")
    for name, store in (("train", make_store("cpu", TRAIN_SHAPES, 1)), ("val", make_store("cpu", VAL_SHAPES[:1], 2))):
        for kind in ("lq", "gt"):
            os.makedirs(out / "pairs" / name / kind)
        for i in range(len(store)):
            lq, gt = store.pair(i)
            np.save(out / "pairs" / name / "lq" / f"{i:03d}.npy", lq.numpy())
            np.save(out / "pairs" / name / "gt" / f"{i:03d}.npy", gt.numpy())
    cli_opt = small_opt(total_iter=CLI_ITERS, print_freq=1, save_checkpoint_freq=2)
    cli_opt["val"]["metrics"].pop("lpips")
    with open(out / "cli.yml", "w", encoding="utf-8") as f:
        yaml.safe_dump(cli_opt, f)
    mp.spawn(_worker, args=(WORLD, (free_port(), free_port()), str(out)), nprocs=WORLD, join=True)
    return out, [torch.load(out / f"rank{r}.pt", weights_only=False) for r in range(WORLD)]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.timeout(900)
def test_trainer_equals_the_ddp_loop(ranks):
    """After every one of 4 iterations all weights are torch.equal: rank 0 to rank 1, and Trainer to the loop written around
    DistributedDataParallel + train_step from the same seeds.  (Without a gradient exchange the ranks part at iteration 1.)"""
    out, res = ranks
    for r in range(WORLD):
        assert res[r]["loop_mode"] == (True, r, WORLD, "NoneType") and res[r]["loop_step"] == ("GraphedDDPTrainStep", False)
        assert res[r]["loop"]["iters"] == [(1, 0), (2, 1), (3, 2), (4, 3)]          # 3 samples per rank and epoch: one batch
        assert res[r]["loop"]["rows"] == res[r]["hand"]["rows"]
        assert res[r]["loop_adam_steps"] == [4.0]
        assert res[r]["loop_result"]["finished"] and res[r]["loop_result"]["iter"] == 4
    assert res[0]["loop"]["rows"] != res[1]["loop"]["rows"]                         # the ranks train on different crops
    for it in range(4):
        assert same(res[0]["loop"]["weights"][it], res[1]["loop"]["weights"][it]), f"iteration {it + 1}: the ranks differ"
        assert same(res[0]["hand"]["weights"][it], res[1]["hand"]["weights"][it]), f"iteration {it + 1}: the DDP loop's ranks differ"
        assert same(res[0]["loop"]["weights"][it], res[0]["hand"]["weights"][it]), f"iteration {it + 1}: Trainer is not the DDP loop"
    assert not same(res[0]["loop"]["weights"][0], res[0]["loop"]["weights"][3])


@pytest.mark.timeout(900)
def test_files_and_log_are_rank_zeros(ranks, tmp_path):
    """Rank 1 writes nothing; rank 0's files are a single-process run's for the same logger settings; the logged l_pix is the
    mean of the two ranks' own values."""
    out, res = ranks
    assert res[1]["files"] == [], res[1]["files"]
    single = recipe.Trainer(_loop_opt(), make_store("cpu", TRAIN_SHAPES, 1), out_dir=str(tmp_path), rank=0, world=WORLD,
                            step_fn=lambda lq, gt: {"l_pix": torch.tensor(0.0)})
    single.run()
    want = _files(tmp_path)
    assert want == ["models/net_g_3.pth", "models/net_g_latest.pth", "train.log", "training_states/3.state"]
    assert _files(out / "rank0" / "loop") == want
    lines = [json.loads(l) for l in open(out / "rank0" / "loop" / "train.log")]
    logged = {l["iter"]: l for l in lines if "l_pix" in l}
    assert sorted(logged) == [2, 4] and lines[-1] == {"end_of_training": True, "iter": 4}
    for it in (2, 4):
        a, b = (res[r]["hand"]["own_l_pix"][it - 1] for r in range(WORLD))
        mean = float(a * 0.5 + b * 0.5)
        got = logged[it]["l_pix"]
        print(f"iteration {it}: logged l_pix {got!r}, mean of the ranks' own {mean!r}, reduce_loss_dict's {res[0]['hand']['reduced'][it - 1]['l_pix']!r}")
        # the same float32 arithmetic (halves are exact, one rounding in the sum) on the same weights; the own values come from a
        # no_grad forward, so two units in the last place are allowed for them, none for the reference's reduced loss
        assert abs(got - mean) <= 4 * F32 * abs(mean)
        assert got == res[0]["hand"]["reduced"][it - 1]["l_pix"]
        assert got == res[0]["loop"]["losses"][it - 1]["l_pix"] == res[1]["loop"]["losses"][it - 1]["l_pix"]
        assert set(logged[it]) == {"iter", "epoch", "lrs", "l_pix", "l_freq", "l_ssim"}


@pytest.mark.timeout(900)
@pytest.mark.parametrize("name", ["three", "one"])
def test_sharded_validation_equals_the_single_process_score(ranks, name):
    """Three pairs (uneven shards) and one pair (rank 1 scores nothing): score() on both ranks is the single-process score() of
    the same weights, as exact doubles."""
    out, res = ranks
    single = res[0]["val"][name]["single"]
    assert set(single) == {"psnr", "ssim"} and np.isfinite(single["psnr"]) and 0 < single["ssim"] < 1
    for r in range(WORLD):
        assert res[r]["val"][name]["single"] == single
        assert res[r]["val"][name]["sharded"] == single, (r, res[r]["val"][name]["sharded"], single)


@pytest.mark.timeout(900)
def test_resume_at_the_same_world_size_is_exact(ranks, tmp_path):
    """Saved mid-epoch at iteration 3 of 6, fresh Trainers continue to the uninterrupted run's weights and rows on both ranks; the
    state names its world size and holds both ranks' random states.  In a single process the same state restarts its epoch."""
    out, res = ranks
    path = out / "rank0" / "first" / "training_states" / "3.state"
    state = torch.load(path, weights_only=True)
    assert set(state["recipe"]) == {"world", "batch", "rngs"} and state["recipe"]["world"] == WORLD and state["recipe"]["batch"] == 1
    assert not os.path.exists(out / "rank1" / "first")
    for r in range(WORLD):
        assert res[r]["straight"]["iters"] == [(1, 0), (2, 0), (3, 1), (4, 1), (5, 2), (6, 2)]     # two batches per epoch and rank
        assert res[r]["saved_at"] == res[r]["resumed_at"] == (3, 1, 1)
        got = state["recipe"]["rngs"][r]
        assert (got[0], tuple(got[1]), got[2]) == res[r]["saved_rng"]
        assert res[r]["resumed"]["iters"] == res[r]["straight"]["iters"][3:]
        assert res[r]["resumed"]["rows"] == res[r]["straight"]["rows"][3:] and res[r]["resumed"]["lrs"] == res[r]["straight"]["lrs"][3:]
        for k in range(3):
            assert same(res[r]["resumed"]["weights"][k], res[r]["straight"]["weights"][3 + k]), (r, 4 + k)
    assert state["recipe"]["rngs"][0] != state["recipe"]["rngs"][1]
    assert same(res[0]["resumed"]["weights"][-1], res[1]["resumed"]["weights"][-1])
    log = [json.loads(l) for l in open(out / "rank0" / "second" / "train.log")]
    assert [l["exact"] for l in log if "resumed" in l] == [True]

    opt = _resume_opt()
    opt["path"]["resume_state"] = str(path)
    t = recipe.Trainer(opt, make_store("cpu", TRAIN_SHAPES * 2, 1), out_dir=str(tmp_path), step_fn=lambda lq, gt: {})
    assert not t.distributed and (t.current_iter, t.epoch, t._pos) == (3, 1, 0)
    assert t.batcher.rng.getstate() == PairedPatchBatcher(t.train_store, gt_size=64, seed=0).rng.getstate()
    log = [json.loads(l) for l in open(tmp_path / "train.log")]
    assert [l["exact"] for l in log if "resumed" in l] == [False]


def test_refusals_name_the_argument(ranks, tmp_path):
    out, res = ranks
    assert not dist.is_initialized()
    with pytest.raises(ValueError, match="distributed"):
        recipe.Trainer(small_opt(), make_store("cpu", TRAIN_SHAPES, 1), out_dir=str(tmp_path), distributed=True)
    for r in range(WORLD):
        assert res[r]["refused_world"] is not None and res[r]["refused_world"].startswith("world:"), res[r]["refused_world"]
        assert res[r]["refused_rank"] is not None and res[r]["refused_rank"].startswith("rank:"), res[r]["refused_rank"]


def test_fft_weight_reaches_the_data_parallel_step(ranks):
    """l_freq with fft_weight 0.3 is 3 x the default's (0.1) on the same batch and weights.  Both are float32: the two weights'
    roundings, one product and one sum over the ranks each - eight half-units of the last place bound the relative difference."""
    out, res = ranks
    for r in range(WORLD):
        a, b = float(res[r]["l_freq"]["0.3"]), float(res[r]["l_freq"]["default"])
        print(f"rank {r}: l_freq {a!r} at 0.3, {b!r} at the default")
        assert b > 0 and abs(a - 3 * b) <= 8 * F32 * a
    assert float(res[0]["l_freq"]["0.3"]) == float(res[1]["l_freq"]["0.3"])


def test_command_line_under_the_launcher_environment(ranks):
    """recipe.main() with RANK / WORLD_SIZE / LOCAL_RANK set: rank 0 prints the result and owns the files, rank 1 prints nothing,
    the group is gone afterwards."""
    out, res = ranks
    for r in range(WORLD):
        assert res[r]["cli"]["code"] == 0 and not res[r]["cli"]["group_left"]
    assert res[1]["cli"]["stdout"] == ""
    result = json.loads(res[0]["cli"]["stdout"])
    assert result["finished"] and result["iter"] == CLI_ITERS and set(result["validation"]) == {"psnr", "ssim"}
    assert _files(out / "rank0" / "cli") == ["models/net_g_2.pth", "models/net_g_best_2.pth", "models/net_g_latest.pth", "train.log",
                                             "training_states/2.state"]
    lines = [json.loads(l) for l in open(out / "rank0" / "cli" / "train.log")]
    assert [l["iter"] for l in lines if "l_pix" in l] == list(range(1, CLI_ITERS + 1))
    assert torch.load(out / "rank0" / "cli" / "training_states" / "2.state", weights_only=True)["recipe"]["world"] == WORLD
