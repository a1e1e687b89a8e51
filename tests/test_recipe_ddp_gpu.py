"""GPU: recipe.Trainer in its distributed mode with real graphs.  Two ranks replay on the one GPU and exchange the flat buffer over
gloo (as tests/test_rccl_gpu.py::test_graphed_ddp_step_two_ranks_one_gpu_gloo does), and one rank runs over an RCCL communicator
with the all-reduce between the replays and inside the graph.  wf = 8 network and stores of test_recipe_cpu.py, 8 iterations of the
[3, 4] schedule, deterministic mode on inside the workers.  Each group of workers is spawned once per module; the tests read what
they saved."""
import os
import socket
from datetime import timedelta

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_recipe_cpu import TRAIN_SHAPES, VAL_SHAPES, make_store, small_opt

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(out_dir, graphed, opt=None, val=False, **kw):
    """One Trainer.run() on cuda:0 -> what on_iter saw, the flat gradient of iteration 1, the weights after every iteration."""
    from wave_mamba_amd import recipe
    dev = "cuda:0"
    opt = opt if opt is not None else small_opt()
    t = recipe.Trainer(opt, make_store(dev, TRAIN_SHAPES, 1), make_store(dev, VAL_SHAPES, 2) if val else None, graphed=graphed,
                       out_dir=str(out_dir), **kw)
    rec = {"iters": [], "lrs": [], "rows": [], "losses": [], "weights": [], "scores": [], "start": (t.current_iter, t.epoch, t._pos)}
    lr0 = t.optimizer.param_groups[0]["lr"]
    rec["lr_is_device_tensor_before"] = isinstance(lr0, torch.Tensor) and lr0.is_cuda
    score = t.score

    def recording_score():
        rec["scores"].append(score())
        return rec["scores"][-1]
    t.score = recording_score

    def seen(it, epoch, lrs, rows, losses):
        rec["iters"].append(it)
        rec["lrs"].append(lrs)
        rec["rows"].append(rows)
        rec["losses"].append({k: float(v) for k, v in losses.items()})
        rec["weights"].append([p.detach().cpu() for p in t.net.parameters()])
        if len(rec["iters"]) == 1:
            step = t._gstep
            rec["grad"] = (step.flat[:-len(step.losses)] if hasattr(step, "flat") else
                           torch.cat([p.grad.reshape(-1) for g in t.optimizer.param_groups for p in g["params"]])).cpu()
    rec["result"] = t.run(on_iter=seen)
    torch.cuda.synchronize()
    del t.score                                                    # the recording wrapper holds `t`: no cycle, the graphs go with `t`
    lr = t.optimizer.param_groups[0]["lr"]
    rec["lr_kept"] = lr is lr0
    rec["lr_end"] = float(lr)
    rec["step"] = (type(t._gstep).__name__, getattr(t._gstep, "capture", None), getattr(t._gstep, "collective", None))
    rec["mode"] = (t.distributed, t.rank, t.world, t.graphed)
    rec["adam_steps"] = sorted({float(st["step"]) for st in t.optimizer.state.values()})
    if val:
        from test_recipe_gpu import _score_by_hand
        rec["by_hand"] = _score_by_hand(t, 4)
    return rec


def _setup(rank, world, port):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    import wave_mamba_amd as wm
    torch.cuda.set_device(0)
    wm.set_deterministic(True)


def _two_rank_worker(rank, world, port, out_dir):
    """Both ranks on the one GPU, gloo between them: a graphed run that saves at iteration 5, a second graphed run, an eager run, a
    resumed run and a graphed run that validates every second iteration."""
    _setup(rank, world, port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
    try:
        mine = os.path.join(out_dir, f"rank{rank}")
        res = {"graphed": _run(os.path.join(mine, "graphed"), True, small_opt(save_checkpoint_freq=5))}
        res["again"] = _run(os.path.join(mine, "again"), True)
        res["eager"] = _run(os.path.join(mine, "eager"), False)
        dist.barrier()
        opt = small_opt(save_checkpoint_freq=5)
        opt["path"]["resume_state"] = os.path.join(out_dir, "rank0", "graphed", "training_states", "5.state")
        res["resumed"] = _run(os.path.join(mine, "resumed"), True, opt)
        opt = small_opt()
        opt["val"]["val_freq"] = 2
        res["validating"] = _run(os.path.join(mine, "validating"), True, opt, val=True)
        res["files"] = sorted(os.listdir(mine)) if os.path.isdir(mine) else []
        torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


def _one_rank_worker(rank, port, out_dir):
    """One rank over RCCL: the single-process graphed Trainer, then the mode forced on with both collectives, from one seed."""
    _setup(0, 1, port)
    import torch.distributed as dist
    dist.init_process_group("nccl", device_id=torch.device("cuda", 0), rank=0, world_size=1, timeout=timedelta(seconds=120))
    try:
        assert dist.get_backend() == "nccl"
        res = {"single": _run(os.path.join(out_dir, "single"), True)}
        for collective in ("split", "captured"):
            res[collective] = _run(os.path.join(out_dir, collective), True, distributed=True, collective=collective)
        torch.save(res, os.path.join(out_dir, "one.pt"))
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def two(tmp_path_factory):
    import torch.multiprocessing as mp
    out = tmp_path_factory.mktemp("recipe_ddp_two")
    mp.spawn(_two_rank_worker, args=(2, _free_port(), str(out)), nprocs=2, join=True)
    return out, [torch.load(out / f"rank{r}.pt", weights_only=False) for r in range(2)]


@pytest.fixture(scope="module")
def one(tmp_path_factory):
    import torch.multiprocessing as mp
    out = tmp_path_factory.mktemp("recipe_ddp_one")
    mp.spawn(_one_rank_worker, args=(_free_port(), str(out)), nprocs=1, join=True)
    return torch.load(out / "one.pt", weights_only=False)


def same(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


def report(what, a, b):
    """Print, per iteration both runs have, how many weight tensors differ and by how much at the most."""
    for k, (wa, wb) in enumerate(zip(a, b)):
        differing = sum(not torch.equal(p, q) for p, q in zip(wa, wb))
        worst = max(float((p - q).abs().max()) for p, q in zip(wa, wb))
        print(f"{what}, iteration {k + 1} of the shorter run: {differing} of {len(wa)} weight tensors differ, max abs {worst:.3e}")


@pytest.mark.timeout(900)
def test_graphed_ranks_reproduce_and_stay_in_lock_step(two):
    """Two graphed runs from one seed end on torch.equal weights, rank 0 on rank 1's; 8 iterations are 8 optimizer steps on every rank; the lrs are the golden sequence and the replays read them: iteration 8
    (lr exactly 0) moves no weight, iterations 4-7 each move at least one."""
    out, res = two
    with np.load(os.path.join(GOLDEN, "recipe.npz")) as z:
        golden = z["lr.cyclic_short"].tolist()
    report("rank 0 against rank 1", res[0]["graphed"]["weights"], res[1]["graphed"]["weights"])
    for r in range(2):
        g = res[r]["graphed"]
        report(f"rank {r}, two graphed runs", g["weights"], res[r]["again"]["weights"])
        assert g["mode"] == (True, r, 2, True) and g["step"] == ("GraphedDDPTrainStep", True, "split")
        assert g["iters"] == list(range(1, 9)) and g["lrs"] == [[v] for v in golden]
        assert g["adam_steps"] == [8.0], "the constructor's warm-up steps were not undone on this rank"
        assert g["lr_is_device_tensor_before"] and g["lr_kept"] and g["lr_end"] == 0.0
        assert same(g["weights"][7], g["weights"][6]), "the replay at lr = 0 moved a weight"
        for it in (4, 5, 6, 7):
            assert not same(g["weights"][it - 1], g["weights"][it - 2]), f"iteration {it} moved no weight"
        assert all(bool(torch.isfinite(p).all()) for p in g["weights"][7])
        assert same(g["weights"][7], res[r]["again"]["weights"][7]), "two graphed runs differ"
    for it in range(8):
        assert same(res[0]["graphed"]["weights"][it], res[1]["graphed"]["weights"][it]), f"iteration {it + 1}: the ranks differ"
    assert res[0]["graphed"]["rows"] != res[1]["graphed"]["rows"]
    assert res[1]["files"] == [], res[1]["files"]                                   # rank 1 writes no file


@pytest.mark.timeout(900)
def test_graphed_against_eager_in_the_mode(two):
    """The graphs against the eager form of the same step: the same (lrs, rows) per rank; the flat gradient of iteration 1 to 1e-5
    of its largest entry and the logged losses (print_freq 4: iterations 4 and 8) to 1e-5 relative, the bars of
    tests/test_rccl_gpu.py::_check_graphed.  The weight difference after 8 iterations is printed."""
    out, res = two
    for r in range(2):
        g, e = res[r]["graphed"], res[r]["eager"]
        assert e["mode"] == (True, r, 2, False) and e["step"] == ("GraphedDDPTrainStep", False, "split")
        assert e["adam_steps"] == [8.0] and not e["lr_is_device_tensor_before"]
        assert (g["lrs"], g["rows"]) == (e["lrs"], e["rows"])
        grad = float((g["grad"] - e["grad"]).abs().max() / e["grad"].abs().max())
        worst = max(float((p - q).abs().max()) for p, q in zip(g["weights"][7], e["weights"][7]))
        differing = sum(not torch.equal(p, q) for p, q in zip(g["weights"][7], e["weights"][7]))
        print(f"rank {r}: flat gradient of iteration 1, graphed against eager: {grad:.3e} of the largest entry; after 8 iterations "
              f"{differing} of {len(g['weights'][7])} weight tensors differ, max abs {worst:.3e}")
        for it in (4, 8):
            print(f"rank {r} iteration {it}: graphed {g['losses'][it - 1]}, eager {e['losses'][it - 1]}")
        assert grad <= 1e-5
        for it in (4, 8):
            la, lb = g["losses"][it - 1], e["losses"][it - 1]
            assert set(la) == set(lb) == {"l_pix", "l_freq", "l_ssim"} and all(abs(la[k] - lb[k]) <= 1e-5 * abs(lb[k]) for k in lb)
    assert res[0]["eager"]["losses"] == res[1]["eager"]["losses"]                   # every rank holds the mean over ranks
    assert res[0]["graphed"]["losses"] == res[1]["graphed"]["losses"]


@pytest.mark.timeout(900)
def test_resume_into_the_graphs_continues_exactly(two):
    """Fresh Trainers resumed from rank 0's state of iteration 5 replay iterations 6-8 to the uninterrupted run's weights on both
    ranks (one batch per epoch and rank: iteration 5 closed epoch 4); the lr is a device tensor before anything is captured and stays the same object: the one graph B reads (lr 0 at
    iteration 8 moves no weight in the resumed run either)."""
    out, res = two
    state = torch.load(out / "rank0" / "graphed" / "training_states" / "5.state", weights_only=True)
    assert state["recipe"]["world"] == 2 and len(state["recipe"]["rngs"]) == 2
    for r in range(2):
        g, c = res[r]["graphed"], res[r]["resumed"]
        report(f"rank {r}, resumed against uninterrupted", c["weights"], g["weights"][5:])
        assert c["start"] == (5, 4, 1) and c["iters"] == [6, 7, 8] and c["lrs"] == g["lrs"][5:] and c["rows"] == g["rows"][5:]
        assert c["adam_steps"] == [8.0]                                             # 5 restored + 3 replays, no warm-up step left
        assert c["lr_is_device_tensor_before"] and c["lr_kept"] and c["lr_end"] == 0.0
        assert same(c["weights"][2], c["weights"][1]) and not same(c["weights"][1], c["weights"][0])
        assert same(c["weights"][2], g["weights"][7]), f"rank {r}: the resumed run ends on other weights than the uninterrupted one"


@pytest.mark.timeout(900)
def test_sharded_validation_between_replays(two):
    """val_freq 2: validation between the replays leaves the training untouched, and the sharded scores are ops.psnr_ssim_y applied
    by hand to all pairs in store order, as exact doubles, on both ranks."""
    out, res = two
    for r in range(2):
        v = res[r]["validating"]
        report(f"rank {r}, validating against not", v["weights"], res[r]["graphed"]["weights"])
        print(f"rank {r}: scores {v['scores'][-1]}, by hand {v['by_hand']}")
        assert same(v["weights"][7], res[r]["graphed"]["weights"][7]), "validation between replays changed the training"
        assert len(v["scores"]) == 5 and v["scores"][-1] == v["scores"][-2]         # iterations 2, 4, 6, 8 and the end (8 again)
        assert (v["scores"][-1]["psnr"], v["scores"][-1]["ssim"]) == v["by_hand"]
        assert np.isfinite(v["scores"][-1]["psnr"]) and 0 < v["scores"][-1]["ssim"] < 1
        assert v["scores"] == res[0]["validating"]["scores"]
    models = sorted(os.listdir(out / "rank0" / "validating" / "models"))
    assert "net_g_latest.pth" in models and "net_g_best_2.pth" in models, models


@pytest.mark.timeout(900)
@pytest.mark.parametrize("collective", ["split", "captured"])
def test_one_rank_over_rccl_equals_the_single_process_loop(one, collective):
    """distributed=True on a one-rank RCCL communicator against the single-process graphed Trainer from the same seed: the
    all-reduce is the identity and the rest is elementwise the same, so the weights are torch.equal after every iteration."""
    s, d = one["single"], one[collective]
    assert s["mode"] == (False, 0, 1, True) and s["step"][0] == "GraphedTrainStep"
    assert d["mode"] == (True, 0, 1, True) and d["step"] == ("GraphedDDPTrainStep", True, collective)
    assert (d["lrs"], d["rows"]) == (s["lrs"], s["rows"]) and d["adam_steps"] == [8.0]
    grad = float((d["grad"] - s["grad"]).abs().max() / s["grad"].abs().max())
    worst = max(float((p - q).abs().max()) for p, q in zip(d["weights"][7], s["weights"][7]))
    print(f"{collective}: gradient of iteration 1 against the single-process loop {grad:.3e} of the largest entry, weights after 8 "
          f"iterations max abs {worst:.3e}; losses at iteration 8 {d['losses'][7]} against {s['losses'][7]}")
    for it in range(8):
        assert same(d["weights"][it], s["weights"][it]), f"iteration {it + 1}: the weights differ"
