"""GPU: what is specific to the device in recipe.Trainer - the learning rate inside a captured graph, eager validation between
replays, and exact resume into a graph.  wf = 8 network of tests/test_deterministic_gpu.py, the stores of test_recipe_cpu.py on the
device, 8 iterations of the [3, 4] schedule (lr 5e-4 for iterations 1-4, then a cosine to exactly 0 at iteration 8), deterministic
mode on.  The runs are made once per module and shared."""
import copy
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import wave_mamba_amd as wm
from wave_mamba_amd import recipe
from test_recipe_cpu import TRAIN_SHAPES, VAL_SHAPES, make_store, small_opt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def deterministic():
    prev = wm.set_deterministic(True)
    yield
    wm.set_deterministic(prev)


@pytest.fixture(scope="module")
def golden_lrs():
    with np.load(os.path.join(GOLDEN, "recipe.npz")) as z:
        return z["lr.cyclic_short"].tolist()


class Run:
    """One Trainer.run(): per iteration the host values on_iter saw and a copy of every weight."""

    def __init__(self, out_dir, graphed, opt=None, val=False, prepare=None):
        self.opt = opt if opt is not None else small_opt()
        self.trainer = recipe.Trainer(self.opt, make_store(DEV, TRAIN_SHAPES, 1), make_store(DEV, VAL_SHAPES, 2) if val else None,
                                      graphed=graphed, out_dir=str(out_dir))
        self.iters, self.lrs, self.rows, self.weights = [], [], [], []
        if prepare is not None:
            prepare(self.trainer)
        self.result = self.trainer.run(on_iter=self._seen)
        torch.cuda.synchronize()
        self.final = [p.detach().clone() for p in self.trainer.net.parameters()]

    def _seen(self, it, epoch, lrs, rows, losses):
        self.iters.append(it)
        self.lrs.append(lrs)
        self.rows.append(rows)
        self.weights.append([p.detach().clone() for p in self.trainer.net.parameters()])


def same(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


def optimizer_steps(t):
    """AdamW's own step counters: the number of optimizer steps every parameter has taken."""
    return {float(st["step"]) for st in t.optimizer.state.values()}


@pytest.fixture(scope="module")
def graphed(tmp_path_factory):
    """Eight graphed iterations, saving at iteration 5 (the state the resume test starts from)."""
    return Run(tmp_path_factory.mktemp("graphed"), True, small_opt(save_checkpoint_freq=5))


@pytest.fixture(scope="module")
def eager(tmp_path_factory):
    return Run(tmp_path_factory.mktemp("eager"), False)


def test_the_replayed_step_reads_the_schedule(graphed, golden_lrs):
    """The lr the replays use is the scheduler's: at iteration 8 it is exactly 0.0 and no weight moves (AdamW's decay scales with
    lr too); after each of iterations 4-7 at least one does; the lrs on_iter saw are the golden sequence."""
    t = graphed.trainer
    assert t.graphed and t._gstep is not None and graphed.iters == list(range(1, 9))
    lr = t.optimizer.param_groups[0]["lr"]
    assert isinstance(lr, torch.Tensor) and lr.is_cuda and lr is t._gstep.lr_tensors[0] and float(lr) == 0.0
    assert graphed.lrs == [[v] for v in golden_lrs]
    assert optimizer_steps(t) == {8.0}, "the capture's warm-up steps were not undone: an iteration is more than one optimizer step"
    assert same(graphed.weights[7], graphed.weights[6]), "the replay at lr = 0 moved a weight: the captured lr is not the scheduler's"
    for it in (4, 5, 6, 7):
        assert not same(graphed.weights[it - 1], graphed.weights[it - 2]), f"iteration {it} moved no weight"
    assert all(bool(torch.isfinite(p).all()) for p in graphed.final)


def test_each_loop_kind_reproduces_itself(graphed, eager, tmp_path):
    """Two graphed runs from one seed end on torch.equal weights, and so do two eager runs; graphed and eager runs see the same
    (lrs, rows).  Whether graphed and eager weights are bit-equal is printed, not asserted."""
    again_g, again_e = Run(tmp_path / "g", True), Run(tmp_path / "e", False)
    assert same(graphed.final, again_g.final), "two graphed runs differ"
    assert same(eager.final, again_e.final), "two eager runs differ"
    assert not eager.trainer.graphed and isinstance(eager.trainer.optimizer.param_groups[0]["lr"], float)
    assert optimizer_steps(eager.trainer) == {8.0}
    assert (graphed.lrs, graphed.rows) == (eager.lrs, eager.rows) == (again_g.lrs, again_g.rows)
    differing = sum(not torch.equal(p, q) for p, q in zip(graphed.final, eager.final))
    worst = max(float((p - q).abs().max()) for p, q in zip(graphed.final, eager.final))
    print(f"graphed against eager after 8 iterations: {differing} of {len(graphed.final)} weight tensors differ, max abs {worst:.3e}")


def test_resume_into_a_graph_continues_exactly(graphed, tmp_path):
    """A fresh Trainer resumed from the state of iteration 5 replays iterations 6-8 to the uninterrupted run's weights; its lr is a
    device tensor again, and the very one the captured step reads."""
    opt = copy.deepcopy(graphed.opt)
    opt["path"]["resume_state"] = os.path.join(graphed.trainer.out_dir, "training_states", "5.state")
    seen = {}

    def before_run(t):
        lr = t.optimizer.param_groups[0]["lr"]
        seen["lr"] = lr
        assert isinstance(lr, torch.Tensor) and lr.is_cuda, f"after resume_training the lr is {type(lr).__name__}"
        assert (t.current_iter, t.epoch, t._gstep) == (5, 2, None)                 # resumed before anything is captured
    run = Run(tmp_path, True, opt, prepare=before_run)
    t = run.trainer
    assert run.iters == [6, 7, 8] and run.lrs == graphed.lrs[5:] and run.rows == graphed.rows[5:]
    assert optimizer_steps(t) == {8.0}                                             # 5 restored + 3 replays, no warm-up step left
    assert t.optimizer.param_groups[0]["lr"] is seen["lr"] is t._gstep.lr_tensors[0]
    assert same(run.final, graphed.final), "the resumed run ends on other weights than the uninterrupted one"


def _score_by_hand(t, crop):
    """ops.psnr_ssim_y on every validation pair of `t` at its current weights -> (mean PSNR, mean SSIM), summed in store order."""
    total = [0.0, 0.0]
    for i in range(len(t.val_store)):
        lq, gt = t.val_store.pair(i)
        t.net.eval()
        with torch.no_grad():
            out = wm.ops.image_post_u8(t.net.test(wm.ops.image_pre_u8(lq, 8, True)), lq.shape[0], lq.shape[1], True)
        t.net.train()
        psnr, ssim = wm.ops.psnr_ssim_y(out, gt, crop, layout="HWC", bgr=True)[0].tolist()
        total = [total[0] + psnr, total[1] + ssim]
    return total[0] / len(t.val_store), total[1] / len(t.val_store)


def test_validation_between_replays(graphed, tmp_path):
    """val_freq 2 in a graphed run: eager validation between replays leaves the training untouched (torch.equal weights with the
    run that never validates), its scores are ops.psnr_ssim_y applied by hand as exact doubles, and net_g_best_{iter}.pth appears
    when and only when the scripted key metric improves or ties."""
    opt = small_opt()
    opt["val"]["val_freq"] = 2
    real, script = [], iter([10.0, 9.0, 11.0, 11.0, 5.0])                          # iterations 2, 4, 6, 8 and the end (8 again)

    def scripted(t):
        score = t.score

        def fake():
            real.append(score())
            return dict(real[-1], psnr=next(script))
        t.score = fake
    run = Run(tmp_path, True, opt, val=True, prepare=scripted)
    assert same(run.final, graphed.final), "validation between replays changed the training"
    assert len(real) == 5 and all(set(r) == {"psnr", "ssim"} for r in real)
    assert real[-1] == real[-2]                                                    # iteration 8 and the end: the same weights
    assert (real[-1]["psnr"], real[-1]["ssim"]) == _score_by_hand(run.trainer, 4)
    assert np.isfinite(real[-1]["psnr"]) and 0 < real[-1]["ssim"] < 1
    models = sorted(os.listdir(tmp_path / "models"))
    assert models == ["net_g_best_2.pth", "net_g_best_6.pth", "net_g_best_8.pth", "net_g_latest.pth"], models
    assert run.trainer.best.records["psnr"] == {"better": "higher", "val": 11.0, "iter": 8}


def test_resume_training_keeps_the_device_lr_tensor_for_a_reference_state():
    """A state the reference wrote holds a float lr: the capturable optimizer's device tensor stays in its group, filled with it."""
    net = torch.nn.Linear(4, 3).to(DEV)
    opt = wm.trainer.make_optimizer(net, capturable=True)
    sched = wm.schedulers.build_scheduler(opt, dict(type="MultiStepRestartLR", milestones=[100]))
    tensor = opt.param_groups[0]["lr"]
    state = {"epoch": 3, "iter": 7, "optimizers": [copy.deepcopy(opt.state_dict())], "schedulers": [sched.state_dict()]}
    state["optimizers"][0]["param_groups"][0]["lr"] = 1.25e-4
    state["optimizers"][0]["param_groups"][0].pop("lr_host", None)
    assert wm.trainer.resume_training(state, [opt], [sched]) == (3, 7)
    group = opt.param_groups[0]
    assert group["lr"] is tensor and tensor.is_cuda and tensor.item() == float(np.float32(1.25e-4)) and group["lr_host"] == 1.25e-4
