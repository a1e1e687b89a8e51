"""CPU: the recipe's schedulers, sampler, options, loop cadence, best-model bookkeeping and a small eager loop
(wave_mamba_amd/schedulers.py, wave_mamba_amd/recipe.py).  Expected learning rates and sampler index lists are the reference's own
(tests/golden/recipe.npz, written by tests/golden/make_golden_recipe.py); the YAML fixture is a copy of the reference's recipe."""
import collections
import copy
import json
import logging
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import wave_mamba_amd as wm
from wave_mamba_amd import recipe, schedulers, trainer
from wave_mamba_amd.data import DeviceImageStore, PairedPatchBatcher

YAML = os.path.join(GOLDEN, "train_wavemamba_uhdll.yml")
SMALL = dict(type="WaveMamba", in_chn=3, wf=8, n_l_blocks=[1, 1, 1], n_h_blocks=[1, 1, 1], ffn_scale=2.0)   # test_deterministic_gpu.py
TRAIN_SHAPES = [(80, 96)] * 5 + [(60, 70)]               # the last one is smaller than gt_size: the reflect-padded path
VAL_SHAPES = [(72, 88)] * 2
SHORT_SCHEDULE = dict(type="CosineAnnealingRestartCyclicLR", periods=[3, 4], restart_weights=[1, 1], eta_mins=[5e-4, 0.0])


def make_store(device, shapes, seed):
    """Seeded uint8 pairs: gt is noise, lq a darker copy of it (values differ, shapes agree)."""
    rng = np.random.default_rng(seed)
    store = DeviceImageStore(device)
    for h, w in shapes:
        gt = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        store.add((gt // 3 + rng.integers(0, 8, (h, w, 3), dtype=np.uint8)).astype(np.uint8), gt)
    return store


def small_opt(total_iter=8, **logger):
    """The recipe's structure at test size: wf = 8, gt_size 64, batch 3, the [3, 4] schedule."""
    log = dict(print_freq=4, save_checkpoint_freq=1000, save_latest_freq=1000)
    log.update(logger)
    return {
        "scale": 1, "manual_seed": 0,
        "datasets": {"train": {"gt_size": 64, "geometric_augs": True, "batch_size_per_gpu": 3, "dataset_enlarge_ratio": 1}},
        "network_g": dict(SMALL),
        "path": {"pretrain_network_g": None, "strict_load": False, "resume_state": None},
        "train": {"optim_g": {"type": "AdamW", "lr": 5e-4, "weight_decay": 1e-3, "betas": [0.9, 0.99]},
                  "scheduler": copy.deepcopy(SHORT_SCHEDULE), "total_iter": total_iter, "warmup_iter": -1,
                  "pixel_ssim_opt": {"loss_weight": 0.25}, "fft_opt": {"type": "FFTLoss", "loss_weight": 0.1}},
        "val": {"val_freq": 1000, "key_metric": "psnr",
                "metrics": {"psnr": {"type": "psnr", "crop_border": 4, "test_y_channel": True},
                            "ssim": {"type": "ssim", "crop_border": 4, "test_y_channel": True},
                            "lpips": {"type": "lpips", "better": "lower"}}},
        "logger": log,
    }


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "recipe.npz")) as z:
        return {k: z[k] for k in z.files}


def lr_cases(gold):
    for name in gold["cases"].tolist():
        yield name, json.loads(str(gold[f"lr.{name}.spec"])), gold[f"lr.{name}.iters"].tolist(), gold[f"lr.{name}"].tolist()


def drive(opt, spec, iters, on_value):
    sched = schedulers.build_scheduler(opt, dict(spec["kwargs"], type=spec["type"]))
    want = dict(zip(iters, range(len(iters))))
    for current_iter in range(1, iters[-1] + 1):
        schedulers.update_learning_rate([sched], [opt], current_iter, spec["warmup_iter"])
        if current_iter in want:
            on_value(want[current_iter], current_iter)
    return sched


def _param():
    return [torch.nn.Parameter(torch.zeros(1))]


# ---- schedulers ------------------------------------------------------------------------------------------------------------------
def test_float_lr_equals_the_reference_exactly(gold):
    """Every golden case (three classes, with and without warm-up, the recipe over 1-300 and 100095-100101, the [3, 4] schedule):
    a float lr is the reference's float64 value, bit for bit."""
    for name, spec, iters, lrs in lr_cases(gold):
        opt = torch.optim.AdamW(_param(), lr=spec["base_lr"])

        def check(k, it):
            lr = opt.param_groups[0]["lr"]
            assert isinstance(lr, float) and lr == lrs[k], f"{name} iteration {it}: {lr!r} != {lrs[k]!r}"
            assert schedulers.current_lrs([opt]) == [lrs[k]]
        drive(opt, spec, iters, check)
    assert gold["lr.cyclic_short"][-1] == 0.0                       # the schedule the GPU tests replay ends at exactly 0


def test_tensor_lr_is_filled_in_place_with_the_float32_rounding(gold):
    """A tensor lr holds float32(golden) after every update, warm-up included, and is the SAME tensor object throughout; its
    float64 value is kept beside it."""
    for name, spec, iters, lrs in lr_cases(gold):
        if name == "cyclic_recipe_end":
            continue                                                 # 100,000 fills: the float test covers the values
        opt = torch.optim.AdamW(_param(), lr=torch.tensor(spec["base_lr"], dtype=torch.float32), foreach=False)
        tensor = opt.param_groups[0]["lr"]
        schedulers.set_lr(opt, [spec["base_lr"]])                    # records the exact float64 base lr

        def check(k, it):
            group = opt.param_groups[0]
            assert group["lr"] is tensor, f"{name} iteration {it}: the lr tensor was rebound"
            assert tensor.item() == float(np.float32(lrs[k])), f"{name} iteration {it}: {tensor.item()!r} != float32({lrs[k]!r})"
            assert group["lr_host"] == lrs[k] and isinstance(group["initial_lr"], float)
        sched = drive(opt, spec, iters, check)
        assert all(isinstance(v, float) for v in sched.base_lrs + sched._last_lr)


def _is_plain(v):
    if isinstance(v, dict):
        return type(v) is dict and all(type(k) in (str, int) and _is_plain(x) for k, x in v.items())
    if isinstance(v, list):
        return all(_is_plain(x) for x in v)
    return type(v) in (int, float, bool)


@pytest.mark.parametrize("name", ["cyclic_short_warmup", "cosine_warmup", "multistep_warmup"])
def test_scheduler_state_round_trip_under_weights_only(gold, name, tmp_path):
    """state_dict() is ints, floats, lists and dicts; saved and read back with weights_only=True into a fresh scheduler (through
    trainer.save_training_state / resume_training) the schedule continues on the golden values."""
    spec, iters, lrs = next((s, i, v) for n, s, i, v in lr_cases(gold) if n == name)
    half = len(iters) // 2
    opt = torch.optim.AdamW(_param(), lr=spec["base_lr"])
    sched = drive(opt, spec, iters[:half], lambda k, it: None)
    assert _is_plain(sched.state_dict()), sched.state_dict()
    path = trainer.save_training_state(str(tmp_path / "s.state"), 0, half, [opt], [sched], extra={"batch": 1, "rng": (3, (1, 2), None)})
    blob = torch.load(path, weights_only=True)
    assert blob["recipe"] == {"batch": 1, "rng": (3, (1, 2), None)} and set(blob) == {"epoch", "iter", "optimizers", "schedulers", "recipe"}
    opt2 = torch.optim.AdamW(_param(), lr=spec["base_lr"])
    sched2 = schedulers.build_scheduler(opt2, dict(spec["kwargs"], type=spec["type"]))
    assert trainer.resume_training(path, [opt2], [sched2]) == (0, half)
    for k in range(half, len(iters)):
        schedulers.update_learning_rate([sched2], [opt2], iters[k], spec["warmup_iter"])
        assert opt2.param_groups[0]["lr"] == lrs[k], (name, iters[k])


def test_scheduler_loads_a_state_shaped_like_the_reference_class_wrote(gold):
    """The reference's state holds a Counter, tuples and (around a tensor lr) tensors under the same keys."""
    spec, iters, lrs = next((s, i, v) for n, s, i, v in lr_cases(gold) if n == "multistep")
    kw = spec["kwargs"]
    state = {"milestones": collections.Counter(kw["milestones"]), "gamma": kw["gamma"], "restarts": tuple(kw["restarts"]),
             "restart_weights": tuple(kw["restart_weights"]), "base_lrs": [torch.tensor(spec["base_lr"], dtype=torch.float64)],
             "last_epoch": 4, "_step_count": 5, "verbose": False, "_get_lr_called_within_step": False,
             "_last_lr": [torch.tensor(lrs[4], dtype=torch.float64)]}
    opt = torch.optim.AdamW(_param(), lr=spec["base_lr"])
    sched = schedulers.build_scheduler(opt, dict(kw, type=spec["type"]))
    sched.load_state_dict(state)
    opt.param_groups[0]["lr"] = lrs[4]                               # what the optimizer's own state would restore
    assert isinstance(sched.milestones, collections.Counter) and sched.milestones[5] == 2 and _is_plain(sched.state_dict())
    for k in range(5, len(iters)):
        schedulers.update_learning_rate([sched], [opt], iters[k])
        assert opt.param_groups[0]["lr"] == lrs[k]


def test_past_the_last_period_is_a_value_error_that_names_the_iteration():
    opt = torch.optim.AdamW(_param(), lr=5e-4)
    sched = schedulers.build_scheduler(opt, SHORT_SCHEDULE)
    assert sched.last_iter() == 8
    for it in range(1, 9):
        schedulers.update_learning_rate([sched], [opt], it)
    with pytest.raises(ValueError, match=r"iteration 9 .*sum\(periods\) = 7"):
        schedulers.update_learning_rate([sched], [opt], 9)
    shipped, _ = recipe.load_options(YAML)
    assert schedulers.build_scheduler(torch.optim.AdamW(_param(), lr=5e-4), shipped["train"]["scheduler"]).last_iter() == 100101
    with pytest.raises(NotImplementedError):
        schedulers.build_scheduler(opt, {"type": "StepLR"})
    assert SHORT_SCHEDULE["type"] == "CosineAnnealingRestartCyclicLR"          # build_scheduler does not pop from its argument


# ---- sampler and options ---------------------------------------------------------------------------------------------------------
def test_sampler_index_lists_equal_the_reference(gold):
    keys = [k for k in gold if k.startswith("sampler.")]
    assert {"sampler.10_3_2_1_4", "sampler.7_1_1_0_0", "sampler.2000_1_8_5_3"} <= set(keys)
    for key in keys:
        n, ratio, world, rank, epoch = (int(v) for v in key.split(".")[1].split("_"))
        s = recipe.EnlargedSampler(n, world, rank, ratio)
        s.set_epoch(epoch)
        assert list(s) == gold[key].tolist() and len(s) == len(gold[key]), key
    s = recipe.EnlargedSampler(7, 1, 0, 1)
    want = gold["sampler.7_1_1_0_0"].tolist()
    assert s.batches(3) == [want[0:3], want[3:6]]                                # the short last batch is dropped


def test_yaml_fixture_parses_to_the_shipped_settings():
    opt, derived = recipe.load_options(YAML, num_train=2000)
    assert opt["network_g"] == dict(type="WaveMamba", in_chn=3, wf=32, n_l_blocks=[1, 2, 4], n_h_blocks=[1, 1, 2], ffn_scale=2.0)
    assert opt["train"]["optim_g"] == dict(type="AdamW", lr=5e-4, weight_decay=1e-3, betas=[0.9, 0.99])
    assert opt["train"]["scheduler"] == dict(type="CosineAnnealingRestartCyclicLR", periods=[100, 100000], restart_weights=[1, 1],
                                             eta_mins=[0.0005, 0.0000001])
    assert derived == {"num_iter_per_epoch": 250, "total_iters": 101000, "total_epochs": 404}
    assert recipe.load_options(open(YAML).read())[1] is None                     # the text itself; no pair count, nothing derived
    assert set(recipe.usable_metrics(opt)) == {"psnr", "ssim"}


@pytest.mark.parametrize("change, key", [
    (lambda o: o["train"]["optim_g"].update(type="Adam"), "train.optim_g.type"),
    (lambda o: o.update(scale=2), "scale"),
    (lambda o: o["val"]["metrics"]["ssim"].update(test_y_channel=False), "val.metrics.ssim.test_y_channel"),
])
def test_options_are_refused_up_front_by_key(change, key):
    opt = small_opt()
    change(opt)
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        recipe.check_options(opt)
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        recipe.Trainer(opt, make_store("cpu", [(64, 64)] * 3, 1))


# ---- loop cadence ----------------------------------------------------------------------------------------------------------------
def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_loop_cadence_with_a_counting_step(tmp_path):
    """print / save / latest / val every 2 / 3 / 4 / 5 over 7 iterations with a stub in place of the step."""
    steps, validated, seen = [], [], []
    opt = small_opt(total_iter=7, print_freq=2, save_checkpoint_freq=3, save_latest_freq=4)
    opt["val"]["val_freq"] = 5.0                                                  # a !!float, as the shipped file writes it

    def step_fn(lq, gt):
        assert lq.shape == gt.shape == (3, 3, 64, 64)
        steps.append(1)
        return {"l_pix": torch.tensor(float(len(steps)))}
    t = recipe.Trainer(opt, make_store("cpu", TRAIN_SHAPES, 1), make_store("cpu", [(16, 16)], 2), out_dir=str(tmp_path), step_fn=step_fn)
    t.validate = lambda current_iter, epoch: validated.append(current_iter)
    out = t.run(on_iter=lambda it, epoch, lrs, rows, losses: seen.append((it, epoch)))
    assert out["finished"] and out["iter"] == 7 and len(steps) == 7
    assert seen == [(1, 0), (2, 0), (3, 1), (4, 1), (5, 2), (6, 2), (7, 3)]       # 6 samples, batch 3: two iterations per epoch
    assert _files(tmp_path) == sorted(["train.log"] + [f"models/net_g_{k}.pth" for k in (3, 4, 6, "latest")]
                                      + [f"training_states/{k}.state" for k in (3, 4, 6)])
    assert validated == [5, 7]                                                    # at iteration 5 and at the end
    lines = [json.loads(l) for l in open(tmp_path / "train.log")]
    assert [(l["iter"], l["l_pix"]) for l in lines if "l_pix" in l] == [(2, 2.0), (4, 4.0), (6, 6.0)]
    assert all(len(l["lrs"]) == 1 for l in lines if "l_pix" in l)


def test_loop_ends_where_the_schedule_ends(tmp_path, caplog):
    """total_iter 12 with periods [3, 4]: iteration 8 is the last one the schedule has a value for.  The loop says so before it
    starts and ends there with its save and validation (the reference dies at iteration 9 with nothing saved)."""
    validated = []
    with caplog.at_level(logging.WARNING, logger="wave_mamba_amd"):
        t = recipe.Trainer(small_opt(total_iter=12), make_store("cpu", TRAIN_SHAPES, 1), make_store("cpu", [(16, 16)], 2),
                           out_dir=str(tmp_path), step_fn=lambda lq, gt: {"l_pix": torch.tensor(0.0)})
    assert any("iteration 8 is the last" in r.getMessage() for r in caplog.records)
    assert sum("lpips" in r.getMessage() for r in caplog.records) == 1              # the lpips metric is skipped with ONE warning
    t.validate = lambda current_iter, epoch: validated.append(current_iter)
    assert t.run()["iter"] == 8 and validated == [8] and os.path.exists(tmp_path / "models" / "net_g_latest.pth")


def test_max_iters_pauses_and_run_continues(tmp_path):
    seen = []
    t = recipe.Trainer(small_opt(total_iter=5), make_store("cpu", TRAIN_SHAPES, 1), out_dir=str(tmp_path),
                       step_fn=lambda lq, gt: {"l_pix": torch.tensor(0.0)})
    out = t.run(max_iters=2, on_iter=lambda it, *a: seen.append(it))
    assert out == {"iter": 2, "epoch": 1, "finished": False}      # epoch 0 has two batches: the next one is epoch 1's
    assert not os.path.exists(tmp_path / "models")                 # a pause is not the end of training: nothing is saved
    assert t.run(on_iter=lambda it, *a: seen.append(it))["finished"] and seen == [1, 2, 3, 4, 5]


# ---- best bookkeeping -------------------------------------------------------------------------------------------------------------
def test_best_bookkeeping_with_a_key_metric():
    """Only the key metric decides; a tie is an update; on an update every record takes this validation's value."""
    best = recipe.BestMetrics({"psnr": {}, "ssim": {}, "err": {"better": "lower"}})
    script = [(10, dict(psnr=20.0, ssim=0.5, err=3.0), True), (20, dict(psnr=19.0, ssim=0.9, err=1.0), False),
              (30, dict(psnr=20.0, ssim=0.4, err=5.0), True), (40, dict(psnr=21.0, ssim=0.4, err=5.0), True)]
    for it, results, want in script:
        assert best.update(results, it, "psnr") is want, it
    assert best.records["psnr"] == {"better": "higher", "val": 21.0, "iter": 40}
    assert best.records["ssim"]["val"] == 0.4 and best.records["err"] == {"better": "lower", "val": 5.0, "iter": 40}
    low = recipe.BestMetrics({"err": {"better": "lower"}})
    assert [low.update({"err": v}, i, "err") for i, v in enumerate([3.0, 3.0, 4.0, 2.0])] == [True, True, False, True]


def test_best_bookkeeping_without_a_key_metric():
    """Every metric keeps its own best; any update saves."""
    best = recipe.BestMetrics({"psnr": {}, "err": {"better": "lower"}})
    script = [(1, dict(psnr=20.0, err=3.0), True), (2, dict(psnr=19.0, err=4.0), False), (3, dict(psnr=19.5, err=3.0), True),
              (4, dict(psnr=20.0, err=9.0), True), (5, dict(psnr=1.0, err=9.0), False)]
    for it, results, want in script:
        assert best.update(results, it) is want, it
    assert (best.records["psnr"]["val"], best.records["psnr"]["iter"]) == (20.0, 4)
    assert (best.records["err"]["val"], best.records["err"]["iter"]) == (3.0, 3)


def test_validation_writes_the_best_file_by_the_key_metric(tmp_path):
    """Trainer.validate with scripted scores: net_g_best_{iter}.pth appears when and only when the key metric improves or ties."""
    t = recipe.Trainer(small_opt(), make_store("cpu", TRAIN_SHAPES, 1), make_store("cpu", [(16, 16)], 2), out_dir=str(tmp_path),
                       step_fn=lambda lq, gt: {})
    scores = iter([dict(psnr=10.0, ssim=0.2), dict(psnr=9.0, ssim=0.9), dict(psnr=10.0, ssim=0.1)])
    t.score = lambda: next(scores)
    for it in (2, 4, 6):
        t.validate(it, 0)
    assert _files(tmp_path / "models") == ["net_g_best_2.pth", "net_g_best_6.pth"]
    log = [json.loads(l) for l in open(tmp_path / "train.log")]
    assert [l["best"]["psnr"]["iter"] for l in log if "validation" in l] == [2, 2, 6]
    t.key_metric, t.best = None, recipe.BestMetrics(t.metrics)
    t.score = lambda: dict(psnr=1.0, ssim=0.1)
    t.validate(8, 0)
    assert "net_g_best_.pth" in _files(tmp_path / "models")


# ---- a small eager loop on the CPU -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_run(tmp_path_factory):
    """Three eager iterations of the wf = 8 network on a CPU store, saving at iteration 2, with one validation at the end."""
    out = tmp_path_factory.mktemp("cpu_run")
    opt = small_opt(total_iter=3, print_freq=1, save_checkpoint_freq=2)
    seen = []
    t = recipe.Trainer(opt, make_store("cpu", TRAIN_SHAPES, 1), make_store("cpu", VAL_SHAPES[:1], 2), out_dir=str(out))
    result = t.run(on_iter=lambda it, epoch, lrs, rows, losses: seen.append((it, epoch, lrs, rows, {k: float(v) for k, v in losses.items()})))
    return out, opt, t, seen, result


def test_cpu_loop_rows_follow_the_sampler_and_the_batcher(cpu_run, gold):
    out, opt, t, seen, result = cpu_run
    batcher = PairedPatchBatcher(make_store("cpu", TRAIN_SHAPES, 1), gt_size=64, seed=0)
    e0, e1 = gold["sampler.6_1_1_0_0"].tolist(), gold["sampler.6_1_1_0_1"].tolist()
    want = [batcher.draw(idx) for idx in (e0[0:3], e0[3:6], e1[0:3])]
    assert [s[3] for s in seen] == want and [s[:2] for s in seen] == [(1, 0), (2, 0), (3, 1)]
    assert [s[2] for s in seen] == [[v] for v in gold["lr.cyclic_short"].tolist()[:3]]
    assert all(set(s[4]) == {"l_pix", "l_freq", "l_ssim"} and all(np.isfinite(v) for v in s[4].values()) for s in seen)
    assert result["finished"] and set(result["validation"]) == {"psnr", "ssim"}
    assert all(np.isfinite(v) for v in result["validation"].values()) and 0 < result["validation"]["ssim"] < 1


def test_cpu_loop_writes_loadable_checkpoints(cpu_run):
    out, opt, t, seen, result = cpu_run
    assert _files(out) == ["models/net_g_2.pth", "models/net_g_best_3.pth", "models/net_g_latest.pth", "train.log",
                           "training_states/2.state"]
    net = wm.build_network(SMALL)
    assert trainer.load_network(net, str(out / "models" / "net_g_latest.pth")) == ([], [], [])
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), t.net.state_dict().values()))
    state = torch.load(out / "training_states" / "2.state", weights_only=True)
    assert state["iter"] == 2 and state["epoch"] == 0 and state["recipe"]["batch"] == 2 and len(state["recipe"]["rng"][1]) == 625
    assert torch.load(out / "models" / "net_g_2.pth", weights_only=True)["iter"] == 2


def test_cpu_loop_resumes_where_it_stopped(cpu_run, tmp_path):
    """A fresh Trainer resumed from iteration 2 draws iteration 3's rows and lr exactly as the uninterrupted run did."""
    out, opt, t, seen, result = cpu_run
    opt2 = copy.deepcopy(opt)
    opt2["path"]["resume_state"] = str(out / "training_states" / "2.state")
    again = []
    t2 = recipe.Trainer(opt2, make_store("cpu", TRAIN_SHAPES, 1), out_dir=str(tmp_path))
    assert (t2.current_iter, t2.epoch) == (2, 0)
    t2.run(on_iter=lambda it, epoch, lrs, rows, losses: again.append((it, epoch, lrs, rows)))
    assert again == [s[:4] for s in seen[2:]]
    worst = max(float((a - b).abs().max()) for a, b in zip(t2.net.state_dict().values(), t.net.state_dict().values()))
    print(f"resumed CPU run against the uninterrupted one: max abs weight difference {worst:.3e}")
    assert worst <= 1e-6                  # one AdamW step of lr 5e-4 apart would be ~5e-4; CPU kernels need not be bit-reproducible
