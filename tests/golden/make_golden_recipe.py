#!/usr/bin/env python3
"""Generate tests/golden/recipe.npz: learning rates of the reference's three schedulers (basicsr/models/lr_scheduler.py) driven
the way BaseModel.update_learning_rate drives them (base_model.py:188-209), and index lists of its EnlargedSampler
(basicsr/data/data_sampler.py).

TEST INFRASTRUCTURE - runs ONLY where the reference tree is mounted read-only at /root/reference (as make_golden.py).  The
fixture is data only.  Both reference files import torch and the standard library alone, so they are loaded by path as they are.

Every optimizer here has a Python-float lr: the reference then computes in float64, which is the definition the package's
schedulers follow for float AND tensor lrs.  The driver below is the reference's update_learning_rate for one optimizer:
scheduler.step() when current_iter > 1, then, while current_iter < warmup_iter, lr = initial_lr / warmup_iter * current_iter.

  lr.<case>            float64 (n,): the lr of group 0 AFTER update_learning_rate(current_iter), per iteration of the case
  lr.<case>.iters      int64 (n,): those iterations
  cases                the case names; lr.<case>.spec: a JSON string {"type", "kwargs", "base_lr", "warmup_iter"}
  sampler.<n>_<ratio>_<world>_<rank>_<epoch>   int64: list(iter(sampler)) after set_epoch(epoch)

Usage:  python tests/golden/make_golden_recipe.py
"""
import importlib.util
import json
import os

import numpy as np
import torch

REF_ROOT = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "recipe.npz")

RECIPE = dict(periods=[100, 100000], restart_weights=[1, 1], eta_mins=[0.0005, 0.0000001])       # train_wavemamba_uhdll.yml:86-90
SHORT = dict(periods=[3, 4], restart_weights=[1, 1], eta_mins=[5e-4, 0.0])
# name: (class, kwargs, base lr, warmup_iter, first iteration kept, last iteration)
LR_CASES = {
    "cyclic_recipe": ("CosineAnnealingRestartCyclicLR", RECIPE, 5e-4, -1, 1, 300),
    "cyclic_recipe_warmup": ("CosineAnnealingRestartCyclicLR", RECIPE, 5e-4, 150, 1, 300),
    "cyclic_recipe_end": ("CosineAnnealingRestartCyclicLR", RECIPE, 5e-4, -1, 100095, 100101),
    "cyclic_short": ("CosineAnnealingRestartCyclicLR", SHORT, 5e-4, -1, 1, 8),
    "cyclic_short_warmup": ("CosineAnnealingRestartCyclicLR", SHORT, 5e-4, 6, 1, 8),
    "cosine": ("CosineAnnealingRestartLR", dict(periods=[100, 200], restart_weights=[1, 1], eta_min=1e-7), 5e-4, -1, 1, 300),
    "cosine_warmup": ("CosineAnnealingRestartLR", dict(periods=[3, 4], eta_min=1e-6), 2e-4, 5, 1, 8),
    "multistep": ("MultiStepRestartLR", dict(milestones=[3, 5, 5, 11], gamma=0.5, restarts=[0, 8], restart_weights=[1, 0.5]),
                  2e-4, -1, 1, 14),
    "multistep_warmup": ("MultiStepRestartLR", dict(milestones=[3, 5, 5, 11], gamma=0.5, restarts=[0, 8], restart_weights=[1, 0.5]),
                         2e-4, 7, 1, 14),
}
SAMPLER_CASES = [(10, 3, 2, 1, 4), (7, 1, 1, 0, 0), (2000, 1, 8, 5, 3), (6, 1, 1, 0, 0), (6, 1, 1, 0, 1), (6, 1, 1, 0, 2),
                 (6, 1, 1, 0, 3), (6, 1, 1, 0, 4)]


def load(name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF_ROOT, *parts))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def drive(cls, kwargs, base_lr, warmup_iter, first, last):
    opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=base_lr)
    sched = cls(opt, **kwargs)
    iters, lrs = [], []
    for current_iter in range(1, last + 1):
        if current_iter > 1:
            opt.step()                                   # (keeps torch's call-order warning quiet; no gradient: nothing moves)
            sched.step()
        if current_iter < warmup_iter:
            for group in opt.param_groups:
                group["lr"] = group["initial_lr"] / warmup_iter * current_iter
        if current_iter >= first:
            lr = opt.param_groups[0]["lr"]
            assert isinstance(lr, float)
            iters.append(current_iter)
            lrs.append(lr)
    return np.array(iters, dtype=np.int64), np.array(lrs, dtype=np.float64)


def main():
    sch = load("lr_scheduler", "basicsr", "models", "lr_scheduler.py")
    smp = load("data_sampler", "basicsr", "data", "data_sampler.py")
    out = {"cases": np.array(list(LR_CASES))}
    for name, (cls, kwargs, base_lr, warmup, first, last) in LR_CASES.items():
        iters, lrs = drive(getattr(sch, cls), kwargs, base_lr, warmup, first, last)
        out[f"lr.{name}"], out[f"lr.{name}.iters"] = lrs, iters
        out[f"lr.{name}.spec"] = np.array(json.dumps({"type": cls, "kwargs": kwargs, "base_lr": base_lr, "warmup_iter": warmup}))
        print(f"{name:24s} {len(lrs):4d} values, first {lrs[0]!r} last {lrs[-1]!r}")
    for n, ratio, world, rank, epoch in SAMPLER_CASES:
        s = smp.EnlargedSampler(range(n), world, rank, ratio)
        s.set_epoch(epoch)
        idx = np.array(list(iter(s)), dtype=np.int64)
        assert len(idx) == len(s)
        out[f"sampler.{n}_{ratio}_{world}_{rank}_{epoch}"] = idx
        print(f"sampler {(n, ratio, world, rank, epoch)}: {len(idx)} indices, first {idx[:6].tolist()}")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
