"""The inputs and yardsticks of the AdamW step's cases, shared by tests/test_adamw_cpu.py (cpu_twin.adamw_step and trainer.HipAdamW
against torch.optim.AdamW) and tests/test_adamw_gpu.py (wm_adamw_step against a float64 evaluation, held to torch's own error).
Everything is seeded and built on the CPU.  A run is STEPS steps from one fp32 start over tensors of SIZES floats, with gradients
whose scale climbs from 1e-6 to 10; its results are computed once per process and handed out as they are - nobody writes to them."""
import functools

import torch

from wave_mamba_amd import ops

CHUNK = ops.GRAD_GUARD_CHUNK
SIZES = [1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]       # 1 3 4 5 4095 4096 4097 8193
STEPS = 20
HYPER = dict(lr=5e-4, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-3)   # the recipe's optimizer (train_wavemamba_uhdll.yml:75-79)
EMA_DECAY = 0.9                                                          # far enough from 1 for the average to move in 20 steps
KINDS = ("param", "exp_avg", "exp_avg_sq", "ema")


def start(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) for n in SIZES]


def grads(step):
    """The gradients of step `step` (0-based): randn times 10^(-6 + 7 step / (STEPS - 1))."""
    g = torch.Generator().manual_seed(1000 + step)
    scale = 10.0 ** (-6.0 + 7.0 * step / (STEPS - 1))
    return [torch.randn(n, generator=g) * scale for n in SIZES]


def torch_run(steps, dtype=torch.float32, state=None, first=0, divide=None):
    """torch.optim.AdamW on the CPU in `dtype` (the reference runs torch's CPU AdamW; float64: the yardstick) from the fp32 start
    - or from `state` = {kind: tensors}, `first` steps in - with the average kept beside it by ema.mul_(d).add_(p, alpha=1 - d).
    divide: every gradient is divided by it first, in `dtype`.  -> {kind: list of tensors}."""
    if state is None:
        params = [p.to(dtype).requires_grad_() for p in start()]
        emas = [p.detach().clone() for p in params]
    else:
        params = [p.detach().to(dtype).clone().requires_grad_() for p in state["param"]]
        emas = [e.to(dtype).clone() for e in state["ema"]]
    opt = torch.optim.AdamW(params, foreach=False, **HYPER)
    if state is not None:
        for p, m, v in zip(params, state["exp_avg"], state["exp_avg_sq"]):
            opt.state[p] = {"step": torch.tensor(float(first)), "exp_avg": m.to(dtype).clone(), "exp_avg_sq": v.to(dtype).clone()}
    for s in range(first, first + steps):
        for p, g in zip(params, grads(s)):
            p.grad = g.to(dtype) if divide is None else g.to(dtype) / divide
        opt.step()
        with torch.no_grad():
            for e, p in zip(emas, params):
                e.mul_(EMA_DECAY).add_(p, alpha=1 - EMA_DECAY)
    return {"param": [p.detach() for p in params], "exp_avg": [opt.state[p]["exp_avg"] for p in params],
            "exp_avg_sq": [opt.state[p]["exp_avg_sq"] for p in params], "ema": emas}


@functools.lru_cache(maxsize=None)
def reference(steps=STEPS, f64=False):
    """torch_run(steps) in fp32 or float64, computed once."""
    return torch_run(steps, torch.float64 if f64 else torch.float32)


def error(got, want64):
    """The tests' metric, per tensor: max |x - f64| / max |f64| - and the worst of a list of tensors."""
    worst = 0.0
    for x, w in zip(got, want64):
        if w.numel():
            worst = max(worst, float((x.detach().cpu().double() - w).abs().max() / w.abs().max()))
    return worst


def errors(got, want64):
    return {k: error(got[k], want64[k]) for k in KINDS if k in got}


def within_twice(mine, reference_errors, what=""):
    """The bar: for each of parameters, exp_avg, exp_avg_sq and the average, the error of the code under test is at most twice
    torch's own against the same float64 evaluation (the kernel contracts lerp's multiply-add and rounds its scalars from a
    float32 lr: at most one more rounding per output).  Prints the pairs before it judges them."""
    for k, e in mine.items():
        print(f"{what}{k}: error {e:.3e}, torch's own {reference_errors[k]:.3e}")
    return all(e <= 2.0 * reference_errors[k] for k, e in mine.items())
