#!/usr/bin/env python3
"""The FFT training loss (trainer.fft_l1; FFTLoss of basicsr/losses/losses.py:300-313) at the recipe's batch, 8 x 3 x 512 x 512:
forward + backward (gradient for the prediction, as in training) of the term with the "hip" backend (ops.fft_l1_mean,
csrc/fft_loss.hip.h) and with the "torch" backend (torch.fft.rfft2 of both images, ops.l1_mean over the spectra), in ONE process,
timed with device events, the two backends ALTERNATING so that neither owns a warm or a cold stretch of the run.  GPU only.

    python tools/bench_fft_loss.py [--rounds 7] [--iters 20]
A round times `iters` calls of one backend, then `iters` calls of the other.  Prints one JSON line: per backend the median, the
lowest and the highest round (ms per call), and whether the time criterion holds (the hip median does not exceed torch's)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wave_mamba_amd as wm
from wave_mamba_amd import trainer


def time_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7, help="alternations after the warm-up (at least 5)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shape", type=int, nargs=4, default=[8, 3, 512, 512])
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("--rounds: at least 5 alternations")
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1234)
    gt = torch.rand(*args.shape, generator=g).to(dev)
    pred = (gt + 0.05 * torch.randn(*args.shape, generator=g).to(dev)).clamp(0, 1).requires_grad_(True)

    def call(backend):
        def fn():
            pred.grad = None
            trainer.fft_l1(pred, gt, backend=backend).backward()
        return fn
    fns = {"hip": call("hip"), "torch": call("torch")}
    values, grads = {}, {}
    for name, fn in fns.items():                                   # warm-up: plans, allocator pools, code objects
        for _ in range(5):
            fn()
        values[name], grads[name] = float(trainer.fft_l1(pred, gt, backend=name).detach()), pred.grad.clone()
    torch.cuda.synchronize()
    ms = {"hip": [], "torch": []}
    for r in range(args.rounds):
        for name in (("hip", "torch") if r % 2 == 0 else ("torch", "hip")):
            ms[name].append(time_ms(fns[name], args.iters))
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {"what": "fft_l1 fwd+bwd " + "x".join(map(str, args.shape)), "build_id": wm._lib.build_id(), "rounds": args.rounds,
           "iters": args.iters}
    for k in ("hip", "torch"):
        res[f"{k}_ms_median"], res[f"{k}_ms_min"], res[f"{k}_ms_max"] = round(med[k], 4), round(min(ms[k]), 4), round(max(ms[k]), 4)
        res[f"{k}_ms_rounds"] = [round(v, 4) for v in ms[k]]
    res["hip_not_slower"] = med["hip"] <= med["torch"]
    res["value_hip"], res["value_torch"] = values["hip"], values["torch"]
    res["grad_rel_max_hip_vs_torch"] = float((grads["hip"] - grads["torch"]).abs().max() / grads["torch"].abs().max())
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
