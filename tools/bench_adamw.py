#!/usr/bin/env python3
"""What the table-driven AdamW step (trainer.HipAdamW, csrc/adamw.hip.h) costs beside torch's fused AdamW.  GPU only; one JSON line
per measurement.

    python tools/bench_adamw.py --optimizer [--replays 200] [--rounds 5]
        a graph holding only optimizer.step() on the shipped parameter set (591 tensors, 1.51 M floats), device events around
        `replays` replays, `rounds` times, torch's fused step and the HIP step ALTERNATING round by round in one process -> us per
        replay, min / median / max over the rounds.  Variants: plain, with the guard's two device scalars, with the moving average
        (HIP only: torch has none), and plain on gradients that are views packed back to back into one flat buffer.  The HIP
        step's time is also given as a multiple of the bound: 9 floats per element (10 with the average) at 8 TB/s.
    python tools/bench_adamw.py --step torch|hip [--ema] [--replays 30] [--rounds 3]
        the config-3 graphed step (batch 8 x 3 x 512 x 512, the shipped network): ms per replay, min / median / max over the rounds.
        `--step torch` uses nothing of this feature, so the same file times a checkout of the parent commit (alternate the two)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
import wave_mamba_amd as wm

PEAK_BYTES_PER_S = 8e12


def capture(fn, dev):
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def one_round(graph, replays):
    for _ in range(10):
        graph.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / replays


def alternate(graphs, replays, rounds):
    """{name: graph} -> {name: {min, median, max}} in us per replay; every round times each graph once, in the dict's order."""
    seen = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            seen[k].append(one_round(g, replays))
    return {k: {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)} for k, v in seen.items()}


def _shipped(dev, backend, **kw):
    torch.manual_seed(0)
    net = wm.WaveMamba(**bench.SHIPPED).to(dev)
    opt = wm.trainer.make_optimizer(net, capturable=True, **({"backend": "hip", **kw} if backend == "hip" else {}))
    params = [p for grp in opt.param_groups for p in grp["params"]]
    for p in params:
        p.grad = 1e-3 * torch.randn_like(p)
    return net, opt, params


def _packed(params, dev):
    sizes = [p.numel() for p in params]
    flat = torch.zeros(sum(sizes), dtype=torch.float32, device=dev)
    views = [v.view_as(p) for v, p in zip(flat.split(sizes), params)]
    for p, v in zip(params, views):
        v.copy_(p.grad)
        p.grad = v
    return flat, views


def optimizer(args, dev):
    record = torch.tensor([1.0, 0.0, 1.0, 0.0], device=dev)
    graphs, keep = {}, []
    for variant in ("plain", "guard_scalars", "ema", "packed_views"):
        for backend in ("torch", "hip"):
            if variant == "ema" and backend == "torch":
                continue
            net, opt, params = _shipped(dev, backend, **({"ema_decay": 0.999} if variant == "ema" else {}))
            if variant == "guard_scalars":
                opt.found_inf, opt.grad_scale = record[1], record[2]
            if variant == "packed_views":
                keep.append(_packed(params, dev))
                misaligned = sum(v.data_ptr() % 16 != 0 for v in keep[-1][1])
            if backend == "hip":
                opt.prepare([p.grad for p in params])
                rows = next(iter(opt._groups[0].kept.values()))[1]
            graphs[f"{variant}_{backend}_us"] = capture(opt.step, dev)
            keep.append((net, opt))
    floats = sum(p.numel() for p in params)
    res = {"what": "optimizer step alone, torch fused and HIP alternating", "build_id": wm._lib.build_id(), "tensors": len(params),
           "floats": floats, "rows": rows, "packed_views_misaligned": misaligned, "replays": args.replays, "rounds": args.rounds}
    res.update(alternate(graphs, args.replays, args.rounds))
    for name, words in (("plain_hip_us", 9), ("ema_hip_us", 10)):
        bound_us = 1e6 * 4 * words * floats / PEAK_BYTES_PER_S
        res[name.replace("_us", "_bound_us")] = round(bound_us, 3)
        res[name.replace("_us", "_times_bound")] = round(res[name]["median"] / bound_us, 2)
    res["criterion_1_ema_hip_no_slower_than_plain_torch"] = res["ema_hip_us"]["median"] <= res["plain_torch_us"]["median"]
    print(json.dumps(res), flush=True)


def step(args, dev):
    g = torch.Generator().manual_seed(1234)
    lq, gt = torch.rand(8, 3, 512, 512, generator=g).to(dev), torch.rand(8, 3, 512, 512, generator=g).to(dev)
    torch.manual_seed(0)
    net = wm.WaveMamba(**bench.SHIPPED).train().to(dev)
    kw = {"backend": "hip", **({"ema_decay": 0.999} if args.ema else {})} if args.step == "hip" else {}
    opt = wm.trainer.make_optimizer(net, capturable=True, **kw)
    graphed = wm.trainer.GraphedTrainStep(net, opt, lq, gt)
    res = {"what": f"config-3 graphed step, optimizer backend {args.step}" + (" with the average" if args.ema else ""),
           "build_id": wm._lib.build_id(), "replays": args.replays, "rounds": args.rounds}
    res["step_us"] = alternate({"step": graphed.graph}, args.replays, args.rounds)["step"]
    res["l_pix"] = float(graphed.losses["l_pix"])
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--optimizer", action="store_true")
    ap.add_argument("--step", choices=("torch", "hip"), default=None)
    ap.add_argument("--ema", action="store_true")
    ap.add_argument("--replays", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adamw: needs a GPU")
    dev = torch.device("cuda", 0)
    if args.optimizer:
        args.replays, args.rounds = args.replays or 200, args.rounds or 5
        optimizer(args, dev)
    if args.step:
        args.replays, args.rounds = args.replays or 30, args.rounds or 3
        step(args, dev)


if __name__ == "__main__":
    main()
