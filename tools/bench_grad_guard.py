#!/usr/bin/env python3
"""What the guarded optimizer step (trainer.GradGuard, csrc/grad_guard.hip.h) costs.  GPU only; one JSON line per measurement.

    python tools/bench_grad_guard.py --launches [--replays 200] [--rounds 5]
        the shipped parameter set (591 tensors, 1.51 M floats) in flat form: a graph holding only the guard's two launches, and one
        holding only the _foreach_copy_ of the 591 gradients into the flat buffer (what GraphedTrainStep newly pays with a guard);
        device events around `replays` replays, `rounds` times -> us per replay, min / median / max over the rounds
    python tools/bench_grad_guard.py --adamw [--replays 200] [--rounds 5]
        the fused AdamW step alone on the same parameter set, captured: plain, with found_inf, with found_inf and grad_scale, with
        both on gradients that are views of a flat buffer (packed, and padded to 16 bytes), and the _foreach_sub_ over the 591 step counters that torch appends for a found_inf
    python tools/bench_grad_guard.py --step off|on [--replays 30] [--rounds 3]
        the config-3 graphed step (batch 8 x 3 x 512 x 512, the shipped network): ms per replay, min / median / max over the rounds.
        `--step off` uses nothing of the guard, so the same file times a checkout of the parent commit (alternate the two)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
import wave_mamba_amd as wm


def replay_us(graph, replays, rounds):
    out = []
    for _ in range(rounds):
        for _ in range(10):
            graph.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(replays):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(1e3 * e0.elapsed_time(e1) / replays)
    return {"min": round(min(out), 3), "median": round(statistics.median(out), 3), "max": round(max(out), 3)}


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


def launches(args, dev):
    torch.manual_seed(0)
    net = wm.WaveMamba(**bench.SHIPPED).to(dev)
    params = [p for p in net.parameters() if p.requires_grad]
    sizes = [p.numel() for p in params]
    grads = [torch.randn_like(p) for p in params]
    flat = torch.zeros(sum(sizes), dtype=torch.float32, device=dev)
    views = [v.view_as(p) for v, p in zip(flat.split(sizes), params)]
    torch._foreach_copy_(views, grads)
    record, skipped = torch.empty(4, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    table = wm.ops.grad_guard_table([flat])
    per_tensor = wm.ops.grad_guard_table(grads)
    res = {"what": "guard launches alone", "build_id": wm._lib.build_id(), "tensors": len(params), "floats": sum(sizes),
           "rows_flat": table[1], "rows_per_tensor": per_tensor[1], "replays": args.replays, "rounds": args.rounds}
    res["guard_flat_us"] = replay_us(capture(lambda: wm.ops.grad_guard(table, 1.0, record, skipped), dev), args.replays, args.rounds)
    res["guard_per_tensor_us"] = replay_us(capture(lambda: wm.ops.grad_guard(per_tensor, 1.0, record, skipped), dev), args.replays,
                                           args.rounds)
    res["foreach_copy_us"] = replay_us(capture(lambda: torch._foreach_copy_(views, grads), dev), args.replays, args.rounds)
    from wave_mamba_amd import cpu_twin
    res["norm"], res["twin_norm"] = float(record[0]), float(cpu_twin.grad_guard([flat])[0])
    print(json.dumps(res), flush=True)


def step(args, dev):
    g = torch.Generator().manual_seed(1234)
    lq, gt = torch.rand(8, 3, 512, 512, generator=g).to(dev), torch.rand(8, 3, 512, 512, generator=g).to(dev)
    torch.manual_seed(0)
    net = wm.WaveMamba(**bench.SHIPPED).train().to(dev)
    opt = wm.trainer.make_optimizer(net, capturable=True)
    kw = {"guard": wm.trainer.GradGuard(max_norm=1.0)} if args.step == "on" else {}
    graphed = wm.trainer.GraphedTrainStep(net, opt, lq, gt, **kw)
    res = {"what": f"config-3 graphed step, guard {args.step}", "build_id": wm._lib.build_id(), "replays": args.replays,
           "rounds": args.rounds, "step_us": replay_us(graphed.graph, args.replays, args.rounds)}
    if kw:
        res["norm"], res["skipped"] = float(kw["guard"].norm), int(kw["guard"].skipped)
        # the gradient copy in situ: the gradients as autograd leaves them (their own strides), into views of a flat buffer
        params = [p for grp in opt.param_groups for p in grp["params"]]
        for p in params:
            p.grad = None
        wm.trainer._total(wm.trainer.losses(net(lq), gt)).backward()
        grads = [p.grad for p in params]
        flat = torch.zeros(sum(p.numel() for p in params), dtype=torch.float32, device=dev)
        views = [v.view_as(p) for v, p in zip(flat.split([p.numel() for p in params]), params)]
        res["grads_with_other_strides"] = sum(v.stride() != g.stride() for v, g in zip(views, grads))
        res["foreach_copy_us"] = replay_us(capture(lambda: torch._foreach_copy_(views, grads), dev), 200, args.rounds)
    print(json.dumps(res), flush=True)


def adamw(args, dev):
    """optimizer.step() alone, captured, on the shipped parameter set: plain, with found_inf, with found_inf and grad_scale - and
    the step-counter correction torch's fused AdamW appends when it is given a found_inf (_foreach_sub_ over the 591 counters)."""
    torch.manual_seed(0)
    net = wm.WaveMamba(**bench.SHIPPED).to(dev)
    opt = wm.trainer.make_optimizer(net, capturable=True)
    params = [p for grp in opt.param_groups for p in grp["params"]]
    for p in params:
        p.grad = 1e-3 * torch.randn_like(p)
    record = torch.tensor([1.0, 0.0, 1.0, 0.0], device=dev)
    res = {"what": "fused AdamW step alone", "build_id": wm._lib.build_id(), "tensors": len(params), "replays": args.replays,
           "rounds": args.rounds}
    res["plain_us"] = replay_us(capture(opt.step, dev), args.replays, args.rounds)
    opt.found_inf = record[1]
    res["found_inf_us"] = replay_us(capture(opt.step, dev), args.replays, args.rounds)
    opt.grad_scale = record[2]
    res["found_inf_grad_scale_us"] = replay_us(capture(opt.step, dev), args.replays, args.rounds)
    # the same step on gradients that are views of one flat buffer (GraphedTrainStep / GraphedDDPTrainStep with a guard): packed, so
    # that a view starts at any 4-byte offset, and with every view's start padded to 16 bytes
    sizes = [p.numel() for p in params]
    for name, slots in (("flat_views_packed_us", sizes), ("flat_views_16B_us", [(n + 3) // 4 * 4 for n in sizes])):
        flat = torch.zeros(sum(slots), dtype=torch.float32, device=dev)
        views = [v[:n].view_as(p) for v, n, p in zip(flat.split(slots), sizes, params)]
        res[name.replace("_us", "_misaligned")] = sum(v.data_ptr() % 16 != 0 for v in views)
        for p, v in zip(params, views):
            v.copy_(1e-3 * torch.randn_like(p))
            p.grad = v
        res[name] = replay_us(capture(opt.step, dev), args.replays, args.rounds)
    steps = [opt.state[p]["step"] for p in params]
    res["foreach_sub_us"] = replay_us(capture(lambda: torch._foreach_sub_(steps, [record[1]] * len(steps)), dev), args.replays, args.rounds)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--adamw", action="store_true")
    ap.add_argument("--step", choices=("off", "on"), default=None)
    ap.add_argument("--replays", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_grad_guard: needs a GPU")
    dev = torch.device("cuda", 0)
    if args.launches:
        args.replays, args.rounds = args.replays or 200, args.rounds or 5
        launches(args, dev)
    if args.adamw:
        args.replays, args.rounds = args.replays or 200, args.rounds or 5
        adamw(args, dev)
    if args.step:
        args.replays, args.rounds = args.replays or 30, args.rounds or 3
        step(args, dev)


if __name__ == "__main__":
    main()
