#!/usr/bin/env python3
"""What does recipe.Trainer's distributed mode cost at world 1?  Iterations per second of `Trainer.run` in three forms, by the
protocol of profiles/recipe/README.md section 1: the shipped configuration and recipe (tests/golden/train_wavemamba_uhdll.yml),
batch 8 x 3 x 512 x 512 formed by PairedPatchBatcher from 32 resident uint8 pairs of 600 x 720, windows of 30 iterations between
two device synchronisations timed with the host clock, five warm-up iterations per loop (they include the capture), the loops
alternating in ONE process, four rounds.  No checkpoint, no validation, print_freq 100.

    single    the single-process graphed loop (GraphedTrainStep): the baseline
    split     distributed=True on a one-rank RCCL communicator, the all-reduce between the two replays
    captured  the same, the all-reduce inside the one graph

The process holds a one-rank `nccl` group throughout (the single-process loop ignores it).  With --world N > 1 (default: the
number of GPUs the machine shows, when there is more than one) N ranks are spawned afterwards, one GPU each, and time the mode's
loop (--collective) the same way: images/s = N x 8 x iterations/s of the slowest rank.  GPU only.  Prints the table and one JSON
line; --out FILE writes the JSON there too.

    python tools/bench_recipe_loop.py [--rounds 4] [--window 30] [--world N] [--collective split] [--out FILE]"""
import argparse
import copy
import json
import os
import socket
import statistics
import sys
import tempfile
import time
from datetime import timedelta

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import wave_mamba_amd as wm
from wave_mamba_amd import recipe
from wave_mamba_amd.data import DeviceImageStore

YAML = os.path.join(ROOT, "tests", "golden", "train_wavemamba_uhdll.yml")
PAIRS, H, W, WARMUP = 32, 600, 720, 5


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def make_store(device, seed=0):
    rng = np.random.default_rng(seed)
    store = DeviceImageStore(device)
    for _ in range(PAIRS):
        gt = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        store.add((gt // 3 + rng.integers(0, 8, (H, W, 3), dtype=np.uint8)).astype(np.uint8), gt)
    return store


def options():
    opt, _ = recipe.load_options(YAML)
    opt = copy.deepcopy(opt)
    opt["logger"].update(print_freq=100, save_checkpoint_freq=10 ** 9, save_latest_freq=None)
    opt["path"] = {"pretrain_network_g": None, "strict_load": True, "resume_state": None}
    opt["val"] = None
    return opt


def window(trainer, iters, device):
    """Seconds for `iters` more iterations of trainer.run between two device synchronisations."""
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    out = trainer.run(max_iters=iters)
    torch.cuda.synchronize(device)
    assert not out["finished"], "the recipe ended inside a timed window"
    return time.perf_counter() - t0


def ranked(rank, world, port, args, out_dir):
    """One rank of the --world run: the mode's loop on GPU `rank`, the same windows; the slowest rank's time counts."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    device = torch.device("cuda", rank)
    torch.cuda.set_device(device)
    dist.init_process_group("nccl", device_id=device, rank=rank, world_size=world, timeout=timedelta(seconds=600))
    try:
        t = recipe.Trainer(options(), make_store(device), graphed=True, out_dir=os.path.join(out_dir, f"world{world}"),
                           collective=args.collective)
        assert t.distributed and t.world == world
        t.run(max_iters=WARMUP)
        rates = []
        for _ in range(args.rounds):
            secs = torch.tensor([window(t, args.window, device)], dtype=torch.float64, device=device)
            dist.all_reduce(secs, op=dist.ReduceOp.MAX)
            rates.append(args.window / float(secs))
        if rank == 0:
            with open(os.path.join(out_dir, "world.json"), "w", encoding="utf-8") as f:
                json.dump(rates, f)
    finally:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--window", type=int, default=30)
    ap.add_argument("--world", type=int, default=None)
    ap.add_argument("--collective", choices=("split", "captured"), default="split")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_recipe_loop: needs a GPU")
    gpus = torch.cuda.device_count()
    world = args.world if args.world is not None else (gpus if gpus > 1 else 1)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    res = {"what": "recipe.Trainer.run, shipped config, batch 8x3x512x512: iterations/s per 30-iteration window",
           "build_id": wm._lib.build_id(), "device": torch.cuda.get_device_name(0), "gpus": gpus, "window": args.window}
    with tempfile.TemporaryDirectory() as tmp:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
        dist.init_process_group("nccl", device_id=device, rank=0, world_size=1, timeout=timedelta(seconds=600))
        try:
            store = make_store(device)
            loops = {"single": recipe.Trainer(options(), store, graphed=True, out_dir=os.path.join(tmp, "single"))}
            for collective in ("split", "captured"):
                loops[collective] = recipe.Trainer(options(), store, graphed=True, out_dir=os.path.join(tmp, collective),
                                                   distributed=True, collective=collective)
            assert not loops["single"].distributed and loops["split"].distributed and loops["captured"].distributed
            for t in loops.values():
                t.run(max_iters=WARMUP)
            rates = {name: [] for name in loops}
            for _ in range(args.rounds):
                for name, t in loops.items():
                    rates[name].append(args.window / window(t, args.window, device))
        finally:
            dist.destroy_process_group()
        del loops, store
        torch.cuda.empty_cache()
        res["rates"] = {k: [round(v, 3) for v in vs] for k, vs in rates.items()}
        res["median"] = {k: round(statistics.median(vs), 3) for k, vs in rates.items()}
        res["ms_per_iter"] = {k: round(1e3 / statistics.median(vs), 2) for k, vs in rates.items()}
        res["spread"] = {k: round((max(vs) - min(vs)) / statistics.median(vs), 4) for k, vs in rates.items()}
        if world > 1:
            import torch.multiprocessing as mp
            mp.spawn(ranked, args=(world, free_port(), args, tmp), nprocs=world, join=True)
            with open(os.path.join(tmp, "world.json"), encoding="utf-8") as f:
                per = json.load(f)
            res["world"] = {"ranks": world, "collective": args.collective, "rates": [round(v, 3) for v in per],
                            "images_per_s": round(world * 8 * statistics.median(per), 1)}
    print("| round | " + " | ".join(res["rates"]) + " |")
    print("|---|" + "---|" * len(res["rates"]))
    for i in range(args.rounds):
        print(f"| {i + 1} | " + " | ".join(f"{res['rates'][k][i]:.3f}" for k in res["rates"]) + " |")
    print("| median | " + " | ".join(f"**{res['median'][k]:.2f}**" for k in res["rates"]) + " |")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
