#!/usr/bin/env python3
"""Host-to-host images/s of wave_mamba_amd.inference.UInt8Pipeline.run on synthetic uint8 images, per image size, in four
configurations that alternate in one process:

    default      UInt8Pipeline(net, dev)                              one eager forward per image (the behaviour before the switches)
    graphed      UInt8Pipeline(net, dev, graphed=True)                pre -> forward -> post replayed from a graph, batch 1
    graphed_b4   UInt8Pipeline(net, dev, graphed=True, batch=4)       four images per replay
    ensemble     UInt8Pipeline(net, dev, graphed=True, ensemble=True) eight transforms per image: two batch-4 forwards per replay

A window is one run() over `count` images between two device synchronisations, timed with the host clock; every configuration is
warmed up (both slots captured) before the first round, and the rounds alternate the configurations.  Per size the tool prints the
rates per round, medians and ranges, the per-round ratios to `default` (rate over default's rate; for the ensemble 8 x its rate
over default's rate, that is the time of eight default forwards over the ensemble's time per image: 1.0 when an ensembled image
costs exactly eight default images, above 1 when it costs less), the host time of one weight-signature check (what every graphed
launch pays to notice changed weights), and how the outputs compare: `graphed` must equal `default` bit for bit; for `graphed_b4` the number of differing uint8 values is counted.
One JSON line per size goes to --out.  GPU only; shipped configuration (wf = 32)."""
import argparse, json, os, statistics, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wave_mamba_amd as wm
from wave_mamba_amd import inference

CONFIGS = {"default": {}, "graphed": {"graphed": True}, "graphed_b4": {"graphed": True, "batch": 4},
           "ensemble": {"graphed": True, "ensemble": True}}
# images per window (multiples of 4: full batches only) for the three single-forward configurations, and for the ensemble
COUNTS = {(400, 600): (96, 12), (720, 1280): (48, 8), (1080, 1920): (32, 4), (2160, 3840): (12, 3)}


def window(pipe, imgs, count):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = sum(1 for _ in pipe.run(imgs[i % len(imgs)] for i in range(count)))
    torch.cuda.synchronize()
    assert n == count
    return count / (time.perf_counter() - t0)


def spread(v):
    return f"{statistics.median(v):.2f} ({min(v):.2f} - {max(v):.2f})"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="600x400,1280x720,1920x1080,3840x2160", help="width x height, comma separated")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--out", default=None, help="append one JSON line per size to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_inference_pipeline: needs a GPU")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = wm.WaveMamba(in_chn=3, wf=32, n_l_blocks=[1, 2, 4], n_h_blocks=[1, 1, 2], ffn_scale=2.0).eval().to(dev)
    rng = np.random.default_rng(0)
    names = a.configs.split(",")
    t0 = time.perf_counter()
    for _ in range(200):
        inference._weights_signature(net)
    sig_us = 1e6 * (time.perf_counter() - t0) / 200
    print(f"weight-signature check ({sum(1 for _ in net.parameters())} parameters): {sig_us:.0f} us per graphed launch", flush=True)
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        count, count_ens = COUNTS.get((h, w), (16, 4))
        imgs = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for _ in range(4)]
        pipes = {n: inference.UInt8Pipeline(net, dev, **CONFIGS[n]) for n in names}
        outs = {n: list(p.run(imgs + imgs)) for n, p in pipes.items()}           # warm-up: eight images, both slots of every batch size
        rates = {n: [] for n in names}
        for _ in range(a.rounds):
            for n in names:
                rates[n].append(window(pipes[n], imgs, count_ens if n == "ensemble" else count))
        rec = {"size": size, "rounds": a.rounds, "signature_check_us": sig_us, "images_per_window": {n: (count_ens if n == "ensemble" else count) for n in names},
               "images_per_s": rates, "captures": {n: pipes[n].captures for n in names}}
        print(f"== {size}: images/s per round, median (min - max)")
        for n in names:
            print(f"  {n:11s} " + "  ".join(f"{r:8.2f}" for r in rates[n]) + f"   {spread(rates[n])}")
        if "default" in names:
            rec["ratio_to_default"] = {}
            for n in names:
                if n == "default":
                    continue
                scale = 8.0 if n == "ensemble" else 1.0                          # the ensemble: against eight default forwards
                ratio = [scale * r / d for r, d in zip(rates[n], rates["default"])]
                rec["ratio_to_default"][n] = ratio
                what = "eight default forwards' time over the ensemble's" if n == "ensemble" else "rate over default's"
                print(f"  {n:11s} {what}, per round: " + "  ".join(f"{r:.3f}" for r in ratio) + f"   {spread(ratio)}")
            d = statistics.median(rates["default"])
            lo, hi = min(rates["default"]), max(rates["default"])
            print(f"  default spread between rounds: {100 * (hi - lo) / d:.1f} %")
            if "graphed" in names:
                rec["graphed_equals_default"] = all(np.array_equal(x, y) for x, y in zip(outs["graphed"], outs["default"]))
                print(f"  graphed == default bit for bit: {rec['graphed_equals_default']}")
            if "graphed_b4" in names:
                diff = [np.abs(x.astype(np.int16) - y.astype(np.int16)) for x, y in zip(outs["graphed_b4"], outs["default"])]
                rec["b4_differing_values"] = int(sum((v != 0).sum() for v in diff))
                rec["b4_values"] = int(sum(v.size for v in diff))
                rec["b4_max_difference"] = int(max(v.max() for v in diff))
                print(f"  graphed_b4 against default: {rec['b4_differing_values']} of {rec['b4_values']} uint8 values differ, by at most "
                      f"{rec['b4_max_difference']}")
        rec["max_memory_allocated_gib"] = torch.cuda.max_memory_allocated(dev) / 2 ** 30
        rec["max_memory_reserved_gib"] = torch.cuda.max_memory_reserved(dev) / 2 ** 30
        print(f"  peak device memory so far: {rec['max_memory_allocated_gib']:.1f} GiB allocated, {rec['max_memory_reserved_gib']:.1f} GiB "
              "reserved (all four pipelines of a size alive at once)", flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")
        del pipes, outs
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
