"""bench.py's plain run and --dump-outputs: the arguments a plain run takes, the arrays it writes (float32, at most 64 MB,
the same sample positions on every run) and - on the GPU - that what a plain run dumps is the timed path's output on the
seeded inputs, checked against the CPU-oracle network."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_the_default():
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.full is False and a.dump_outputs is None
    a = bench.parse_args(["--steps", "3", "--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def test_dump_outputs_small_whole_large_sampled(tmp_path):
    import bench
    g = torch.Generator().manual_seed(0)
    big = torch.rand(1, 3, 2176, 3840, generator=g)[:, :, :2160, :3840]          # the UHD output, cropped as bench.step does
    small = torch.rand(1, 3, 40, 56, generator=g, dtype=torch.float64)
    w = bench.dump_outputs(str(tmp_path / "a"), {"output": big, "small": small})
    assert set(w) == {"output_sample.npy", "small.npy"} and "sample" in w["output_sample.npy"]
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and s.shape == (1, 3, 40, 56) and np.array_equal(s, small.float().numpy())
    o = np.load(tmp_path / "a" / "output_sample.npy")
    assert o.dtype == np.float32 and o.shape == (bench.DUMP_MAX_ELEMENTS,)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 * 2 ** 20
    # the sampled positions depend on the shape alone: a second run picks the same elements
    bench.dump_outputs(str(tmp_path / "b"), {"output": big.clone()})
    assert np.array_equal(np.load(tmp_path / "b" / "output_sample.npy"), o)
    flat = big.reshape(-1).numpy()
    idx = torch.randperm(big.numel(), generator=torch.Generator().manual_seed(bench.DUMP_SAMPLE_SEED))
    assert np.array_equal(o, flat[idx[:bench.DUMP_MAX_ELEMENTS].sort().values.numpy()])


@pytest.mark.gpu
def test_plain_run_line_and_dumped_output(tmp_path):
    """A plain run at a small size: one JSON line with the headline fields and none of the --full legs, and the dumped array
    is the forward of the seeded network on the seeded image (the CPU-oracle network on the same inputs, 1e-4)."""
    import bench
    from oracle import oracle
    from oracle import backend as oracle_backend
    h, w = 136, 200                                                  # reflect-padded to 256 x 256, cropped back
    out = tmp_path / "dump"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
        os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
        "--height", str(h), "--width", str(w), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["metric"] == "UHD (3840x2160) images/sec fwd" and line["unit"] == "images/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32" and line["steps"] == 3
    assert line["ms_per_step"] > 0 and abs(line["value"] - 1e3 / line["ms_per_step"]) <= 1e-6 * line["value"]
    for leg in ("roofline", "cpu_baseline", "roofline_table", "training_config3_one_gpu"):
        assert leg not in line
    assert list(line["outputs"]["arrays"]) == ["output.npy"]
    got = torch.from_numpy(np.load(out / "output.npy"))
    assert got.dtype == torch.float32 and got.shape == (1, 3, h, w)

    img = torch.rand(1, 3, h, w, generator=torch.Generator().manual_seed(bench.image_seed(0)))
    net = bench.build_model("cpu")
    with oracle_backend.ops_backend(oracle), torch.no_grad():
        want = net.restoration_network(bench.pad_to(img))[:, :, :h, :w]
    assert_close(got, want, 1e-4, "bench --dump-outputs vs CPU-oracle network")
