#!/usr/bin/env python3
"""The INPUT gradient of the reference training step whose parameter gradients make_golden_grads.py stores (build container
only: imports the reference arch from /root/reference through the stub harness of make_golden.py; only tensors are written).

    python tests/golden/make_golden_input_grad.py        ->  tests/golden/train_grads_wf8_input.npz

The same model, weights (the `w.` tensors of train_grads_wf8.npz), batch and loss as make_golden_grads.py, with
`lq.requires_grad_()`: `g.lq` is d(l_pix + l_fft)/d lq from the reference's fp32 autograd, `t.lq` the same step in float64
(make_golden_grads.truth_f64's evaluation).  Both runs must reproduce the losses the two committed files hold, or nothing is
written.  tests/test_partial_grad_gpu.py reads it for the pattern "every parameter frozen, the input wants a gradient".
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                    # noqa: E402   (stub harness + reference import)
import make_golden_grads as mgg             # noqa: E402   (the configuration and the step)


def main():
    torch.set_num_threads(os.cpu_count())
    arch, _ = mg.import_reference_arch()
    g = np.load(os.path.join(HERE, "train_grads_wf8.npz"))
    t = np.load(os.path.join(HERE, "train_grads_wf8_f64.npz"))
    torch.manual_seed(0)
    net = arch.WaveMamba(**mgg.CFG).train()
    net.load_state_dict({k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w.")}, strict=False)
    gt = torch.from_numpy(g["gt"])

    lq = torch.from_numpy(g["lq"]).clone().requires_grad_()
    pred, l_pix, l_fft = mgg.step(net, lq, gt)
    (l_pix + l_fft).backward()
    l_pix, l_fft = l_pix.detach(), l_fft.detach()
    assert abs(float(l_pix) - g["losses"][0]) < 1e-7 and abs(float(l_fft) - g["losses"][1]) < 1e-6, \
        f"fp32 losses {float(l_pix)!r} {float(l_fft)!r} against the stored {g['losses']}"
    assert float((pred.detach() - torch.from_numpy(g["pred"])).abs().max()) < 1e-6
    # the parameter gradients of this run are the stored ones as well (same step, one more leaf)
    for k, p in net.named_parameters():
        ref = torch.from_numpy(g["g." + k])
        assert float((p.grad - ref).abs().max()) <= 1e-5 * float(ref.abs().max()) + 1e-12, k

    net64 = arch.WaveMamba(**mgg.CFG).train()
    net64.load_state_dict(net.state_dict())
    net64 = net64.double()
    lq64 = torch.from_numpy(g["lq"]).double().requires_grad_()
    saved = (torch.Tensor.float, torch.float, torch.float32)
    torch.Tensor.float = lambda self, *a, **k: self.double()
    torch.float = torch.float32 = torch.float64
    try:
        pred64, p64, f64 = mgg.step(net64, lq64, gt.double())
        assert pred64.dtype == torch.float64
        (p64 + f64).backward()
        p64, f64 = p64.detach(), f64.detach()
    finally:
        torch.Tensor.float, torch.float, torch.float32 = saved
    assert abs(float(p64) - t["losses"][0]) < 1e-12 and abs(float(f64) - t["losses"][1]) < 1e-12, \
        f"float64 losses {float(p64)!r} {float(f64)!r} against the stored {t['losses']}"
    for k, p in net64.named_parameters():
        ref = torch.from_numpy(t["t." + k])
        assert float((p.grad - ref).abs().max()) <= 1e-10 * float(ref.abs().max()) + 1e-300, k
    assert lq64.grad.dtype == torch.float64 and lq.grad.dtype == torch.float32

    path = os.path.join(HERE, "train_grads_wf8_input.npz")
    np.savez_compressed(path, **{"g.lq": mg.npy(lq.grad), "t.lq": mg.npy(lq64.grad)})
    e = float((lq.grad.double() - lq64.grad).abs().max() / lq64.grad.abs().max())
    print(f"wrote {path} ({os.path.getsize(path)} bytes); reference fp32 vs float64 input gradient: rel max {e:.3e}")


if __name__ == "__main__":
    main()
