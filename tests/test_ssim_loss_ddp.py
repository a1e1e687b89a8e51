"""CPU, world size 2 over gloo: trainer.GraphedDDPTrainStep(..., ssim_weight=0.25) in its eager form (capture=False) - the three
losses behind the gradients in the flat buffer, the one all-reduce, AdamW on views of the buffer - against DistributedDataParallel
+ trainer.train_step(..., ssim_weight=0.25) from the same weights.  World 2: g0/2 + g1/2 is one rounding whatever the reduction's
order, so gradients and parameters are bit-equal (as tests/test_ddp_gloo.py holds the two-term step)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

CFG = dict(in_chn=3, wf=8, n_l_blocks=[1, 1, 1], n_h_blocks=[1, 1, 1], ffn_scale=2.0)
WEIGHT = 0.25


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    import wave_mamba_amd as wm
    from oracle import oracle
    from oracle import backend as oracle_backend
    oracle.set_num_threads(2)
    oracle_backend.set_ops_backend(oracle)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        g = torch.Generator().manual_seed(78)
        lq, gt = torch.rand(2, 2, 3, 32, 32, generator=g), torch.rand(2, 2, 3, 32, 32, generator=g)    # [step][image]
        shard = slice(rank, rank + 1)
        torch.manual_seed(0)
        net_a = wm.WaveMamba(**CFG).train()
        torch.manual_seed(100 + rank)
        net_b = wm.WaveMamba(**CFG).train()
        ddp = wm.trainer.wrap_ddp(net_a)
        opt_a = wm.trainer.make_optimizer(ddp)
        if rank == 0:
            net_b.load_state_dict(net_a.state_dict())
        opt_b = wm.trainer.make_optimizer(net_b)
        step_b = wm.trainer.GraphedDDPTrainStep(net_b, opt_b, lq[0, shard], gt[0, shard], capture=False, ssim_weight=WEIGHT)
        n_grad = sum(p.numel() for p in net_b.parameters())
        rec = {"flat_numel": step_b.flat.numel(), "n_grad": n_grad, "steps": []}
        for s in range(2):
            with torch.no_grad():
                own = WEIGHT * float(wm.trainer.ssim_loss(net_b(lq[s, shard]), gt[s, shard]))     # this rank's term, before the step
            la = wm.trainer.train_step(ddp, opt_a, lq[s, shard], gt[s, shard], as_float=False, ssim_weight=WEIGHT)
            lb = step_b(lq[s, shard], gt[s, shard])
            rec["steps"].append({"own_ssim": own,
                                 "loss_a": {k: float(v) for k, v in la.items()}, "loss_b": {k: float(v) for k, v in lb.items()},
                                 "tail": step_b.flat[-3:].clone(),
                                 "grad_a": [p.grad.clone() for p in net_a.parameters()],
                                 "grad_b": [p.grad.clone() for p in net_b.parameters()],
                                 "w_a": [p.detach().clone() for p in net_a.parameters()],
                                 "w_b": [p.detach().clone() for p in net_b.parameters()]})
        torch.save(rec, os.path.join(out_dir, f"ssim{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_flat_bucket_step_with_the_ssim_term_equals_the_ddp_step(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, free_port(), str(tmp_path)), nprocs=world, join=True)
    res = [torch.load(tmp_path / f"ssim{r}.pt") for r in range(world)]
    for r in res:
        assert r["flat_numel"] == r["n_grad"] + 3                                    # gradients | l_pix | l_freq | l_ssim
    for s in range(2):
        steps = [r["steps"][s] for r in res]
        mean_ssim = sum(st["own_ssim"] for st in steps) / world
        for st in steps:
            assert set(st["loss_b"]) == {"l_pix", "l_freq", "l_ssim"} == set(st["loss_a"])
            assert st["tail"].tolist() == [st["loss_b"][k] for k in ("l_pix", "l_freq", "l_ssim")]
            for ga, gb, wa, wb, wb0 in zip(st["grad_a"], st["grad_b"], st["w_a"], st["w_b"], steps[0]["w_b"]):
                assert torch.equal(ga, gb) and torch.equal(wa, wb)
                assert torch.equal(wb, wb0)                                          # ranks stay in lock step
            # every rank holds the mean over ranks of all three losses; the reference's reduce leaves it on rank 0 only
            for k in ("l_pix", "l_freq", "l_ssim"):
                assert abs(st["loss_b"][k] - steps[0]["loss_a"][k]) <= 1e-6 * abs(steps[0]["loss_a"][k]), (s, k)
            assert abs(st["loss_b"]["l_ssim"] - mean_ssim) <= 1e-6 * abs(mean_ssim), s
        assert steps[0]["own_ssim"] != steps[1]["own_ssim"]                          # the ranks saw different images
