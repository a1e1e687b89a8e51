"""GPU: the FFT training loss on its HIP kernels (ops.fft_l1_mean, csrc/fft_loss.hip.h; FFTLoss of basicsr/losses/losses.py:300-313)
against the float64 truth of the reference composition, and the facts around it: exact zeros, the target's gradient, repeated calls
in both modes, graph replays, the trainer's `fft_backend` and the torch.library op.  Cases and bars: tests/fft_loss_cases.py - every
gradient comparison asserts first that no spectrum bin of its input is weak."""
import pytest
import torch

from conftest import rel_err
import fft_loss_cases as fc
import wave_mamba_amd as wm
from wave_mamba_amd import trainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL = dict(in_chn=3, wf=8, n_l_blocks=[1, 1, 1], n_h_blocks=[1, 1, 1], ffn_scale=2.0)


def hip_value_and_grads(pred, target, scale=None, need=(True, True)):
    p = pred.detach().clone().to(DEV).requires_grad_(need[0])
    t = target.detach().clone().to(DEV).requires_grad_(need[1])
    v = wm.ops.fft_l1_mean(p, t)
    assert v.dtype == torch.float32 and v.dim() == 0 and v.is_cuda
    (v if scale is None else scale * v).backward()
    return v.detach(), p.grad, t.grad


@pytest.mark.parametrize("c", fc.all_cases(), ids=fc.case_id)
def test_value_and_gradient_against_float64(c):
    d = fc.case(*c)
    v, gp, _ = hip_value_and_grads(d["pred"], d["target"], need=(True, False))
    fc.check_value_and_grad(c, float(v), gp.cpu(), "hip")


def test_identical_inputs_give_exact_zeros():
    x = torch.rand(2, 3, 32, 64, generator=torch.Generator().manual_seed(3)).to(DEV).requires_grad_(True)
    v = wm.ops.fft_l1_mean(x, x)
    v.backward()
    assert float(v) == 0.0 and bool((x.grad == 0).all())
    v, gp, gt = hip_value_and_grads(x, x.detach().clone())
    assert float(v) == 0.0 and bool((gp == 0).all()) and bool((gt == 0).all())


def test_the_target_s_gradient_is_the_negative_and_the_upstream_gradient_scales():
    pred, target = fc.flat_pair(1, 2, 64, 128, seed=fc.FLAT_SEED)
    v, gp, gt = hip_value_and_grads(pred, target)
    assert torch.equal(gt, -gp) and float(gp.abs().max()) > 0
    v2, none, gt_only = hip_value_and_grads(pred, target, need=(False, True))
    assert none is None and torch.equal(gt_only, gt) and torch.equal(v2, v)
    _, gp_only, none = hip_value_and_grads(pred, target, need=(True, False))
    assert none is None and torch.equal(gp_only, gp)
    _, g3, _ = hip_value_and_grads(pred, target, scale=3.0)
    want = 3.0 * gp
    inf = torch.full_like(want, float("inf"))
    assert bool(((g3 >= torch.nextafter(want, -inf)) & (g3 <= torch.nextafter(want, inf))).all())       # within 1 ulp
    assert not torch.equal(g3, gp)


def test_two_calls_and_both_modes_give_the_same_bits():
    pred, target = fc.flat_pair(2, 3, 128, 64, seed=11)
    first = hip_value_and_grads(pred, target)
    again = hip_value_and_grads(pred, target)
    prev = wm.set_deterministic(True)
    try:
        det = hip_value_and_grads(pred, target)
    finally:
        wm.set_deterministic(prev)
    for other in (again, det):
        assert all(torch.equal(a, b) for a, b in zip(first, other))


def test_backward_twice_from_one_record():
    pred, target = fc.flat_pair(1, 2, 64, 64, seed=12)
    p = pred.to(DEV).requires_grad_(True)
    v = wm.ops.fft_l1_mean(p, target.to(DEV))
    g1, = torch.autograd.grad(v, p, retain_graph=True)
    g2, = torch.autograd.grad(v, p, retain_graph=True)
    assert torch.equal(g1, g2) and float(g1.abs().max()) > 0


def test_bf16_and_non_contiguous_inputs_are_converted_like_ssim_mean_s():
    pred, target = fc.flat_pair(1, 2, 32, 32, seed=13)
    pb, tb = pred.bfloat16().to(DEV), target.bfloat16().to(DEV)
    want = hip_value_and_grads(pb.float(), tb.float(), need=(True, False))
    p = pb.clone().requires_grad_(True)
    v = wm.ops.fft_l1_mean(p, tb)
    v.backward()
    assert v.dtype == torch.float32 and p.grad.dtype == torch.bfloat16
    assert torch.equal(v.detach(), want[0]) and torch.equal(p.grad, want[1].bfloat16())
    pt = pred.to(DEV).transpose(2, 3)
    assert not pt.is_contiguous()
    want = hip_value_and_grads(pt.contiguous(), target, need=(True, False))
    p = pt.detach().requires_grad_(True)
    v = wm.ops.fft_l1_mean(p, target.to(DEV))
    v.backward()
    assert torch.equal(v.detach(), want[0]) and torch.equal(p.grad, want[1])


UNSUPPORTED = [(1, 1, 24, 40), (1, 1, 8, 16), (1, 1, 2048, 16)]


@pytest.mark.parametrize("shape", UNSUPPORTED, ids=["x".join(map(str, s)) for s in UNSUPPORTED])
def test_unsupported_shapes_raise_in_ops_and_fall_back_in_the_trainer(shape):
    pred, target = (t.to(DEV) for t in fc.randn_pair(shape, 5))
    assert not wm.ops.fft_l1_supported(*shape[2:])
    with pytest.raises(RuntimeError, match=r"powers of two in \[16, 1024\]"):
        wm.ops.fft_l1_mean(pred, target)

    def run(**kw):
        p = pred.clone().requires_grad_(True)
        v = trainer.fft_l1(p, target, **kw)
        v.backward()
        return v.detach(), p.grad
    v0, g0 = run()
    v1, g1 = run(backend="hip")
    assert torch.equal(v0, v1)
    assert float((g0 - g1).abs().max()) <= 1e-6


def _eager_noise():
    """What a training loop does between two replays: kernels and allocations of its own."""
    for n, v in ((8, float("nan")), (320, 1e30), (65536, float("nan")), (1 << 20, 1e30)):
        t = torch.full((n,), v, device=DEV)
        del t
    torch.cuda.synchronize()


def test_graph_replays_with_eager_work_between_them():
    shape = (2, 3, 64, 64)
    ps = torch.zeros(shape, device=DEV).requires_grad_(True)
    ts = torch.zeros(shape, device=DEV)
    first = fc.flat_pair(*shape, seed=20)
    with torch.no_grad():
        ps.copy_(first[0])
        ts.copy_(first[1])
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        for _ in range(2):
            torch.autograd.grad(wm.ops.fft_l1_mean(ps, ts), ps)
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        v = wm.ops.fft_l1_mean(ps, ts)
        g, = torch.autograd.grad(v, ps)
    for seed in (21, 22, 23):
        pred, target = fc.flat_pair(*shape, seed=seed)
        want_v, want_g, _ = hip_value_and_grads(pred, target, need=(True, False))
        with torch.no_grad():
            ps.copy_(pred)
            ts.copy_(target)
        graph.replay()
        assert torch.equal(v.detach(), want_v) and torch.equal(g, want_g), f"replay with seed {seed}"
        assert float(want_g.abs().max()) > 0
        _eager_noise()


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------
def _state_and_batch(seed):
    torch.manual_seed(0)
    state = {k: v.clone() for k, v in wm.WaveMamba(**SMALL).state_dict().items()}
    gg = torch.Generator().manual_seed(seed)
    return state, torch.rand(2, 3, 64, 64, generator=gg).to(DEV), torch.rand(2, 3, 64, 64, generator=gg).to(DEV)


def _net(state):
    net = wm.WaveMamba(**SMALL).train().to(DEV)
    net.load_state_dict(state)
    return net


def test_train_step_with_the_hip_backend_reports_the_same_losses():
    """(In the deterministic mode: outside it ops.l1_mean adds its workgroup sums in completion order, and l_pix of two runs of ONE
    path already differs in the last bit.)"""
    state, lq, gt = _state_and_batch(31)
    got = {}
    prev = wm.set_deterministic(True)
    try:
        for backend in (None, "hip"):
            net = _net(state)
            got[backend] = trainer.train_step(net, trainer.make_optimizer(net), lq, gt, as_float=False, fft_backend=backend)
    finally:
        wm.set_deterministic(prev)
    assert torch.equal(got[None]["l_pix"], got["hip"]["l_pix"])
    a, b = float(got[None]["l_freq"]), float(got["hip"]["l_freq"])
    print(f"l_freq: torch {a!r} hip {b!r} rel {abs(a - b) / abs(a):.2e}")
    assert abs(a - b) <= fc.value_bar(0.0) * abs(a)


def test_losses_with_the_hip_backend_meet_the_gradient_bar():
    c = ("flat", (2, 3, 64, 64), fc.FLAT_SEED)
    d = fc.case(*c)
    fc.check_margin(c)
    p = d["pred"].to(DEV).requires_grad_(True)
    terms = trainer.losses(p, d["target"].to(DEV), fft_backend="hip")
    assert len(terms) == 2
    g, = torch.autograd.grad(terms[1], p)
    ev, eg = abs(float(terms[1]) - 0.1 * d["value"]) / (0.1 * d["value"]), rel_err(g, 0.1 * d["gpred"])[1]
    print(f"losses(fft_backend='hip'): value rel err {ev:.2e}, gradient max rel err {eg:.2e} (bar {fc.grad_bar(d['e_grad']):.1e})")
    assert ev <= fc.value_bar(d["e_value"]) and eg <= fc.grad_bar(d["e_grad"])
    prev = wm.set_fft_loss("hip")
    try:
        by_default = trainer.losses(p, d["target"].to(DEV))
    finally:
        wm.set_fft_loss(prev)
    assert torch.equal(by_default[1].detach(), terms[1].detach())


def _three_eager_steps(state, lq, gt):
    net = _net(state)
    opt = trainer.make_optimizer(net)
    for _ in range(3):
        losses = trainer.train_step(net, opt, lq, gt, as_float=False, ssim_weight=0.25, fft_backend="hip")
    return [p.detach().clone() for p in net.parameters()], {k: v.clone() for k, v in losses.items()}


def _three_replays(state, lq, gt):
    net = _net(state)
    step = trainer.GraphedTrainStep(net, trainer.make_optimizer(net, capturable=True), lq, gt, ssim_weight=0.25, fft_backend="hip")
    for _ in range(3):
        losses = step(lq, gt)
        assert bool(torch.isfinite(losses["l_freq"]))                      # an eager launch (and a host read) between replays
    torch.cuda.synchronize()
    return [p.detach().clone() for p in net.parameters()], {k: v.clone() for k, v in losses.items()}


@pytest.mark.parametrize("run", [_three_eager_steps, _three_replays], ids=["eager", "graphed"])
def test_deterministic_steps_with_the_hip_backend_are_bit_equal(run):
    state, lq, gt = _state_and_batch(32)
    prev = wm.set_deterministic(True)
    try:
        w1, l1 = run(state, lq, gt)
        w2, l2 = run(state, lq, gt)
    finally:
        wm.set_deterministic(prev)
    assert len(l1) == 3 and all(bool(torch.isfinite(v)) for v in l1.values())
    bad = sum(not torch.equal(a, b) for a, b in zip(w1, w2))
    assert bad == 0, f"{bad} of {len(w1)} weight tensors differ"
    assert all(torch.equal(l1[k], l2[k]) for k in l1), (l1, l2)


# ---- the torch.library op ---------------------------------------------------------------------------------------------------------------
def test_torch_library_op_gives_the_bits_of_ops_fft_l1_mean():
    import wave_mamba_amd.torch_ops  # noqa: F401
    pred, target = fc.flat_pair(2, 3, 32, 128, seed=14)
    want = hip_value_and_grads(pred, target, scale=0.5)
    p, t = pred.to(DEV).requires_grad_(True), target.to(DEV).requires_grad_(True)
    v = torch.ops.wavemamba_hip.fft_l1_mean(p, t)
    (0.5 * v).backward()
    assert torch.equal(v.detach(), want[0]) and torch.equal(p.grad, want[1]) and torch.equal(t.grad, want[2])
