"""GPU: the SSIM training loss on its HIP kernels (ops.ssim_mean, csrc/ssim_loss.hip.h; cal_ssim.SSIM() of femasr_model.py:29)
against the reference's float64 values and gradients (tests/golden/ssim_loss.npz), a float64 evaluation written out here for the
tile-edge shapes, repeated calls, graph replays, the graphed training step and the torch.library op.

Bars (the same as tests/test_ssim_loss_cpu.py): |SSIM - SSIM_f64| <= 1e-5, or 2 x the reference's float32 error where that
exceeds 5e-6; gradients per tensor, l2- and max-abs-relative to the truth, <= truth_bar(reference float32 error) - for the
shapes evaluated here, where no float32 reference is at hand, truth_bar(0) = 1e-4.  `equal`: |1 - SSIM| <= 1e-6, finite
gradients no larger than 1e-4 of the `noise` case's."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from test_ssim_loss_cpu import check_case, noise_max_of, ssim_golden, truth_bar
import wave_mamba_amd as wm
from wave_mamba_amd import trainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TH, TW = wm.ops.SSIM_TILE_H, wm.ops.SSIM_TILE_W               # one workgroup per TH x TW tile (csrc/ssim_loss.hip.h)


def ssim_f64(pred, gt):
    """cal_ssim's definition in float64 on the CPU, the 2-D way: (SSIM, d/dpred, d/dgt).  The window is the float32 outer
    product of the float32 taps, as the reference builds it; zero padding of 5."""
    a = pred.detach().cpu().double().requires_grad_(True)
    b = gt.detach().cpu().double().requires_grad_(True)
    C = a.shape[1]
    g = torch.tensor([-(i - 5) ** 2 / 4.5 for i in range(11)], dtype=torch.float64).exp().float()
    g = g / g.sum()
    w = torch.outer(g, g).double().expand(C, 1, 11, 11).contiguous()
    blur = lambda t: F.conv2d(t, w, padding=5, groups=C)
    mu1, mu2 = blur(a), blur(b)
    s1, s2, s12 = blur(a * a) - mu1 ** 2, blur(b * b) - mu2 ** 2, blur(a * b) - mu1 * mu2
    s = (((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 ** 2 + mu2 ** 2 + 1e-4) * (s1 + s2 + 9e-4))).mean()
    ga, gb = torch.autograd.grad(s, (a, b))
    return float(s), ga, gb


def noise_pair(shape, seed):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(shape, generator=g)
    return (gt + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1).to(DEV), gt.to(DEV)


@pytest.mark.parametrize("case", sorted(ssim_golden()))
def test_golden_cases_through_ops_ssim_mean(case):
    cases = ssim_golden()
    d = cases[case]
    p, t = d["pred"].to(DEV).requires_grad_(True), d["gt"].to(DEV).requires_grad_(True)
    s = wm.ops.ssim_mean(p, t)
    assert s.dtype == torch.float32 and s.dim() == 0 and s.is_cuda
    s.backward()
    check_case(case, d, float(s.detach()), p.grad.cpu(), t.grad.cpu(), noise_max_of(cases, case) if case.startswith("equal") else None)


EDGE_SHAPES = [
    ("one tile", (1, 1, TH, TW)),
    ("tile + 1", (1, 1, TH + 1, TW + 1)),
    ("three ragged tiles each way", (1, 3, 2 * TH + 6, 2 * TW + 11)),
    ("three ragged tiles, W a multiple of 4", (1, 3, 2 * TH + 6, 2 * TW + 12)),      # staged with 16-byte loads
    ("H = 1", (1, 2, 1, TW + 8)),
    ("W = 1", (1, 2, TH + 16, 1)),
    ("window larger than the image", (1, 1, 6, 6)),
    ("seven planes", (7, 1, 9, 10)),
]


@pytest.mark.parametrize("what,shape", EDGE_SHAPES, ids=[w for w, _ in EDGE_SHAPES])
def test_tile_edge_shapes_against_float64(what, shape):
    """Both inputs require a gradient at once, and the upstream gradient is not 1: loss = 0.25 (1 - SSIM)."""
    pred, gt = noise_pair(shape, 100 + len(what))
    want, ga64, gb64 = ssim_f64(pred, gt)
    p, t = pred.clone().requires_grad_(True), gt.clone().requires_grad_(True)
    s = wm.ops.ssim_mean(p, t)
    (0.25 * (1 - s)).backward()
    print(f"{what}: value err {abs(float(s) - want):.2e}")
    assert abs(float(s) - want) <= 1e-5
    for name, g, truth in (("pred", p.grad, -0.25 * ga64), ("gt", t.grad, -0.25 * gb64)):
        l2, mx = rel_err(g, truth)
        print(f"{what}: d/d{name} l2 {l2:.2e} max {mx:.2e}")
        assert l2 <= truth_bar(0.0) and mx <= truth_bar(0.0), f"{what}: d/d{name} l2 {l2:.3e} max {mx:.3e}"


def kind_pair(kind, shape, seed):
    """The fixture's smooth / dark / unclamped inputs (tests/golden/make_golden_ssim_loss.py describes them), made here."""
    g = torch.Generator().manual_seed(seed)
    u, n = torch.rand(shape, generator=g), torch.randn(shape, generator=g)
    if kind == "smooth":                                          # 7 x 7 box blur of uniform noise
        gt = F.avg_pool2d(F.pad(u, (3, 3, 3, 3), mode="replicate"), 7, stride=1)
        pred = (gt + 0.1 * n).clamp(0, 1)
    elif kind == "dark":
        gt = 0.05 * u
        pred = (gt + 0.005 * n).clamp(0, 1)
    else:                                                         # unclamped: values outside [0, 1]
        gt, pred = u, u + 0.5 * n
        assert float(pred.min()) < 0.0 and float(pred.max()) > 1.0
    return pred.contiguous().to(DEV), gt.contiguous().to(DEV)


@pytest.mark.parametrize("kind", ["smooth", "dark", "unclamped"])
def test_other_input_kinds_on_a_multi_tile_shape_against_float64(kind):
    """The fixture holds these kinds at the three small shapes only (one (2, 3, 40, 130) case is 1 MB); here they run over
    2 x 5 tiles with ragged ends against the float64 evaluation.  No float32 reference is at hand: truth_bar(0) = 1e-4."""
    pred, gt = kind_pair(kind, (2, 3, 40, 130), 500 + len(kind))
    want, ga64, gb64 = ssim_f64(pred, gt)
    p, t = pred.clone().requires_grad_(True), gt.clone().requires_grad_(True)
    s = wm.ops.ssim_mean(p, t)
    s.backward()
    print(f"{kind}: value err {abs(float(s) - want):.2e}")
    assert abs(float(s) - want) <= 1e-5
    for name, g, truth in (("pred", p.grad, ga64), ("gt", t.grad, gb64)):
        l2, mx = rel_err(g, truth)
        print(f"{kind}: d/d{name} l2 {l2:.2e} max {mx:.2e}")
        assert l2 <= truth_bar(0.0) and mx <= truth_bar(0.0), f"{kind}: d/d{name} l2 {l2:.3e} max {mx:.3e}"


def test_planes_off_a_16_byte_boundary_give_the_same_bits():
    """W % 4 == 0 and 16-byte-aligned planes are staged with 16-byte loads, anything else element by element: the same inputs
    one float off the boundary (a contiguous view at storage offset 1) give bit-equal value and gradients."""
    shape = (2, 3, TH + 7, 2 * TW + 4)
    pred, gt = noise_pair(shape, 61)
    n = pred.numel()

    def shifted(t):
        buf = torch.empty(n + 1, device=DEV)
        v = buf[1:].view(shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v
    runs = []
    for p, t in ((pred.clone(), gt.clone()), (shifted(pred), shifted(gt))):
        p.requires_grad_(True)
        t.requires_grad_(True)
        s = wm.ops.ssim_mean(p, t)
        s.backward()
        runs.append((s.detach(), p.grad, t.grad))
    assert pred.data_ptr() % 16 == 0
    assert all(torch.equal(x, y) for x, y in zip(*runs))
    want, ga64, gb64 = ssim_f64(pred, gt)
    assert abs(float(runs[0][0]) - want) <= 1e-5
    for g, truth in ((runs[0][1], ga64), (runs[0][2], gb64)):
        l2, mx = rel_err(g, truth)
        assert l2 <= truth_bar(0.0) and mx <= truth_bar(0.0), (l2, mx)


def _kernels_of(fn):
    """The names of the device kernels `fn` launches (torch.profiler), after one unrecorded call."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]


def test_launch_counts_two_forward_and_one_per_gradient():
    """ops.ssim_mean (what trainer.ssim_loss calls): the tile kernel and the fixed-order sum forward, one filter kernel per
    requested gradient backward - and no other kernel, no memset and no copy in the forward + backward of the SSIM itself."""
    pred, gt = noise_pair((2, 3, TH + 5, 2 * TW + 3), 51)
    upstream = torch.full((), -0.25, device=DEV)                  # made beforehand: autograd's own ones_like is a fill kernel

    def run(want_pred, want_gt):
        p, t = pred.clone().requires_grad_(want_pred), gt.clone().requires_grad_(want_gt)

        def go():
            s = wm.ops.ssim_mean(p, t)
            if want_pred or want_gt:
                torch.autograd.grad(s, [x for x in (p, t) if x.requires_grad], upstream)
        return sorted(_kernels_of(go))
    for want_pred, want_gt in ((False, False), (True, False), (False, True), (True, True)):
        names = run(want_pred, want_gt)
        own = [n for n in names if "ssim_loss" in n]
        print(f"pred grad {want_pred}, gt grad {want_gt}: {names}")
        assert sum("ssim_loss_fwd_kernel" in n for n in own) == 1 and sum("ssim_loss_finish_kernel" in n for n in own) == 1
        assert sum("ssim_loss_bwd_kernel" in n for n in own) == int(want_pred) + int(want_gt)
        assert len(own) == 2 + int(want_pred) + int(want_gt)
        assert len(names) == len(own), f"other device work in the SSIM forward + backward: {names}"


def test_non_contiguous_input_and_single_sided_gradients():
    g = torch.Generator().manual_seed(9)
    big = torch.rand(2, 5, TH + 3, TW + 5, generator=g).to(DEV)
    gt = torch.rand(2, 3, TH + 3, TW + 5, generator=g).to(DEV)
    pred = big[:, 1:4]                                           # a channel slice: not contiguous
    assert not pred.is_contiguous()
    want, ga64, gb64 = ssim_f64(pred, gt)
    leaf = big.clone().requires_grad_(True)
    s = wm.ops.ssim_mean(leaf[:, 1:4], gt)                       # only pred wants a gradient
    s.backward()
    assert abs(float(s) - want) <= 1e-5
    l2, mx = rel_err(leaf.grad[:, 1:4], ga64)
    assert l2 <= truth_bar(0.0) and mx <= truth_bar(0.0), (l2, mx)
    assert float(leaf.grad[:, 0].abs().max()) == 0.0 and float(leaf.grad[:, 4].abs().max()) == 0.0
    t = gt.clone().requires_grad_(True)
    s2 = wm.ops.ssim_mean(pred, t)                               # only the target wants one
    s2.backward()
    assert torch.equal(s2.detach(), s.detach())
    l2, mx = rel_err(t.grad, gb64)
    assert l2 <= truth_bar(0.0) and mx <= truth_bar(0.0), (l2, mx)
    with torch.no_grad():                                        # nothing is kept without a gradient
        s3 = wm.ops.ssim_mean(leaf[:, 1:4], t)
    assert not s3.requires_grad and torch.equal(s3, s.detach())
    assert wm.ops._ssim_forward(pred.contiguous(), gt, False, False)[1:] == (None, None, None, None)


def test_repeated_calls_are_bit_identical():
    pred, gt = noise_pair((2, 3, 2 * TH + 5, 3 * TW + 7), 21)
    runs = []
    for _ in range(3):
        p, t = pred.clone().requires_grad_(True), gt.clone().requires_grad_(True)
        s = wm.ops.ssim_mean(p, t)
        s.backward()
        runs.append((s.detach().clone(), p.grad.clone(), t.grad.clone()))
    for r in runs[1:]:
        assert all(torch.equal(x, y) for x, y in zip(r, runs[0]))


def _eager_noise():
    """What a training loop does between two replays: kernels and allocations of its own (NaN / 1e30 fills of several sizes)."""
    for n, v in ((8, float("nan")), (320, 1e30), (1024, float("nan")), (65536, 1e30), (1 << 20, float("nan"))):
        t = torch.full((n,), v, device=DEV)
        del t
    torch.cuda.synchronize()


def test_forward_and_backward_replay_from_a_graph_with_eager_work_between():
    """The memset-node failure mode (profiles/r06/graph_memset_node.md): nothing in the captured forward + backward may be zeroed
    by a memset node or reduced by ATen.  Replay, eager work, replay, then new inputs: value and gradient equal the eager ones."""
    shape = (2, 3, 2 * TH + 5, 2 * TW + 9)
    pairs = [noise_pair(shape, 31), noise_pair(shape, 32)]

    def eager(pred, gt):
        p = pred.clone().requires_grad_(True)
        s = wm.ops.ssim_mean(p, gt)
        g, = torch.autograd.grad(0.25 * (1 - s), p)
        return s.detach().clone(), g.clone()
    want = [eager(*pr) for pr in pairs]
    a, b = pairs[0][0].clone().requires_grad_(True), pairs[0][1].clone()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                               # warm-up off the capture's stream
        torch.autograd.grad(0.25 * (1 - wm.ops.ssim_mean(a, b)), a)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = wm.ops.ssim_mean(a, b)
        ga, = torch.autograd.grad(0.25 * (1 - s), a)
    for k, (pred, gt) in enumerate([pairs[0], pairs[0], pairs[1], pairs[0]]):
        with torch.no_grad():
            a.copy_(pred)
            b.copy_(gt)
        graph.replay()
        torch.cuda.synchronize()
        ws, wg = want[1] if pred is pairs[1][0] else want[0]
        assert torch.equal(s.detach(), ws), f"replay {k}: SSIM {float(s)} eager {float(ws)}"
        assert torch.equal(ga, wg), f"replay {k}: gradient differs by {float((ga - wg).abs().max()):.3e}"
        _eager_noise()


def test_graphed_train_step_with_the_ssim_term():
    """GraphedTrainStep(..., ssim_weight=0.25) on the wf8 net at 64 x 64 against eager train_step from the same state (the bars of
    test_gpu_parity.py's graphed-step test), and l_ssim = 0.25 (1 - SSIM) of the network's output evaluated in float64."""
    cfg = dict(in_chn=3, wf=8, n_l_blocks=[1, 1, 1], n_h_blocks=[1, 1, 1], ffn_scale=2.0)
    gg = torch.Generator().manual_seed(77)
    batches = [(torch.rand(2, 3, 64, 64, generator=gg).to(DEV), torch.rand(2, 3, 64, 64, generator=gg).to(DEV)) for _ in range(2)]

    def fresh():
        torch.manual_seed(0)
        net = wm.WaveMamba(**cfg).train().to(DEV)
        return net, trainer.make_optimizer(net, capturable=True)
    net_e, opt_e = fresh()
    for _ in range(3):                                           # the graphed step's warm-up, eagerly
        trainer.train_step(net_e, opt_e, *batches[0], as_float=False, ssim_weight=0.25)
    want, truth = [], []
    for lq, gt in batches:
        out = net_e(lq).detach()                                 # with grad enabled: the training forward, as train_step runs it
        truth.append(0.25 * (1.0 - ssim_f64(out, gt)[0]))
        want.append(trainer.loss_values(trainer.train_step(net_e, opt_e, lq, gt, as_float=False, ssim_weight=0.25)))
    net_g, opt_g = fresh()
    step = trainer.GraphedTrainStep(net_g, opt_g, *batches[0], ssim_weight=0.25)
    got = [trainer.loss_values(step(lq, gt)) for lq, gt in batches]
    for a, b, t in zip(got, want, truth):
        assert set(a) == {"l_pix", "l_freq", "l_ssim"}
        for k in a:
            assert abs(a[k] - b[k]) <= 1e-5 * abs(b[k]), f"{k}: graphed {a[k]} eager {b[k]}"
        assert abs(b["l_ssim"] - t) <= 0.25 * 1e-5, f"eager l_ssim {b['l_ssim']} float64 {t}"
        # the truth is of the EAGER net's output; the graphed net's weights differ from it by rounding (held to 1e-5 of each loss
        # two lines up), so the graphed term gets the value bar plus that allowance
        assert abs(a["l_ssim"] - t) <= 0.25 * 1e-5 + 1e-5 * abs(t), f"graphed l_ssim {a['l_ssim']} float64 {t}"
    worst = max(float((p.detach() - q.detach()).abs().max() / (q.detach().abs().max() + 1e-12))
                for p, q in zip(net_g.parameters(), net_e.parameters()))
    assert worst <= 1e-3, f"parameters after 3 + 2 steps differ by {worst:.2e}"


def test_library_op_equals_ops_ssim_mean_and_passes_opcheck():
    import wave_mamba_amd.torch_ops  # noqa: F401  (registers the ops)
    ns = torch.ops.wavemamba_hip
    pred, gt = noise_pair((2, 3, TH + 7, TW + 3), 41)
    a1, b1 = pred.clone().requires_grad_(True), gt.clone().requires_grad_(True)
    a2, b2 = pred.clone().requires_grad_(True), gt.clone().requires_grad_(True)
    s1, s2 = ns.ssim_mean(a1, b1), wm.ops.ssim_mean(a2, b2)
    assert torch.equal(s1, s2)
    (0.25 * (1 - s1)).backward()
    (0.25 * (1 - s2)).backward()
    assert torch.equal(a1.grad, a2.grad) and torch.equal(b1.grad, b2.grad)
    a3 = pred.clone().requires_grad_(True)
    ns.ssim_mean(a3, gt).backward()                              # one-sided: the other gradient is not computed
    assert rel_err(a3.grad, -4.0 * a2.grad)[1] <= 1e-6
    utils = ("test_faketensor", "test_autograd_registration")
    small = [t.clone().requires_grad_(True) for t in noise_pair((1, 2, 7, 9), 42)]
    torch.library.opcheck(ns.ssim_mean.default, tuple(small), test_utils=utils)
    torch.library.opcheck(ns.ssim_mean_backward.default, (small[0].detach(), small[1].detach(), torch.ones((), device=DEV), True, True),
                          test_utils=("test_faketensor",))


def test_error_paths():
    a = torch.rand(1, 3, 8, 8, device=DEV)
    with pytest.raises(RuntimeError):
        wm.ops.ssim_mean(a.cpu(), a.cpu())                       # _require_cuda
    with pytest.raises(RuntimeError):
        wm.ops.ssim_mean(a, a.cpu())
    with pytest.raises(RuntimeError):
        wm.ops.ssim_mean(a, torch.rand(1, 3, 8, 9, device=DEV))  # shape mismatch
    with pytest.raises(RuntimeError):
        wm.ops.ssim_mean(a[0], a[0])                             # not 4-D
    with pytest.raises(RuntimeError):
        wm.ops.ssim_mean(a[:0], a[:0])                           # empty
    assert float(trainer.ssim_loss(a, a)) == 0.0                 # fp32 CUDA tensors: the kernels (identical images: exactly 1)
