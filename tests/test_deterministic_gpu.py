"""GPU: the deterministic training mode (ops.set_deterministic / WM_DETERMINISTIC=1).

With the mode on, the nine accumulate-into entry points run their wm_*_det forms (per-workgroup partials, fixed-order finish) and
the two channel gathers of the HFE branch take the ordered wm_channel_gather_bwd: every gradient and the loss value are bit-equal
run to run, per operator, over whole training steps and under graph capture.  Accuracy is held to the bars of the existing test of
each entry point (cited case by case), against float64 evaluated on the host.

Shapes.  Two atomic addends commute, so every shape is taken from that kernel's grid rule (csrc/*.hip) such that at least FOUR
partials meet on every output element, with one ragged dimension:
  dwconv3x3_wgrad   partials per value = B x ceil(W / (4 lanes-per-row)) x ceil(H / 64): B = 3, H = 72 / 70 -> 6
  layernorm2d_bwd   workgroups = min(512, ceil(B H W tpp / 256)): 3 x 40 x 36 -> 34 (C = 32, 64: the pair kernel), 18 (C = 16)
  layernorm_tok_bwd workgroups = min(1024, ceil(T / (1024 / C))): T = 4440 -> 139 (C = 32), T = 4320 -> 270 (C = 64)
  linear_wgrad      workgroups = ceil(ceil(T / 512) / 8): T = 20011 -> 5, and eight waves per workgroup through LDS
  plane_sums        B x min(cap, ceil(H W / 8192)): B = 5 -> 5; B = 3, 97 x 101 -> 6
  scale_add_bwd     B x min(8.., ceil(H W / 1024)): 3 x 2 -> 6
  l1_mean_fwd       ceil(n / 8192) (16-byte form) or ceil(n / 2048): 8 x 3 x 256 x 256 -> 192 (with 5 workgroups the atomic form never
                    differed in 20 repeats - profiles/deterministic/README.md - so the shape was enlarged), 36783 -> 18
  selscan_bwd       dA / dD / dbias: blocks per channel of the finish kernel = ceil(20 nblocks / 960): L >= 2400 -> 4;
                    dB / dC: wpg = ceil((dim / G) / 64): dim = 200, G = 1 -> 4 (the last slice holds 8 channels); wpg = 1 beside it
  channel_gather    an index with up to five sources on one destination and destinations that receive nothing"""
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close, rel_err
from oracle import oracle
import wave_mamba_amd as wm
from wave_mamba_amd.archs import wavemamba_arch as arch
from test_gpu_parity import GRAD_NAMES, TOL, gen, random_scan_case, scan_grads_f64, truth_bar

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPEATS = 20
SHIPPED = dict(in_chn=3, wf=32, n_l_blocks=[1, 2, 4], n_h_blocks=[1, 1, 2], ffn_scale=2.0)
SMALL = dict(in_chn=3, wf=8, n_l_blocks=[1, 1, 1], n_h_blocks=[1, 1, 1], ffn_scale=2.0)       # tests/test_rccl_gpu.py: CFG


@pytest.fixture
def deterministic():
    prev = wm.set_deterministic(True)
    yield
    wm.set_deterministic(prev)


class Case:
    """One operator call on fixed inputs: run() -> the outputs under test (device tensors); check(outputs) holds them to float64."""

    def __init__(self, run, check):
        self.run, self.check = run, check


def _leaves(*ts):
    return [t.to(DEV).requires_grad_(True) for t in ts]


def _off16(t):
    """t on the device as a contiguous view ONE float into a larger buffer: a data pointer that is 4-byte but not 16-byte aligned
    (the kernels drop their 16-byte accesses there)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _dwconv(shape, bias=True, misaligned=False):
    """bias=False: a depth-wise conv without bias (db NULL in the library call) -> (dW,) alone; misaligned: x and gy as _off16 views."""
    B, C, H, W = shape
    gg = gen(H * W)
    x, w, b, gy = (torch.randn(*shape, generator=gg), torch.randn(C, 1, 3, 3, generator=gg) * 0.3, torch.randn(C, generator=gg),
                   torch.randn(*shape, generator=gg))
    xg, wg, bg = _leaves(x, w, b)
    gyd = gy.to(DEV)
    if misaligned:
        xg, gyd = _off16(x).requires_grad_(True), _off16(gy)
    names = ("dW", "db") if bias else ("dW",)

    def run():
        if bias:
            return torch.autograd.grad(wm.ops.dwconv3x3_train(xg, wg, bg), (wg, bg), gyd)
        return torch.autograd.grad(wm.ops.dwconv3x3_train(xg, wg, None), (wg,), gyd)

    def check(got):
        xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
        want = torch.autograd.grad(F.conv2d(xr, wr, br, padding=1, groups=C), (wr, br), gy.double())
        assert len(got) == len(names)
        for name, a, r in zip(names, got, want):
            assert_close(a, r.float(), 2e-5, f"dwconv {name} {shape}")      # the bar of test_dwconv3x3_gradients_vs_torch_autograd
    return Case(run, check)


def _layernorm2d(shape, misaligned=False):
    B, C, H, W = shape
    x, w, b, gy = (torch.randn(*shape, generator=gen(1)) * 2 + 0.5, torch.randn(C, generator=gen(2)), torch.randn(C, generator=gen(3)),
                   torch.randn(*shape, generator=gen(4)))
    xg, wg, bg = _leaves(x, w, b)
    gyd = gy.to(DEV)
    if misaligned:
        xg, gyd = _off16(x).requires_grad_(True), _off16(gy)

    def check(got):
        xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
        mu = xr.mean(1, keepdim=True)
        var = (xr - mu).pow(2).mean(1, keepdim=True)
        y = wr.view(1, -1, 1, 1) * ((xr - mu) / (var + 1e-6).sqrt()) + br.view(1, -1, 1, 1)
        want = torch.autograd.grad(y, (xr, wr, br), gy.double())
        for name, a, r in zip(("gx", "dw", "db"), got, want):
            assert_close(a, r.float(), 5e-5, f"LayerNorm2d {name} {shape}")  # the bar of test_layernorm2d_gradients_vs_torch_autograd
    return Case(lambda: torch.autograd.grad(wm.ops.layernorm2d_train(xg, wg, bg, 1e-6), (xg, wg, bg), gyd), check)


def _layernorm_tok(shape):
    C = shape[-1]
    gg = gen(C + len(shape))
    x, w, b, gy = (torch.randn(*shape, generator=gg) * 2.0 + 0.5, torch.randn(C, generator=gg) * 0.5 + 1.0, torch.randn(C, generator=gg),
                   torch.randn(*shape, generator=gg))
    xg, wg, bg = _leaves(x, w, b)
    gyd = gy.to(DEV)

    def check(got):
        xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
        want = torch.autograd.grad(F.layer_norm(xr, (C,), wr, br, 1e-5), (xr, wr, br), gy.double())
        for name, a, r in zip(("gx", "dweight", "dbias"), got, want):
            assert_close(a, r.float(), 2e-5, f"layernorm_tok {name} {shape}")  # the bar of test_layernorm_tok_forward_backward_vs_torch
    return Case(lambda: torch.autograd.grad(wm.ops.layernorm_tok(xg, wg, bg, 1e-5), (xg, wg, bg), gyd), check)


def _linear(T, O, I):
    gg = gen(T % 97 + O)
    x, w, gy = torch.randn(T, I, generator=gg), torch.randn(O, I, generator=gg) / I ** 0.5, torch.randn(T, O, generator=gg)
    xg, wg = _leaves(x, w)
    gyd = gy.to(DEV)

    def check(got):
        assert_close(got[0], (gy.double().t() @ x.double()).float(), 2e-5, f"linear gw {(T, O, I)}")   # the bar of test_linear_wgrad_vs_torch
    return Case(lambda: torch.autograd.grad(wm.ops.linear_nobias(xg, wg), (wg,), gyd), check)


def _plane_sums(shape):
    x = torch.randn(*shape, generator=gen(2))
    xd = x.to(DEV)

    def check(got):
        # the bar of test_zeros_small_hands_out_zeroed_distinct_slices (and of the bias gradient in test_conv2d_wgrad_vs_float64)
        assert_close(got[0], x.double().sum((0, 2, 3)).float(), 1e-5, f"plane_sums {shape}")
    return Case(lambda: (wm.ops.plane_sums(xd),), check)


def _scale_add(shape):
    B, C, H, W = shape
    gg = gen(B * 100 + W)
    x, o, g = (torch.randn(B, C, H, W, generator=gg) for _ in range(3))
    s = torch.randn(C, generator=gg) * 0.3 + 1
    xg, sg, og = _leaves(x, s, o)
    gd = g.to(DEV)

    def check(got):
        want = (g.double() * x.double()).sum((0, 2, 3))
        assert_close(got[0], want.float(), 2e-5, f"scale_add d/dscale {shape}")      # the bar of test_scale_add_vs_fp64_autograd
    return Case(lambda: torch.autograd.grad(wm.ops.scale_add(xg, sg, og), (sg,), gd), check)


def _l1_mean(shape):
    gg = gen(3)
    a, b = torch.rand(*shape, generator=gg), torch.rand(*shape, generator=gg)
    ad, bd = a.to(DEV), b.to(DEV)

    def check(got):
        want = float((a.double() - b.double()).abs().mean())
        print(f"l1_mean {tuple(shape)}: {abs(float(got[0]) - want) / want:.2e} of the float64 mean")
        assert got[0].shape == () and abs(float(got[0]) - want) <= 2e-6 * want, (float(got[0]), want)   # the bar of test_l1_mean_vs_float64
    return Case(lambda: (wm.ops.l1_mean(ad, bd),), check)


def _selscan(batch, dim, L, N, G, plain=False):
    """plain: the scan without D and delta_bias and with delta_softplus=False (dD and dbias NULL in the library call; delta is made
    positive, as a step that is not passed through softplus has to be) -> the five remaining gradients."""
    case = random_scan_case(batch, dim, L, N, G, seed=7 + L)
    softplus = not plain
    if plain:
        case = (case[0], case[1].abs() * 0.2 + 0.01) + case[2:5] + (None, None)
    dy = torch.randn(batch, dim, L, generator=gen(L))
    leaves = [None if t is None else t.to(DEV).requires_grad_(True) for t in case]
    dyd = dy.to(DEV)

    def run():
        y = wm.ops.selective_scan_fn(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], leaves[5], None, leaves[6], softplus)
        return torch.autograd.grad(y, [t for t in leaves if t is not None], dyd)

    def check(got):
        # the bars of test_scan_backward_vs_oracle: reduced gradients against float64 at truth_bar(the oracle's own fp32 error)
        # (all-zero ones - dA at L = 1 - by its absolute check), the others at TOL
        want = oracle.selscan_bwd_raw(*case, dy, softplus)
        truth = scan_grads_f64(*case, dy, delta_softplus=softplus)
        names = [n for n, t in zip(GRAD_NAMES, case) if t is not None]
        assert len(got) == len(names)
        for name, g in zip(names, got):
            ref = want[GRAD_NAMES.index(name)]
            if name in ("dA", "dD", "dbias") and float(truth[name].abs().max()) == 0.0:
                assert float(g.abs().max()) <= 1e-6, f"{name}: expected zeros, max abs {float(g.abs().max()):.3e}"
            elif name in ("dA", "dD", "dbias"):
                e_ref = max(rel_err(ref.double(), truth[name]))
                e_got = max(rel_err(g.cpu().double(), truth[name]))
                assert e_got <= truth_bar(e_ref), f"{name} {(batch, dim, L, N, G)}: {e_got:.3e} vs float64 (oracle fp32: {e_ref:.3e})"
            else:
                assert_close(g, truth[name].float(), TOL, f"{name} {(batch, dim, L, N, G)}")
    return Case(run, check)


def _gather_index(B, C, M, seed):
    """(B, M) int32 indices into C channels: channel 1 is named five times and channel 2 three times in every batch element, the
    upper half of the channels never - repeated destinations and destinations that receive nothing."""
    idx = torch.randint(0, max(1, C // 2), (B, M), generator=gen(seed), dtype=torch.int32)
    idx[:, :5] = 1
    idx[:, M - 3:] = 2
    return idx


def _gather(form, B, C, M, plane, idx=None, misaligned=False):
    """form "cat": _cat_gathered on (B, C, H, W) maps (PAConv's second input); "maps": channel_gather on (B, C, HW) token maps (what
    nearest_candidate_maps calls with the matched indices).  idx: a given (B, M) int32 index instead of _gather_index's;
    misaligned: the map and the incoming gradient as _off16 views."""
    gg = gen(B + C + M)
    x2 = torch.randn(B, C, *plane, generator=gg)
    x = torch.randn(B, 8, *plane, generator=gg)
    if idx is None:
        idx = _gather_index(B, C, M, seed=M)
        assert int(idx.max()) < max(3, C // 2)                                # the upper half of the channels receives nothing
    gy = torch.randn(B, (8 if form == "cat" else 0) + M, *plane, generator=gg)
    x2g, = _leaves(x2)
    xd, idxd, gyd = x.to(DEV), idx.to(DEV), gy.to(DEV)
    if misaligned:
        x2g, gyd = _off16(x2).requires_grad_(True), _off16(gy)
    full = idx.long().reshape(idx.shape + (1,) * len(plane)).expand(-1, -1, *plane)
    unnamed = torch.ones(B, C, dtype=torch.bool).scatter_(1, idx.long(), False)      # (b, c) that no index names

    fulld = full.to(DEV)

    def run():
        if form == "cat":
            y = arch._cat_gathered(xd, x2g, idxd)
        else:                    # nearest_candidate_maps' switch, with a given index (the function computes its own)
            y = wm.ops.channel_gather(x2g, idxd) if wm.is_deterministic() else torch.gather(x2g, 1, fulld)
        return (y.detach(),) + torch.autograd.grad(y, (x2g,), gyd)

    def check(got):
        y, gx = got
        want_y = torch.gather(x2, 1, full)
        assert torch.equal(y.cpu(), torch.cat([x, want_y], 1) if form == "cat" else want_y)
        g2 = gy[:, 8:] if form == "cat" else gy
        truth = torch.zeros(B, C, *plane, dtype=torch.float64).scatter_add_(1, full, g2.double())
        ref32 = torch.zeros(B, C, *plane).scatter_add_(1, full, g2)
        e_ref, e_got = max(rel_err(ref32, truth)), max(rel_err(gx.cpu(), truth))
        assert e_got <= truth_bar(e_ref), f"gather backward {form}: {e_got:.3e} vs float64 (fp32 scatter-add: {e_ref:.3e})"
        assert int((gx.cpu()[unnamed] != 0).sum()) == 0, "a destination that no index names must be zero"
    return Case(run, check)


CASES = {
    "dwconv3x3_wgrad-16B": lambda: _dwconv((3, 32, 72, 36)),
    "dwconv3x3_wgrad-elementwise": lambda: _dwconv((3, 7, 70, 37)),
    "layernorm2d_bwd-pair32": lambda: _layernorm2d((3, 32, 40, 36)),
    "layernorm2d_bwd-pair64": lambda: _layernorm2d((3, 64, 40, 37)),
    "layernorm2d_bwd-c16": lambda: _layernorm2d((3, 16, 40, 37)),
    "layernorm_tok_bwd-c32": lambda: _layernorm_tok((3, 40, 37, 32)),
    "layernorm_tok_bwd-c64": lambda: _layernorm_tok((3, 40, 36, 64)),
    "linear_wgrad-128x32": lambda: _linear(20011, 128, 32),
    "linear_wgrad-32x64": lambda: _linear(20011, 32, 64),
    "plane_sums-16B": lambda: _plane_sums((5, 32, 40, 36)),
    "plane_sums-elementwise": lambda: _plane_sums((3, 64, 97, 101)),
    "scale_add_bwd-16B": lambda: _scale_add((3, 32, 40, 36)),
    "scale_add_bwd-elementwise": lambda: _scale_add((3, 64, 40, 37)),
    "l1_mean_fwd-16B": lambda: _l1_mean((8, 3, 256, 256)),
    "l1_mean_fwd-elementwise": lambda: _l1_mean((3, 3, 61, 67)),
    "selscan_bwd-wpg4": lambda: _selscan(1, 200, 2405, 16, 1),
    "selscan_bwd-wpg1": lambda: _selscan(1, 64, 2400, 16, 2),
    "channel_gather_bwd-cat": lambda: _gather("cat", 3, 32, 32, (40, 36)),
    "channel_gather_bwd-maps": lambda: _gather("maps", 3, 64, 48, (1481,)),
}
NINE = [k for k in CASES if not k.startswith("channel_gather")]


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def differing_repeats(c, repeats=REPEATS):
    """Run the case once for the reference, then `repeats` more times - the second half while a second stream runs an unrelated
    matrix-core convolution (as test_ss2d_core_backward_bit_reproducible_stress does).  -> (number of repeats in which any output
    element differed from the reference, the reference outputs)."""
    ref = [t.clone() for t in c.run()]
    torch.cuda.synchronize()
    xa = torch.randn(1, 64, 128, 128, generator=gen(12)).to(DEV)
    w3 = (torch.randn(64, 64, 3, 3, generator=gen(13)) / 24).to(DEV)
    side = torch.cuda.Stream(DEV)
    bad = torch.zeros(repeats, dtype=torch.int64, device=DEV)
    keep = []
    for r in range(repeats):
        if r >= repeats // 2:
            with torch.cuda.stream(side), torch.no_grad():
                keep.append(wm.ops.conv2d(xa, w3))
                if len(keep) > 6:
                    keep.pop(0)
        for a, b in zip(c.run(), ref):
            bad[r] += (a != b).sum()
    torch.cuda.synchronize()
    return int((bad > 0).sum()), ref


@pytest.mark.parametrize("name", list(CASES))
def test_entry_point_is_bit_reproducible_and_right(name, deterministic):
    """Mode on: 20 repeated calls on the same inputs give torch.equal outputs, half of them with another stream busy; the same
    outputs meet the existing float64 bar of that entry point."""
    c = case(name)
    differed, ref = differing_repeats(c)
    assert differed == 0, f"{name}: {differed} of {REPEATS} repeats differ from the first call"
    assert all(bool(torch.isfinite(t).all()) for t in ref)
    c.check(ref)


@pytest.mark.parametrize("name", NINE)
def test_mode_off_launches_no_deterministic_kernel(name):
    """Mode off: the call takes today's launch path - the finish kernel of the wm_*_det forms (profiling class "det_finish",
    recorded by every one of them) never runs; with the mode on the same call records it."""
    c = case(name)
    counts = {}
    for on in (False, True):
        prev = wm.set_deterministic(on)
        wm.ops.prof_enable(["det_finish"])
        try:
            c.run()
            torch.cuda.synchronize()
            counts[on] = wm.ops.prof_collect()["det_finish"][0]
        finally:
            wm.ops.prof_enable(False)
            wm.set_deterministic(prev)
    assert counts[False] == 0 and counts[True] >= 1, counts


def _three_steps(cfg, state, lq, gt):
    """Three train_steps of a fresh network and optimizer from `state` -> (gradients after the first step, weights and the three
    loss values after the third)."""
    net = wm.WaveMamba(**cfg).train().to(DEV)
    net.load_state_dict(state)
    opt = wm.trainer.make_optimizer(net)
    wm.trainer.train_step(net, opt, lq, gt, as_float=False, ssim_weight=0.25)
    grads = [p.grad.detach().clone() for p in net.parameters()]
    for _ in range(2):
        losses = wm.trainer.train_step(net, opt, lq, gt, as_float=False, ssim_weight=0.25)
    return grads, [p.detach().clone() for p in net.parameters()], {k: v.clone() for k, v in losses.items()}


@pytest.mark.parametrize("cfg", [SHIPPED, SMALL], ids=["shipped", "wf8"])
def test_three_training_steps_twice_are_bit_equal(cfg, deterministic):
    """From one saved state, three train_steps run twice (fresh network and optimizer each time, 3 x 3 x 64 x 64, ssim_weight 0.25):
    every parameter gradient after the first step, every weight and all three loss values after the third are torch.equal."""
    torch.manual_seed(0)
    state = {k: v.clone() for k, v in wm.WaveMamba(**cfg).state_dict().items()}
    gg = gen(21)
    lq, gt = torch.rand(3, 3, 64, 64, generator=gg).to(DEV), torch.rand(3, 3, 64, 64, generator=gg).to(DEV)
    g1, w1, l1 = _three_steps(cfg, state, lq, gt)
    g2, w2, l2 = _three_steps(cfg, state, lq, gt)
    names = [n for n, _ in wm.WaveMamba(**cfg).named_parameters()]
    assert len(l1) == 3 and all(bool(torch.isfinite(v)) for v in l1.values())
    bad_g = [n for n, a, b in zip(names, g1, g2) if not torch.equal(a, b)]
    assert not bad_g, f"{len(bad_g)} of {len(names)} gradients differ after the first step, first: {bad_g[:5]}"
    bad_w = [n for n, a, b in zip(names, w1, w2) if not torch.equal(a, b)]
    assert not bad_w, f"{len(bad_w)} of {len(names)} weights differ after the third step, first: {bad_w[:5]}"
    assert all(torch.equal(l1[k], l2[k]) for k in l1), (l1, l2)


def test_two_graphed_train_steps_replay_to_bit_equal_weights(deterministic):
    """Two GraphedTrainStep objects built from identical state (wf = 8), three replays each with an eager launch between replays:
    bit-equal weights - the workspaces of the deterministic forms under capture, and no accumulator left over between replays."""
    gg = gen(22)
    lq, gt = torch.rand(3, 3, 64, 64, generator=gg).to(DEV), torch.rand(3, 3, 64, 64, generator=gg).to(DEV)

    def run():
        torch.manual_seed(0)
        net = wm.WaveMamba(**SMALL).train().to(DEV)
        step = wm.trainer.GraphedTrainStep(net, wm.trainer.make_optimizer(net, capturable=True), lq, gt, ssim_weight=0.25)
        for _ in range(3):
            losses = step(lq, gt)
            assert bool(torch.isfinite(losses["l_pix"]))                      # an eager launch (and a host read) between replays
        torch.cuda.synchronize()
        return [p.detach().clone() for p in net.parameters()]
    a, b = run(), run()
    bad = sum(not torch.equal(p, q) for p, q in zip(a, b))
    assert bad == 0, f"{bad} of {len(a)} weight tensors differ between two graphed runs"
