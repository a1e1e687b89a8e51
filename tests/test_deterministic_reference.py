"""GPU: the deterministic training mode (ops.set_deterministic / WM_DETERMINISTIC=1) held to float64 where test_deterministic_gpu.py
only holds it to itself.  That file picks, per operator, one family of shapes at which many partials meet on every output (right for
races) and asserts bit-equality; a gradient that is wrong the same way every time passes it.  Here:

  A  the zero-padded convolution weight gradient (ops._conv_weight_grad with the mode on: maps whose width is no multiple of 32 are
     right-padded and go to wm_conv2d_wgrad) against the float64 gradient of F.conv2d, and the output-channel counts that stay on ATen;
  B  whole training steps with the mode on against the reference goldens that test_gpu_parity.py checks with the mode off;
  C  the wm_*_det forms and the channel gathers at the edges of the finish kernel's bookkeeping: one partial only, NULL optional
     outputs, records whose used length differs from their padded length, planes that are 4-byte but not 16-byte aligned, empty
     problems, the gather's M = 1024 limit;
  D  the status codes of those entry points from real ctypes calls (refusals that return before any launch).

No bar is new: each is the one an existing test applies to the same kernel, cited where it is used (most inside the Case builders
of test_deterministic_gpu.py, which this module reuses)."""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close, rel_err
import wave_mamba_amd as wm
from wave_mamba_amd import _lib, ops
from test_deterministic_gpu import _dwconv, _gather, _l1_mean, _layernorm2d, _layernorm_tok, _linear, _plane_sums, _scale_add, _selscan
from test_gpu_parity import (check_shipped256_step, check_shipped64_fingerprints, check_wf8_step_gradients, gen, truth_bar)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture
def deterministic():
    prev = wm.set_deterministic(True)
    yield
    wm.set_deterministic(prev)


class _Seen(list):
    """The launched entry points' names, in order; .args[i]: the arguments of launch i as ops._launch received them."""

    def __init__(self):
        super().__init__()
        self.args = []


@contextlib.contextmanager
def launch_spy():
    """The names of the library entry points launched inside the block (every launch goes through ops._launch); autograd stays on,
    unlike under test_hfe_heads.launches."""
    names = _Seen()
    real = ops._launch

    def spy(dev, name, *a, **k):
        names.append(name)
        names.args.append(a)
        return real(dev, name, *a, **k)
    ops._launch = spy
    try:
        yield names
    finally:
        ops._launch = real


# ------------------------------------------------------------------------------------------------
# A. the padded weight-gradient path
# ------------------------------------------------------------------------------------------------
WGRAD_CASES = [
    (3, 2, 64, 64, 8, 16),       # the shipped network's level-2 map of a 64-crop
    (3, 1, 32, 96, 5, 24),       # 96 output channels: two passes over one workspace
    (3, 2, 3, 32, 6, 33),        # pads to 64; ragged input tile
    (3, 1, 32, 3, 4, 31),        # ragged output tile; pad of a single column
    (3, 1, 16, 16, 1, 1),        # a single pixel: only the centre tap is non-zero
    (1, 2, 32, 64, 4, 8),        # 1x1 (in_proj as a convolution)
    (1, 1, 192, 32, 3, 47),      # twelve input tiles
    (1, 3, 12, 32, 5, 40),       # pads to 64, batch 3
    (1, 2, 32, 96, 3, 17),       # six output tiles
]
# output channels whose count, rounded up to 16s, is not 1, 2, 4 or 6 (33-48, 65-80, > 96): the kernel has no form for them, padded
# or not, at either kernel size (ops.conv2d_wgrad_supported)
WGRAD_ON_ATEN = [(3, 1, 32, 72, 4, 16), (1, 1, 32, 72, 4, 16), (3, 1, 16, 40, 4, 16), (1, 2, 16, 112, 3, 8)]


@functools.lru_cache(maxsize=None)
def wgrad_case(ks, B, Cin, Cout, H, W):
    """Host inputs and the float64 gradients of F.conv2d's weight and bias for a random gy (computed once per shape)."""
    gg = gen(ks * 1000 + Cin * 7 + Cout + H + W)
    x = torch.randn(B, Cin, H, W, generator=gg)
    w = torch.randn(Cout, Cin, ks, ks, generator=gg) * 0.1
    b = torch.randn(Cout, generator=gg)
    gy = torch.randn(B, Cout, H, W, generator=gg)
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    dW, db = torch.autograd.grad(F.conv2d(x.double(), wr, br, padding=ks // 2), (wr, br), gy.double())
    return x, w, b, gy, dW, db


def conv_param_grads(case, bias, repeats=1):
    """`repeats` backward calls through ops.conv2d_train -> ([(dW, db or None), ...], the entry points launched by the backwards)."""
    x, w, b, gy = (t.to(DEV) for t in case[:4])
    wg = w.requires_grad_(True)
    bg = b.requires_grad_(True) if bias else None
    out, names = [], []
    for _ in range(repeats):
        y = ops.conv2d_train(x, wg, bg)
        with launch_spy() as seen:
            g = torch.autograd.grad(y, (wg, bg) if bias else (wg,), gy)
        out.append((g[0], g[1] if bias else None))
        names.append(list(seen))
    return out, names


def hold_conv_grads(case, got, what):
    """dW and db against float64 at 1e-5, the bar of test_conv2d_wgrad_vs_float64 (the same kernel, the same products; the padded
    columns add exact zeros).  The one exception: where ATen's own fp32 weight gradient of the same input, measured here, is further
    than 5e-6 from float64, dW is held to truth_bar(that error), as the reduced-gradient tests do."""
    x, w, b, gy, dW, db = case
    ks = w.shape[2]
    aten = torch.ops.aten.convolution_backward(gy.to(DEV), x.to(DEV), w.to(DEV), None, [1, 1], [ks // 2, ks // 2], [1, 1], False,
                                               [0, 0], 1, [False, True, False])[1]
    e_aten, e_got = max(rel_err(aten, dW)), max(rel_err(got[0], dW))
    bar = truth_bar(e_aten) if e_aten > 5e-6 else 1e-5
    print(f"{what}: dW {e_got:.2e} of float64 (ATen fp32 {e_aten:.2e}, bar {bar:g})")
    assert got[0].shape == dW.shape and bool(torch.isfinite(got[0]).all())
    assert e_got <= bar, f"{what}: dW {e_got:.3e} vs float64 > {bar:g} (ATen fp32: {e_aten:.3e})"
    if got[1] is not None:
        print(f"{what}: db {max(rel_err(got[1], db)):.2e} of float64")
        assert_close(got[1], db.float(), 1e-5, f"{what} db")


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("ks,B,Cin,Cout,H,W", WGRAD_CASES)
@pytest.mark.parametrize("mode", ["aten", "f16"])
def test_padded_weight_gradient_vs_float64(mode, ks, B, Cin, Cout, H, W, bias, deterministic):
    """Mode on, a map whose width is no multiple of 32: the weight (and bias) gradient of conv2d_train comes from exactly one
    wm_conv2d_wgrad launch per backward, meets the float64 bar of that kernel, and five backward calls are torch.equal.  Mode off,
    the same call launches no wm_conv2d_wgrad (the width is refused: ATen's weight gradient)."""
    case = wgrad_case(ks, B, Cin, Cout, H, W)
    what = f"padded wgrad {mode} ks={ks} {B}x{Cin}->{Cout} {H}x{W} {'with' if bias else 'no'} bias"
    prev = ops.set_train_conv_mode(mode)
    try:
        got, names = conv_param_grads(case, bias, repeats=5)
        wm.set_deterministic(False)
        _, names_off = conv_param_grads(case, bias)
    finally:
        ops.set_train_conv_mode(prev)
    for seen in names:
        assert seen.count("wm_conv2d_wgrad") == 1, seen
    assert names_off[0].count("wm_conv2d_wgrad") == 0, names_off
    hold_conv_grads(case, got[0], what)
    for r, (dW, db) in enumerate(got[1:]):
        assert torch.equal(dW, got[0][0]), f"{what}: dW of backward {r + 2} differs from the first"
        assert db is None or torch.equal(db, got[0][1]), f"{what}: db of backward {r + 2} differs from the first"


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", WGRAD_ON_ATEN)
@pytest.mark.parametrize("mode", ["aten", "f16"])
def test_weight_gradient_that_stays_on_aten_in_the_mode(mode, shape, bias, deterministic):
    """33-48, 65-80 or more than 96 output channels, 3x3 or 1x1: wm_conv2d_wgrad has no form for them, so with the mode on the call
    still falls through to ATen's weight gradient (not ordered; the shipped configuration has no such convolution) - right against
    float64, and no wm_conv2d_wgrad launch."""
    case = wgrad_case(*shape)
    prev = ops.set_train_conv_mode(mode)
    try:
        got, names = conv_param_grads(case, bias)
    finally:
        ops.set_train_conv_mode(prev)
    assert names[0].count("wm_conv2d_wgrad") == 0, names
    hold_conv_grads(case, got[0], f"wgrad on ATen {mode} {shape}")


# ------------------------------------------------------------------------------------------------
# B. whole training steps with the mode on, against the goldens
# ------------------------------------------------------------------------------------------------
def _took_the_deterministic_forms(names):
    for entry in ("wm_layernorm2d_bwd_det", "wm_dwconv3x3_wgrad_det", "wm_channel_gather_bwd"):
        assert names.count(entry) >= 1, f"the step launched no {entry}: the mode was not on where the operators were called"
    for entry in ("wm_layernorm2d_bwd", "wm_dwconv3x3_wgrad", "wm_plane_sums", "wm_linear_wgrad", "wm_scale_add_bwd", "wm_l1_mean_fwd",
                  "wm_layernorm_tok_bwd", "wm_selscan_bwd"):
        assert names.count(entry) == 0, f"the step launched the atomic {entry} with the mode on"


def test_wf8_step_gradients_with_the_mode_on(deterministic):
    """wf = 8 on 64 x 64 (maps 32 / 16 / 8 wide: the padded weight gradient at two widths): every gradient tensor against
    train_grads_wf8_f64.npz at truth_bar - test_training_step_per_parameter_gradients_on_gpu's assertions, mode on."""
    with launch_spy() as names:
        check_wf8_step_gradients()
    _took_the_deterministic_forms(names)
    assert names.count("wm_conv2d_wgrad") >= 1


def test_shipped64_fingerprints_with_the_mode_on(deterministic):
    """The shipped configuration on 64 x 64: test_training_step_on_gpu_matches_reference's fingerprint assertions, mode on."""
    with launch_spy() as names:
        check_shipped64_fingerprints()
    _took_the_deterministic_forms(names)
    assert names.count("wm_conv2d_wgrad") >= 1


def test_shipped256_step_with_the_mode_on(golden, deterministic):
    """The shipped configuration on 256 x 256 (every width a multiple of 32): the _det forms at their real partial counts -
    test_training_step_shipped_config_256_vs_reference's assertions (sampled tensors plus whole-tensor sums), mode on."""
    check_shipped256_step(golden("train_grads_shipped256"))


# ------------------------------------------------------------------------------------------------
# C. the _det forms and the gathers at their edges
# ------------------------------------------------------------------------------------------------
def _index(rows):
    return torch.tensor(rows, dtype=torch.int32)


# name -> (the entry point the call must launch, the Case builder).  Shapes are those the mode-off tests of each kernel use
# (test_dwconv3x3_gradients_vs_torch_autograd, test_layernorm2d_gradients_vs_torch_autograd, test_layernorm_tok_forward_backward_
# vs_torch, test_linear_wgrad_vs_torch, test_l1_mean_vs_float64, test_scan_backward_vs_oracle), so each builder's bar is known to hold.
EDGES = {
    "dwconv-one-pixel": ("wm_dwconv3x3_wgrad_det", lambda: _dwconv((1, 1, 1, 1))),                 # one partial: S = 2, one lane idle
    "dwconv-ragged": ("wm_dwconv3x3_wgrad_det", lambda: _dwconv((2, 5, 7, 9))),
    "dwconv-three-pixels": ("wm_dwconv3x3_wgrad_det", lambda: _dwconv((1, 3, 1, 1))),
    "dwconv-nobias": ("wm_dwconv3x3_wgrad_det", lambda: _dwconv((2, 5, 7, 9), bias=False)),        # o1 of kDetDw NULL
    "layernorm2d-one-pixel": ("wm_layernorm2d_bwd_det", lambda: _layernorm2d((1, 64, 1, 1))),
    "layernorm2d-3x5": ("wm_layernorm2d_bwd_det", lambda: _layernorm2d((1, 32, 3, 5))),
    "layernorm2d-c8": ("wm_layernorm2d_bwd_det", lambda: _layernorm2d((2, 8, 5, 130))),
    "layernorm_tok-5x8": ("wm_layernorm_tok_bwd_det", lambda: _layernorm_tok((5, 8))),
    "layernorm_tok-c16": ("wm_layernorm_tok_bwd_det", lambda: _layernorm_tok((3, 130, 16))),
    "linear-three-tokens": ("wm_linear_wgrad_det", lambda: _linear(3, 64, 16)),
    "linear-64-tokens": ("wm_linear_wgrad_det", lambda: _linear(64, 16, 16)),
    "linear-two-units": ("wm_linear_wgrad_det", lambda: _linear(513, 32, 32)),                     # two 512-token units, one workgroup
    "plane_sums-one-pixel": ("wm_plane_sums_det", lambda: _plane_sums((1, 1, 1, 1))),
    "plane_sums-row": ("wm_plane_sums_det", lambda: _plane_sums((2, 3, 1, 5))),
    "plane_sums-many-planes": ("wm_plane_sums_det", lambda: _plane_sums((8, 96, 2, 2))),           # one element-wise block per plane
    "scale_add-5x7": ("wm_scale_add_bwd_det", lambda: _scale_add((1, 8, 5, 7))),
    "l1_mean-five": ("wm_l1_mean_fwd_det", lambda: _l1_mean((5,))),
    "l1_mean-5d": ("wm_l1_mean_fwd_det", lambda: _l1_mean((2, 3, 128, 65, 2))),
    "selscan-L1": ("wm_selscan_bwd_det", lambda: _selscan(1, 8, 1, 4, 2)),                         # dA exactly zero
    "selscan-N7": ("wm_selscan_bwd_det", lambda: _selscan(1, 40, 50, 7, 4)),                       # records used 7 + 2 of 16 + pad
    "selscan-N32": ("wm_selscan_bwd_det", lambda: _selscan(1, 64, 45, 32, 2)),
    "selscan-wpg2": ("wm_selscan_bwd_det", lambda: _selscan(2, 96, 77, 16, 1)),
    "selscan-N7-plain": ("wm_selscan_bwd_det", lambda: _selscan(1, 40, 50, 7, 4, plain=True)),     # o1 and o2 of kDetScan NULL
    "gather-single": ("wm_channel_gather_bwd", lambda: _gather("maps", 1, 1, 1, (1,), idx=_index([[0]]))),
    "gather-small": ("wm_channel_gather_bwd", lambda: _gather("maps", 2, 3, 5, (3,), idx=_index([[0, 2, 2, 1, 0], [1, 1, 1, 1, 1]]))),
    "gather-M1024": ("wm_channel_gather_bwd", lambda: _gather("maps", 1, 4, 1024, (4,),            # channel 3 receives nothing
                                                              idx=torch.randint(0, 3, (1, 1024), generator=gen(5), dtype=torch.int32))),
}
# name -> (entry point, builder(misaligned)): W % 4 == 0 / HW % 4 == 0, so only the data pointers (4-byte but not 16-byte aligned)
# take the kernels off their 16-byte accesses; for the depth-wise weight gradient the grid, and with it the number of partials,
# then differs from the vector form's, which the workspace query assumed first.
MISALIGNED = {
    "dwconv": ("wm_dwconv3x3_wgrad_det", lambda mis: _dwconv((1, 8, 6, 8), misaligned=mis)),
    "layernorm2d": ("wm_layernorm2d_bwd_det", lambda mis: _layernorm2d((1, 16, 8, 8), misaligned=mis)),
    "gather": ("wm_channel_gather_bwd", lambda mis: _gather("maps", 2, 6, 7, (8,), misaligned=mis)),
}


def _run_twice_and_check(entry, c, what):
    with launch_spy() as names:
        got = [t.clone() for t in c.run()]
    assert names.count(entry) == 1, f"{what}: expected one {entry}, launched {names}"
    assert all(bool(torch.isfinite(t).all()) for t in got)
    c.check(got)
    again = c.run()
    assert len(again) == len(got) and all(torch.equal(a, b) for a, b in zip(again, got)), f"{what}: the second call differs"
    return got


@pytest.mark.parametrize("name", list(EDGES))
def test_det_form_at_an_edge_vs_float64(name, deterministic):
    """Mode on: the call launches the deterministic entry point once, meets that builder's float64 bar, and a second call on the
    same inputs is torch.equal to the first."""
    entry, build = EDGES[name]
    _run_twice_and_check(entry, build(), name)


def test_optional_outputs_reach_the_library_as_null(deterministic):
    """The two cases above that leave an optional parameter out hand the library NULL for its gradient - the finish kernel's
    `o1` (kDetDw) and `o1` / `o2` (kDetScan) branches are the ones those cases run, not a host-side substitute buffer."""
    with launch_spy() as seen:
        EDGES["dwconv-nobias"][1]().run()
        EDGES["selscan-N7-plain"][1]().run()
    a = seen.args[seen.index("wm_dwconv3x3_wgrad_det")]                 # x, gy, dW, db, workspace, ...
    assert a[2] is not None and a[3] is None
    a = seen.args[seen.index("wm_selscan_bwd_det")]                     # u, delta, A, B, C, D, delta_bias, dout, du, ddelta, dA, dB, dC, dD, dbias
    assert a[5] is None and a[6] is None and a[10] is not None and a[13] is None and a[14] is None


@pytest.mark.parametrize("name", list(MISALIGNED))
def test_det_form_on_planes_off_the_16_byte_grid(name, deterministic):
    """The same problem from 16-byte aligned tensors and from views one float into a larger buffer: both meet the float64 bar, the
    second call of each is torch.equal, and the two results agree within the bar of that builder (they may differ in summation
    order: another grid)."""
    entry, build = MISALIGNED[name]
    bar = {"dwconv": 2e-5, "layernorm2d": 5e-5, "gather": 0.0}[name]      # the builders' bars (_dwconv, _layernorm2d); the gather adds
    aligned = _run_twice_and_check(entry, build(False), name + " aligned")              # in ascending j in both forms: the same bits
    shifted = _run_twice_and_check(entry, build(True), name + " misaligned")
    for a, s in zip(aligned, shifted):
        if bar:
            assert_close(s, a, bar, f"{name}: misaligned against aligned")
        else:
            assert torch.equal(s, a), f"{name}: misaligned differs from aligned"


def test_channel_gather_refuses_more_than_1024_gathered_channels(deterministic):
    x = torch.randn(1, 4, 4, device=DEV, requires_grad=True)
    idx = torch.zeros(1, ops.CHANNEL_GATHER_MAX_M + 1, dtype=torch.int32, device=DEV)
    assert ops.channel_gather(x, idx[:, :ops.CHANNEL_GATHER_MAX_M]).shape == (1, ops.CHANNEL_GATHER_MAX_M, 4)
    with pytest.raises(NotImplementedError):
        ops.channel_gather(x, idx)


# name -> (builder of the operator at batch 0 (T = 0 for the token operators), indices of the PARAMETER gradients in run()'s result).
# Every operator here takes an empty batch with the mode off (a mode-off call that raises fails the test); l1_mean refuses an empty
# input by design, in both modes: test_l1_mean_refuses_an_empty_input.
EMPTY = {
    "dwconv": (lambda: _dwconv((0, 5, 7, 9)), (0, 1)),
    "dwconv-nobias": (lambda: _dwconv((0, 5, 7, 9), bias=False), (0,)),
    "layernorm2d": (lambda: _layernorm2d((0, 16, 5, 7)), (1, 2)),
    "layernorm_tok": (lambda: _layernorm_tok((0, 16)), (1, 2)),
    "linear": (lambda: _linear(0, 64, 16), (0,)),
    "plane_sums": (lambda: _plane_sums((0, 3, 1, 5)), (0,)),
    "scale_add": (lambda: _scale_add((0, 8, 5, 7)), (0,)),
    "selscan": (lambda: _selscan(0, 8, 20, 4, 2), (2, 5, 6)),                # dA, dD, dbias
    "gather": (lambda: _gather("maps", 0, 3, 5, (3,), idx=torch.zeros(0, 5, dtype=torch.int32)), ()),
}


def _dirty_the_allocator():
    """Fill and free small blocks, so that the torch.empty outputs of the next calls come back holding NaN, not zeros."""
    blocks = [torch.full((n,), float("nan"), device=DEV) for n in (16, 64, 128, 256, 512, 1024, 2048) for _ in range(8)]
    torch.cuda.synchronize()
    del blocks


@pytest.mark.parametrize("name", list(EMPTY))
def test_empty_problem_gives_zero_parameter_gradients(name):
    """An operator that accepts an empty batch with the mode off must, with the mode on, return parameter gradients that are
    exactly zero: the outputs are torch.empty in the mode, so the library zeroes them itself."""
    build, params = EMPTY[name]
    c = build()
    c.run()                                                  # mode off: every operator of EMPTY takes an empty batch
    torch.cuda.synchronize()
    prev = wm.set_deterministic(True)
    try:
        _dirty_the_allocator()
        got = c.run()
        torch.cuda.synchronize()
    finally:
        wm.set_deterministic(prev)
    for i in params:
        assert got[i].numel() > 0 and bool(torch.isfinite(got[i]).all()) and float(got[i].abs().max()) == 0.0, \
            f"{name}: output {i} of an empty problem is not zero: {got[i].flatten()[:8].tolist()}"
    assert all(t.numel() == 0 for i, t in enumerate(got) if i not in params)


@pytest.mark.parametrize("on", [False, True], ids=["mode_off", "mode_on"])
def test_l1_mean_refuses_an_empty_input(on):
    """The mean of nothing: ops.l1_mean raises RuntimeError before any launch, whatever the mode."""
    a = torch.empty(0, device=DEV)
    prev = wm.set_deterministic(on)
    try:
        with launch_spy() as names, pytest.raises(RuntimeError, match="empty input"):
            ops.l1_mean(a, a.clone())
    finally:
        wm.set_deterministic(prev)
    assert names == []


# ------------------------------------------------------------------------------------------------
# D. status codes of the _det entry points and the gathers, from real calls
# ------------------------------------------------------------------------------------------------
SENTINEL = 12345.0


def _rand(*shape):
    return torch.randn(*shape, device=DEV)


def _out(*shape):
    return torch.full(shape, SENTINEL, device=DEV)


def _det_call(name):
    """-> (workspace bytes of the good problem, the output tensors, call(ws pointer, ws bytes, negative=False) -> status) for one
    wm_*_det entry point on real device buffers; negative: the first size is -1."""
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    if name == "wm_dwconv3x3_wgrad_det":
        B, C, H, W = 2, 4, 6, 8
        x, gy, outs = _rand(B, C, H, W), _rand(B, C, H, W), [_out(C, 1, 3, 3), _out(C)]
        return lib.wm_dwconv3x3_wgrad_det_workspace_bytes(B, C, H, W), outs, lambda ws, nb, neg=False: lib.wm_dwconv3x3_wgrad_det(
            p(x), p(gy), p(outs[0]), p(outs[1]), ws, nb, -1 if neg else B, C, H, W, st)
    if name == "wm_layernorm2d_bwd_det":
        B, L, C = 2, 35, 16
        x, w, gy, outs = _rand(B, C, L), _rand(C), _rand(B, C, L), [_out(B, C, L), _out(C), _out(C)]
        return lib.wm_layernorm2d_bwd_det_workspace_bytes(B, L, C), outs, lambda ws, nb, neg=False: lib.wm_layernorm2d_bwd_det(
            p(x), p(w), p(gy), 1e-6, p(outs[0]), p(outs[1]), p(outs[2]), ws, nb, -1 if neg else B, L, C, st)
    if name == "wm_layernorm_tok_bwd_det":
        T, C = 37, 16
        x, w, gy, outs = _rand(T, C), _rand(C), _rand(T, C), [_out(T, C), _out(C), _out(C)]
        return lib.wm_layernorm_tok_bwd_det_workspace_bytes(T, C), outs, lambda ws, nb, neg=False: lib.wm_layernorm_tok_bwd_det(
            p(x), p(w), p(gy), 1e-5, p(outs[0]), p(outs[1]), p(outs[2]), ws, nb, -1 if neg else T, C, st)
    if name == "wm_linear_wgrad_det":
        T, O, I = 100, 16, 16
        gy, x, outs = _rand(T, O), _rand(T, I), [_out(O, I)]
        return lib.wm_linear_wgrad_det_workspace_bytes(T, O, I), outs, lambda ws, nb, neg=False: lib.wm_linear_wgrad_det(
            p(gy), p(x), p(outs[0]), ws, nb, -1 if neg else T, O, I, st)
    if name == "wm_plane_sums_det":
        B, C, H, W = 2, 3, 5, 7
        x, outs = _rand(B, C, H, W), [_out(C)]
        return lib.wm_plane_sums_det_workspace_bytes(B, C, H, W), outs, lambda ws, nb, neg=False: lib.wm_plane_sums_det(
            p(x), p(outs[0]), ws, nb, -1 if neg else B, C, H, W, st)
    if name == "wm_scale_add_bwd_det":
        B, C, L = 2, 4, 35
        g, x, s, outs = _rand(B, C, L), _rand(B, C, L), _rand(C), [_out(B, C, L), _out(C)]
        return lib.wm_scale_add_bwd_det_workspace_bytes(B, C, L), outs, lambda ws, nb, neg=False: lib.wm_scale_add_bwd_det(
            p(g), p(x), p(s), p(outs[0]), p(outs[1]), ws, nb, -1 if neg else B, C, L, st)
    if name == "wm_l1_mean_fwd_det":
        n = 1000
        a, b, outs = _rand(n), _rand(n), [_out(1)]
        return lib.wm_l1_mean_fwd_det_workspace_bytes(n), outs, lambda ws, nb, neg=False: lib.wm_l1_mean_fwd_det(
            p(a), p(b), p(outs[0]), ws, nb, -1 if neg else n, st)
    assert name == "wm_selscan_bwd_det"
    batch, dim, L, N, G = 1, 8, 20, 4, 2
    u, dl, A, Bm, Cm, D, bias, dy = (_rand(batch, dim, L), _rand(batch, dim, L), -torch.rand(dim, N, device=DEV), _rand(batch, G, N, L),
                                     _rand(batch, G, N, L), _rand(dim), _rand(dim), _rand(batch, dim, L))
    outs = [_out(batch, dim, L), _out(batch, dim, L), _out(dim, N), _out(batch, G, N, L), _out(batch, G, N, L), _out(dim), _out(dim)]
    return lib.wm_selscan_bwd_det_workspace_bytes(batch, dim, L, N, G), outs, lambda ws, nb, neg=False: lib.wm_selscan_bwd_det(
        p(u), p(dl), p(A), p(Bm), p(Cm), p(D), p(bias), p(dy), *[p(o) for o in outs], ws, nb, -1 if neg else batch, dim, L, N, G, 1, st)


DET_ENTRIES = ["wm_dwconv3x3_wgrad_det", "wm_layernorm2d_bwd_det", "wm_layernorm_tok_bwd_det", "wm_linear_wgrad_det", "wm_plane_sums_det",
               "wm_scale_add_bwd_det", "wm_l1_mean_fwd_det", "wm_selscan_bwd_det"]


def test_every_det_entry_point_of_the_binding_is_covered():
    bound = sorted(n for n in _lib.SIGNATURES if n.endswith("_det"))
    assert bound == sorted(DET_ENTRIES), bound


@pytest.mark.parametrize("name", DET_ENTRIES)
def test_det_abi_status_codes_from_real_calls(name):
    """In the style of test_core_abi_error_codes_from_real_calls: every case is a refusal that returns before any launch, and the
    sentinel-filled outputs are unchanged after each - a workspace one byte short of the _workspace_bytes answer -> WM_EWORKSPACE,
    a NULL workspace on a non-empty problem -> WM_ENULL, a negative size -> WM_EINVAL."""
    need, outs, call = _det_call(name)
    assert need > 0
    ws = torch.empty(need + 64, dtype=torch.uint8, device=DEV)

    def untouched():
        torch.cuda.synchronize()
        return all(bool((o == SENTINEL).all()) for o in outs)
    assert call(ws.data_ptr(), need - 1) == _lib.WM_EWORKSPACE and untouched()
    assert call(None, need) == _lib.WM_ENULL and untouched()
    assert call(None, 0) == _lib.WM_ENULL and untouched()
    assert call(ws.data_ptr(), need, True) == _lib.WM_EINVAL and untouched()


def test_channel_gather_abi_status_codes_from_real_calls():
    """wm_channel_gather_fwd / _bwd: M = 1025 in the backward -> WM_EUNSUPPORTED, a pointer off by 2 bytes -> WM_EALIGN, C = 0 with
    something to gather in the forward -> WM_EINVAL; the sentinel-filled outputs are unchanged after each refusal."""
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    B, C, M, HW = 1, 2, 1025, 4
    x, gy, idx = _rand(B, C, HW), _rand(B, M, HW), torch.zeros(B, M, dtype=torch.int32, device=DEV)
    y, gx = _out(B, M, HW), _out(B, C, HW)
    p = lambda t: t.data_ptr()

    def untouched():
        torch.cuda.synchronize()
        return bool((y == SENTINEL).all()) and bool((gx == SENTINEL).all())
    assert lib.wm_channel_gather_bwd(p(gy), p(idx), p(gx), B, C, M, HW, st) == _lib.WM_EUNSUPPORTED and untouched()
    assert lib.wm_channel_gather_bwd(p(gy) + 2, p(idx), p(gx), B, C, 5, HW, st) == _lib.WM_EALIGN and untouched()
    assert lib.wm_channel_gather_bwd(p(gy), p(idx), p(gx) + 2, B, C, 5, HW, st) == _lib.WM_EALIGN and untouched()
    assert lib.wm_channel_gather_fwd(p(x) + 2, p(idx), p(y), B, C, 5, HW, st) == _lib.WM_EALIGN and untouched()
    assert lib.wm_channel_gather_fwd(p(x), p(idx), p(y) + 2, B, C, 5, HW, st) == _lib.WM_EALIGN and untouched()
    assert lib.wm_channel_gather_fwd(p(x), p(idx), p(y), B, 0, 5, HW, st) == _lib.WM_EINVAL and untouched()
    assert lib.wm_channel_gather_fwd(p(x), p(idx), p(y), B, C, -1, HW, st) == _lib.WM_EINVAL and untouched()
