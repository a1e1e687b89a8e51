"""The training convolutions on wide-range operands, every output element judged against the a-priori bound of conv_range.py.

conv2d_f16 (forward and input gradient) rests on a magnitude pass that must find the largest element wherever it lies, and on fp16
subnormals surviving the split's conversion and the matrix instruction; conv2d_wgrad on all three products of its bf16 split.  A
whole-tensor norm sees none of it (test_conv_range_cpu.py).  References and bounds are float64 on the CPU, computed once per case."""
import functools

import pytest
import torch
import torch.nn.functional as F

import wave_mamba_amd as wm
from conftest import assert_close
import conv_range as cr
from test_deterministic_gpu import _off16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SELECT = {"first_gen": wm.ops.CONV3X3_FIRST_GEN, "wave_specialised": wm.ops.CONV3X3_WAVE_SPECIALISED}


class _select:
    """The 3x3 kernel pinned for the block (None: the library's own choice - the 1x1 has one kernel), CONV3X3_AUTO afterwards."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if self.name is not None:
            wm.ops.conv2d_select(SELECT[self.name])

    def __exit__(self, *exc):
        wm.ops.conv2d_select(wm.ops.CONV3X3_AUTO)


def _seed(ks, Cin, Cout, H):
    return ks * 1000 + Cin + Cout + H


@functools.lru_cache(maxsize=None)
def _fwd_case(ks, Cin, Cout, plane):
    """banded x, banded weight, a bias; float64 results and bounds with and without the bias.  The bias is randn on the even channels
    and 2^-24 of that on the odd ones: next to a bias of magnitude 1 the bound is the bias's own rounding (6e-8) and says nothing
    about the quiet regions; the small one keeps them judged, and a bias read from the wrong channel is an error of its whole size."""
    B, H, W = plane
    x = cr.banded((B, Cin, H, W), _seed(ks, Cin, Cout, H))
    w = cr.banded_weight(Cout, Cin, ks, ks * 77 + Cin * 5 + Cout)
    b = torch.randn(Cout, generator=torch.Generator().manual_seed(Cout))
    b[1::2] *= 2.0 ** -24
    return (x, w, b, {False: cr.conv_ref64(x, w, ks), True: cr.conv_ref64(x, w, ks, b)},
            {False: cr.conv_bound(x, w, ks, "f16"), True: cr.conv_bound(x, w, ks, "f16", b)})


@functools.lru_cache(maxsize=None)
def _dgrad_case(ks, Cin, Cout, plane):
    """banded gy over the Cout channels, banded forward weight; the float64 input gradient and its bound (Cin and Cout exchanged)."""
    B, H, W = plane
    gy = cr.banded((B, Cout, H, W), _seed(ks, Cin, Cout, H) + 5)
    w = cr.banded_weight(Cout, Cin, ks, ks * 77 + Cin * 5 + Cout)
    wt = cr.dgrad_weight(w)
    return gy, w, cr.conv_ref64(gy, wt, ks), cr.conv_bound(gy, wt, ks, "f16")


# ------------------------------------------------------------------------------------------------
# a. forward, every fp16 launch form of conv2d_walk
# ------------------------------------------------------------------------------------------------
PLANES = [(2, 24, 40), (2, 9, 33)]
FWD_3X3 = [(16, 64), (16, 32), (32, 96), (3, 32), (32, 3)]       # two row tiles, one, 2 + 1, ragged input chunk, ragged row tile
FWD_1X1 = [(32, 96), (16, 64), (12, 32)]                         # three row tiles in one launch, two, one (ragged input chunk)
FWD_CASES = ([(3, sel, ci, co, pl) for sel in SELECT for ci, co in FWD_3X3 for pl in PLANES]
             + [(3, sel, 16, 32, (1, 5, 7)) for sel in SELECT]
             + [(1, None, ci, co, pl) for ci, co in FWD_1X1 for pl in PLANES] + [(1, None, 16, 64, (1, 5, 7))])


@pytest.mark.parametrize("ks,select,Cin,Cout,plane", FWD_CASES)
def test_conv2d_f16_forward_per_element(ks, select, Cin, Cout, plane):
    """conv2d_f16 on banded operands against the float64 convolution, per element, with and without a bias; bit-equal run to run."""
    x, w, b, refs, bounds = _fwd_case(ks, Cin, Cout, plane)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    with _select(select):
        for bias in (False, True):
            got = wm.ops.conv2d_f16(xd, wd, bd if bias else None)
            again = wm.ops.conv2d_f16(xd, wd, bd if bias else None)
            aten = F.conv2d(xd, wd, bd if bias else None, padding=ks // 2)
            what = f"conv2d_f16 ks={ks} {select or '1x1'} {Cin}->{Cout} {plane} bias={bias}"
            r_got, at = cr.worst_ratio(got, refs[bias], bounds[bias])
            r_aten, _ = cr.worst_ratio(aten, refs[bias], bounds[bias])
            print(f"{what}: worst error / bound {r_got:.3g} at {at} (ATen fp32: {r_aten:.3g})")
            cr.assert_within(got, refs[bias], bounds[bias], what)
            assert torch.equal(again, got), f"{what}: not reproducible run to run"


# ------------------------------------------------------------------------------------------------
# b. the input-gradient form
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks,select,Cin,Cout", [(3, sel, ci, co) for sel in SELECT for ci, co in ((16, 64), (3, 32))] + [(1, None, 32, 96)])
def test_conv2d_f16_input_gradient_per_element(ks, select, Cin, Cout):
    """conv2d_f16(gy, w, dgrad=True) on a banded gy and a banded forward weight against the float64 input gradient, per element."""
    gy, w, ref, bound = _dgrad_case(ks, Cin, Cout, (2, 24, 40))
    gyd, wd = gy.to(DEV), w.to(DEV)
    with _select(select):
        got = wm.ops.conv2d_f16(gyd, wd, dgrad=True)
        again = wm.ops.conv2d_f16(gyd, wd, dgrad=True)
        aten = F.conv2d(gyd, cr.dgrad_weight(wd), padding=ks // 2)
    what = f"conv2d_f16 dgrad ks={ks} {select or '1x1'} {Cin}->{Cout}"
    r_got, at = cr.worst_ratio(got, ref, bound)
    print(f"{what}: worst error / bound {r_got:.3g} at {at} (ATen fp32: {cr.worst_ratio(aten, ref, bound)[0]:.3g})")
    cr.assert_within(got, ref, bound, what)
    assert torch.equal(again, got), f"{what}: not reproducible run to run"


# ------------------------------------------------------------------------------------------------
# c. through autograd
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks", [3, 1])
def test_conv2d_train_f16_gradients_per_element(ks):
    """conv2d_train under set_train_conv_mode("f16"), x, w and gy banded: the forward and gx per element with the fp16 bound, gw per
    entry with the bf16 weight-gradient bound (W % 32 == 0: conv2d_wgrad serves it), gb against the float64 sums."""
    B, Cin, Cout, H, W = 2, 16, 32, 8, 32
    x, w, b, refs, bounds = _fwd_case(ks, Cin, Cout, (B, H, W))
    gy = cr.banded((B, Cout, H, W), 4242 + ks)
    xq, wq, bq = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
    assert wm.ops.conv2d_wgrad_supported(xq, wq), "the weight gradient of this shape must be the HIP kernel's"
    prev = wm.ops.set_train_conv_mode("f16")
    try:
        y = wm.ops.conv2d_train(xq, wq, bq)
        gx, gw, gb = torch.autograd.grad(y, (xq, wq, bq), gy.to(DEV))
    finally:
        wm.ops.set_train_conv_mode(prev)
    wt = cr.dgrad_weight(w)
    for what, got, ref, bound in (("forward", y, refs[True], bounds[True]),
                                  ("gx", gx, cr.conv_ref64(gy, wt, ks), cr.conv_bound(gy, wt, ks, "f16")),
                                  ("gw", gw, cr.wgrad_ref64(gy, x, ks), cr.wgrad_bound(gy, x, ks))):
        r, at = cr.worst_ratio(got, ref, bound)
        print(f"conv2d_train f16 ks={ks} {what}: worst error / bound {r:.3g} at {at}")
        cr.assert_within(got, ref, bound, f"conv2d_train f16 ks={ks} {what}")
    assert_close(gb, gy.double().sum((0, 2, 3)).float().to(DEV), 1e-5, f"conv2d_train f16 ks={ks} gb")


# ------------------------------------------------------------------------------------------------
# d. the weight-gradient kernel alone
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks,B,Cin,Cout,H,W", [(3, 2, 64, 64, 8, 32), (3, 2, 3, 32, 6, 32), (1, 2, 32, 64, 4, 64), (1, 1, 192, 32, 3, 32)])
def test_conv2d_wgrad_per_entry(ks, B, Cin, Cout, H, W):
    """wm_conv2d_wgrad on banded gy and x against the float64 weight gradient, per entry of dW with the bf16 bound."""
    gy = cr.banded((B, Cout, H, W), ks * 1000 + Cin * 7 + Cout + H)
    x = cr.banded((B, Cin, H, W), ks * 1000 + Cin * 7 + Cout + H + 1)
    ref, bound = cr.wgrad_ref64(gy, x, ks), cr.wgrad_bound(gy, x, ks)
    got = wm.ops.conv2d_wgrad(gy.to(DEV), x.to(DEV), ks)
    aten = torch.ops.aten.convolution_backward(gy.to(DEV), x.to(DEV), torch.zeros(Cout, Cin, ks, ks, device=DEV), None, [1, 1],
                                               [ks // 2, ks // 2], [1, 1], False, [0, 0], 1, [False, True, False])[1]
    what = f"conv2d_wgrad ks={ks} {B}x{Cin}->{Cout} {H}x{W}"
    r, at = cr.worst_ratio(got, ref, bound)
    print(f"{what}: worst error / bound {r:.3g} at {at} (ATen fp32: {cr.worst_ratio(aten, ref, bound)[0]:.3g})")
    cr.assert_within(got, ref, bound, what)
    assert torch.equal(wm.ops.conv2d_wgrad(gy.to(DEV), x.to(DEV), ks), got), f"{what}: not reproducible run to run"


# ------------------------------------------------------------------------------------------------
# e. the magnitude pass
# ------------------------------------------------------------------------------------------------
def _amax_walk(nx):
    """The pass over x of cv_amax_prep_kernel for an aligned x of nx elements, from the launcher's rule (wm_conv2d_f16_steps):
    -> (workgroups, stride in quads, quads, unrolled trips of thread 0, first quad only the remainder loop reaches)."""
    nq = nx // 4
    wgs = min(max(-(-nq // 2048), 1), 512)
    stride = 256 * wgs
    trips = {i0: len(range(i0, max(nq - 3 * stride, i0), 4 * stride)) for i0 in (0, stride - 1)}
    assert trips[0] == trips[stride - 1], "every thread makes the same number of unrolled trips at the sizes used here"
    return wgs, stride, nq, trips[0], 4 * stride * trips[0]


def _peak_positions(shape):
    """Flat positions of the ONE large element, by the loop that has to find it."""
    nx = 1
    for d in shape:
        nx *= d
    wgs, stride, nq, trips, rem0 = _amax_walk(nx)
    pos = {"first": 0, "last": nx - 1}
    if trips:
        for k, name in ((1, "second load"), (2, "third load"), (3, "fourth load")):
            pos[name] = 4 * (k * stride + (77 * k) % stride) + k            # a quad of the k-th further load, component k
    if rem0 < nq:
        pos["remainder loop"] = 4 * (rem0 + (nq - rem0) // 2) + 2
        pos["remainder loop, last quad"] = 4 * (nq - 1)
    return pos, (wgs, stride, nq, trips, rem0)


AMAX_X = [((1, 16, 40, 52), 3, 32), ((1, 16, 40, 52), 1, 32), ((1, 3, 7, 9), 3, 32)]


@pytest.mark.parametrize("shape,ks,Cout", AMAX_X)
def test_magnitude_pass_finds_the_largest_input_element_wherever_it_lies(shape, ks, Cout):
    """x = randn with ONE element at +-2^22 (the sign alternates over the positions): were the magnitude pass to miss it, the scale
    would come from the randn part (2^12), the element would be 2^34 in fp16 - Inf - and its neighbourhood Inf / NaN.

    Positions, from the launcher's rule (workgroups = clamp(ceil(floor(nx / 4) / 2048), 1, 512), stride = 256 x workgroups quads):
      (1, 16, 40, 52): nx = 33280, 8320 quads, 5 workgroups, stride 1280: ONE unrolled trip (quads i, i + 1280, i + 2560, i + 3840 for
        i < 1280), then the remainder loop over quads 5120 .. 8319, no scalar tail.  Elements 0; 5429 (quad 1357: second load),
        10858 (quad 2714: third), 16287 (quad 4071: fourth); 26882 (quad 6720: the remainder loop alone) and 33276 (quad 8319, its
        last); 33279 (the last element).
      (1, 3, 7, 9): nx = 189 = 4 x 47 + 1, one workgroup, no unrolled trip: elements 0, 94 (quad 23, remainder loop), 184 (quad 46),
        and 188 - the scalar tail's only element.
    Each also as a contiguous view 4 bytes off a 16-byte boundary: the pass takes its all-scalar form and the convolution kernels
    load single floats, so the library accepts the call (wm_conv2d_f16_steps checks the alignment of the fragments alone) and the
    result must be the aligned call's, bit for bit."""
    Cin = shape[1]
    pos, (wgs, stride, nq, trips, rem0) = _peak_positions(shape)
    if shape == (1, 16, 40, 52):
        assert (wgs, stride, nq, trips, rem0) == (5, 1280, 8320, 1, 5120)
        assert pos == {"first": 0, "second load": 5429, "third load": 10858, "fourth load": 16287, "remainder loop": 26882,
                       "remainder loop, last quad": 33276, "last": 33279}
    else:
        assert (wgs, nq, trips, rem0) == (1, 47, 0, 0) and pos == {"first": 0, "remainder loop": 94, "remainder loop, last quad": 184, "last": 188}
    g = torch.Generator().manual_seed(shape[1] + ks)
    base = torch.randn(*shape, generator=g)
    w = torch.randn(Cout, Cin, ks, ks, generator=g) / (ks * Cin ** 0.5)
    wd = w.to(DEV)
    for n, (name, p) in enumerate(pos.items()):
        x = base.clone()
        x.view(-1)[p] = (-1.0) ** n * 2.0 ** 22
        ref, bound = cr.conv_ref64(x, w, ks), cr.conv_bound(x, w, ks, "f16")
        what = f"peak at element {p} ({name}) of {shape}, ks={ks}"
        got = wm.ops.conv2d_f16(x.to(DEV), wd)
        assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite outputs - the magnitude pass missed it"
        r = cr.assert_within(got, ref, bound, what)
        xo = _off16(x)
        got_o = wm.ops.conv2d_f16(xo, wd)
        assert torch.equal(got_o, got), f"{what}: the 16-byte-misaligned view differs from the aligned call"
        print(f"{what}: worst error / bound {r:.3g}; misaligned view bit-equal")


@pytest.mark.parametrize("ks,Cin,Cout,nprep", [(1, 16, 32, 1), (3, 16, 32, 3), (3, 64, 64, 18), (3, 96, 96, 32), (3, 3, 3, 3)])
def test_magnitude_pass_finds_the_largest_weight_element_in_every_preparing_workgroup(ks, Cin, Cout, nprep):
    """The weight with ONE element at 2^22 times the rest, first, last and (3 -> 3 at 3x3: nw = 81 = 4 x 20 + 1) in the scalar tail of
    the pass over w.  Every preparing workgroup takes max |w| for itself and scales its share of the fragments by it: 1, 3, 18 and
    32 of them (wm_conv2d_f16_steps: ~512 fragment items each, at most 32).  A workgroup that missed the element would write Inf."""
    items = -(-Cin // 16) * ks * ks * -(-Cout // 32) * 128
    assert (1 if items <= 512 else 32 if items >= 32 * 512 else -(-items // 512)) == nprep
    g = torch.Generator().manual_seed(Cin + Cout + ks)
    x = torch.randn(1, Cin, 4, 8, generator=g)
    base = torch.randn(Cout, Cin, ks, ks, generator=g) / (ks * Cin ** 0.5)
    nw = base.numel()
    positions = {"first": 0, "last": nw - 1, "middle": 4 * (nw // 8) + 1}
    if nw % 4:
        assert (nw, nw - 1) == (81, 80)                                   # the scalar tail's only element is the last one
    xd = x.to(DEV)
    for n, (name, p) in enumerate(positions.items()):
        for dgrad in (False, True):
            # `passed` is the tensor the pass reads (position p is a position in ITS memory); dgrad: the forward weight of the
            # convolution whose input gradient is conv(x, w)
            passed = (cr.dgrad_weight(base) if dgrad else base).clone()
            passed.view(-1)[p] *= (-1.0) ** n * 2.0 ** 22
            w = cr.dgrad_weight(passed) if dgrad else passed
            ref, bound = cr.conv_ref64(x, w, ks), cr.conv_bound(x, w, ks, "f16")
            what = f"weight peak at element {p} ({name}) of {nw}, ks={ks} {Cin}->{Cout} dgrad={dgrad}"
            got = wm.ops.conv2d_f16(xd, passed.to(DEV), dgrad=dgrad)
            assert bool(torch.isfinite(got).all()), f"{what}: non-finite outputs - a preparing workgroup missed it"
            r = cr.assert_within(got, ref, bound, what)
            print(f"{what}: worst error / bound {r:.3g}")


# ------------------------------------------------------------------------------------------------
# f. non-finite elements
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks,select", [(3, "first_gen"), (3, "wave_specialised"), (1, None)])
def test_conv2d_f16_non_finite_elements_stay_local(ks, select):
    """conv2d.hip.h: the magnitude pass takes its maximum over the FINITE elements, so one +Inf, one -Inf and one NaN in x leave the
    scale to the largest finite element (1e5 here - above fp16's range at scale 1).  Outputs that touch none of the three are finite
    and within the bound (Xmax over the finite elements) of the float64 convolution of x with the three zeroed; outputs that touch
    one are non-finite."""
    B, Cin, Cout, H, W = 2, 16, 32, 9, 33
    g = torch.Generator().manual_seed(99 + ks)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, ks, ks, generator=g) / (ks * Cin ** 0.5)
    x[0, 2, 4, 20] = 1.0e5
    bad = {(0, 0, 0, 0): float("inf"), (1, 9, 5, 32): float("-inf"), (0, 15, 8, 11): float("nan")}
    x0 = x.clone()
    for idx, v in bad.items():
        x[idx] = v
        x0[idx] = 0.0
    touched = F.conv2d((~torch.isfinite(x)).double().sum(1, keepdim=True), torch.ones(1, 1, ks, ks, dtype=torch.float64), padding=ks // 2) > 0
    assert int(touched.sum()) == {3: 4 + 6 + 6, 1: 3}[ks]                  # a corner, a right-edge and a bottom-edge window
    touched = touched.expand(B, Cout, H, W)
    ref, bound = cr.conv_ref64(x0, w, ks), cr.conv_bound(x, w, ks, "f16")
    assert torch.equal(bound, cr.conv_bound(x0, w, ks, "f16"))
    with _select(select):
        got = wm.ops.conv2d_f16(x.to(DEV), w.to(DEV)).cpu()
    what = f"non-finite elements, ks={ks} {select or '1x1'}"
    assert not bool(torch.isfinite(got[touched]).any()), f"{what}: {int(torch.isfinite(got[touched]).sum())} outputs touching an Inf / NaN are finite"
    assert bool(torch.isfinite(got[~touched]).all()), f"{what}: {int((~torch.isfinite(got[~touched])).sum())} untouched outputs are not finite"
    r = cr.assert_within(torch.where(touched, ref, got.double()), ref, bound, what)
    print(f"{what}: worst error / bound of the untouched outputs {r:.3g}")
