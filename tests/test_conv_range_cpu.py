"""The per-element bound of conv_range.py, held against the documented arithmetic emulated on the CPU: it must admit the honest form
and must NOT admit a form that flushes fp16 subnormals or leaves out one of the three products - else the GPU tests that use it
(test_conv_range_gpu.py) would be vacuous or could never pass.  No GPU.

Figures (worst error / bound over every output element; printed by the tests, recorded in profiles/conv_range/README.md):
    honest fp16 form   3x3 16 -> 64 on (2, ., 24, 40): 0.14     1x1 32 -> 96: 0.25     input gradient 3x3 64 -> 16: 0.06
    flushing form                                      192                    447                                  100
    without lo * hi                                    101                    121                                   51
    ATen fp32 (CPU)                                    0.13                   0.12                                  0.05
    weight gradient, bf16 form, 3x3 2 x 64 -> 64 on 8 x 32: honest 0.10, without lo * hi 40
(the last digits depend on the host's fp32 summation order; the assertions leave a factor of four or more on either side)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import conv_range as cr

# operands of test_conv_range_gpu.py: (ks, Cin, Cout, map)
CASES = [(3, 16, 64, (2, 24, 40)), (3, 32, 96, (2, 9, 33)), (3, 3, 32, (2, 24, 40)), (1, 32, 96, (2, 24, 40)), (1, 12, 32, (2, 9, 33))]


@functools.lru_cache(maxsize=None)
def _operands(ks, Cin, Cout, plane, dgrad):
    """(x, weight of the convolution that runs, float64 result, bound, quiet-output mask); dgrad: x is a banded gy over Cout channels
    and the convolution is the input gradient's, on the transposed, rotated banded weight."""
    B, H, W = plane
    if dgrad:
        x = cr.banded((B, Cout, H, W), seed=ks * 1000 + Cin + Cout + H)
        w = cr.dgrad_weight(cr.banded_weight(Cout, Cin, ks, seed=ks * 77 + Cin * 5 + Cout))
    else:
        x = cr.banded((B, Cin, H, W), seed=ks * 1000 + Cin + Cout + H)
        w = cr.banded_weight(Cout, Cin, ks, seed=ks * 77 + Cin * 5 + Cout)
    return x, w, cr.conv_ref64(x, w, ks), cr.conv_bound(x, w, ks, "f16"), cr.quiet_outputs(tuple(x.shape))


@pytest.mark.parametrize("dgrad", [False, True])
@pytest.mark.parametrize("ks,Cin,Cout,plane", CASES)
def test_bound_admits_the_documented_fp16_form_and_no_broken_one(ks, Cin, Cout, plane, dgrad):
    x, w, ref, bound, quiet = _operands(ks, Cin, Cout, plane, dgrad)
    what = f"ks={ks} {Cin}->{Cout} {plane}{' dgrad' if dgrad else ''}"
    honest = cr.assert_within(cr.emulate_conv(x, w, ks), ref, bound, f"honest emulation {what}")
    aten, _ = cr.worst_ratio(F.conv2d(x, w, padding=ks // 2), ref, bound)
    flushed = cr.emulate_conv(x, w, ks, flush=True)
    r_flush, at = cr.worst_ratio(flushed, ref, bound)
    # ... and the excess lies in the quiet regions: judged there alone it is as large
    qmask = quiet.expand_as(ref)
    r_quiet, _ = cr.worst_ratio(torch.where(qmask, flushed.double(), ref), ref, bound)
    frac = float(((flushed.double() - ref).abs() > bound).double().mean())
    dropped = {p: cr.worst_ratio(cr.emulate_conv(x, w, ks, drop=p), ref, bound)[0] for p in cr.PRODUCTS[1:]}
    print(f"{what}: honest {honest:.2f}, ATen fp32 {aten:.2f}, flushing {r_flush:.0f} at {at} ({100 * frac:.0f} % of the elements over), "
          f"quiet regions alone {r_quiet:.0f}, without " + ", ".join(f"{p}: {v:.0f}" for p, v in dropped.items()))
    assert aten <= 1.0, f"{what}: ATen's fp32 convolution itself misses the bound ({aten:.2f}): the bound is too tight"
    assert r_quiet >= 10.0, f"{what}: flushing fp16 subnormals stays within 10x the bound in the quiet regions ({r_quiet:.2f})"
    for p, v in dropped.items():
        assert v > 1.0, f"{what}: the form without the {p} product stays within the bound ({v:.2f})"


@functools.lru_cache(maxsize=None)
def _wgrad_operands(ks, B, Cin, Cout, H, W):
    gy = cr.banded((B, Cout, H, W), seed=ks * 1000 + Cin * 7 + Cout + H)
    x = cr.banded((B, Cin, H, W), seed=ks * 1000 + Cin * 7 + Cout + H + 1)
    return gy, x, cr.wgrad_ref64(gy, x, ks), cr.wgrad_bound(gy, x, ks)


@pytest.mark.parametrize("ks,B,Cin,Cout,H,W", [(3, 2, 64, 64, 8, 32), (3, 2, 3, 32, 6, 32), (1, 2, 32, 64, 4, 64), (1, 1, 192, 32, 3, 32)])
def test_bound_admits_the_documented_bf16_weight_gradient_and_no_broken_one(ks, B, Cin, Cout, H, W):
    gy, x, ref, bound = _wgrad_operands(ks, B, Cin, Cout, H, W)
    what = f"wgrad ks={ks} {B}x{Cin}->{Cout} {H}x{W}"
    honest = cr.assert_within(cr.emulate_wgrad(gy, x, ks), ref, bound, f"honest emulation {what}")
    dropped = {p: cr.worst_ratio(cr.emulate_wgrad(gy, x, ks, drop=p), ref, bound)[0] for p in cr.PRODUCTS[1:]}
    print(f"{what}: honest {honest:.2f}, without " + ", ".join(f"{p}: {v:.0f}" for p, v in dropped.items()))
    for p, v in dropped.items():
        assert v > 1.0, f"{what}: the form without the {p} product stays within the bound ({v:.2f})"


def test_the_whole_tensor_figure_cannot_tell_them_apart():
    """Why the bound is per element: conftest's rel_err of the flushing form is the honest form's."""
    from conftest import rel_err
    x, w, ref, _, _ = _operands(3, 16, 64, (2, 24, 40), False)
    e_honest = max(rel_err(cr.emulate_conv(x, w, 3), ref.float()))
    e_flush = max(rel_err(cr.emulate_conv(x, w, 3, flush=True), ref.float()))
    print(f"whole-tensor rel err: honest {e_honest:.2e}, flushing {e_flush:.2e}")
    assert e_flush <= 1e-6 and e_honest <= 1e-6            # both pass test_conv2d_f16_vs_float64's bar
