"""GPU: the launch forms that the host picks from the shape and the pointers and that no other unit test reaches.

Every wm_* entry point chooses its kernel form on the host.  The shapes below are computed from those rules (files under
wave_mamba_amd/csrc/) so that the named form runs; each case is held to a float64 evaluation of the same operation at the bar of
that kernel's existing test (tests/test_gpu_parity.py), and to the project's bit-identical sibling path where there is one.

 1 wm_lfss_out_conv_fwd -> lfss_out_conv_acc_kernel<4>   lfss.hip:328-339: W % 64 == 0 and B H W >= 2^18; nstrips = W / 64,
     nbands = ceil(H / 4), bpw = clamp(ceil(B nbands nstrips / 4096), 1, 8), a walk = bpw consecutive bands of one strip
       (1, 4098, 64)   262272 >= 262144 positions; 1 strip (both halo columns in one wave); 1025 bands, the last of 4098 - 4096 = 2 rows
       (4, 259, 256)   265216 positions; 65 bands, the last of 259 - 256 = 3 rows; 4 images (batch stride); bpw = ceil(1040 / 4096) = 1
       (3, 1370, 512)  343 bands x 8 strips x 3 = 8232 -> bpw = ceil(8232 / 4096) = 3; 343 = 114 x 3 + 1: the last walk holds ONE band
       (8, 2052, 512)  513 bands x 8 strips x 8 = 32832 -> ceil(32832 / 4096) = 9, clamped to 8 (bit-identity with the pair only)
 2 wm_selscan_fwd with z (the gate inside the scan pass)   selscan.hip.h:151, 283-300; the plan is scan_fwd.hip:38-61:
     rows = batch G ceil(dim / G / 64), chunk = max(64, ceil(L / ceil(12288 / rows)) rounded up to 16), 16-byte form iff L % 4 == 0
       (2, 64, 192, 16, 1)  L % 4 == 0: 16-byte gate; chunk 64 -> 3 chunks
       (1, 64, 130, 16, 1)  L % 4 == 2: element-wise gate; 3 chunks, the last of 2 steps
       (1, 96, 256, 16, 1)  96 channels per group: 2 waves per group, the second of 32 channels; 4 chunks
       (1, 32, 128, 32, 2)  N = 32 -> NP = 32; 2 chunks
       (3, 8, 4, 4, 2)      L = 4: one tile (16 steps) shorter than a chunk, one chunk, no workspace
 3 wm_selscan_fwd / _bwd on misaligned operands   scan_fwd.hip:332, scan_bwd.hip:341: the 16-byte form needs L % 4 == 0 AND every
     plane pointer 16-byte aligned; (2, 64, 192, 16, 1) with u, delta, B, C, z, dy as contiguous views 4 bytes into a buffer
     -> element-wise form although L % 4 == 0, 3 chunks, with the last state
 4 wm_gate_fwd / _bwd, element-wise form   lfss.hip:546, 565 (gates.hip.h:54-60, 76-83): per_b % 4 != 0 or a pointer off 16 bytes
       (2, 5, 3, 3) per_b = 45;  (1, 3, 7, 9) per_b = 189;  glu_gate on (2, 10, 3, 3): per_b = 45, second half 180 bytes in;
       (2, 64, 5, 5) per_b = 1600 = 4 x 400: 16-byte form, grid.x = ceil(1600 / 1024) = 2, the second workgroup has 144 of 256 quads
 5 wm_dwconv3x3_fwd / _wgrad past gridDim.z   lfss.hip:54 (dwconv.hip.h:82, 205): grid.z = min(plane groups, 65535), then pg += gridDim.z
       (4097, 64, 2, 4)  W = 4 <= 64, W % 4 == 0: 16 lanes per row, 4 planes per wave -> 262208 / 4 = 65552 groups > 65535
       (1025, 64, 3, 3)  W % 4 != 0: element-wise, one plane per wave -> 65600 groups > 65535
 6 wm_skff_fwd, several workgroups per plane   hfe_wgrad.hip:224-236: bpp = min(ceil(floor(H W / 4) / 2048), ceil(4096 / (B C)))
       (1, 32, 96, 96)    9216 / 4 = 2304 -> bpp 2 (cap 128); H W % 4 == 0: 16-byte form
       (2, 16, 91, 91)    8281 % 4 == 1: element-wise; floor(8281 / 4) = 2070 -> bpp 2
       (1, 64, 192, 256)  49152 / 4 = 12288 -> bpp 6 (cap 64)
 7 wm_conv2d_fwd, more than three 32-channel row tiles   conv.hip, conv2d_walk: mtot = ceil(Cout / 32); 1x1: MT = 3 while >= 3 tiles are
     left, then 2 or 1; 3x3: MT = 2 while >= 2 are left, then 1 (with a residual the wave-specialised kernel goes one tile a launch)
       Cout 128: mtot 4 -> 1x1 3 + 1 (mbase 3), 3x3 2 + 2 (mbase 2);  Cout 160: mtot 5 -> 1x1 3 + 2, 3x3 2 + 2 + 1;
       Cout 136: mtot 5, the last tile holds 8 channels
     and the check every entry over Conv2dArgs ends with (conv_tail_check): B = 65536 > gridDim.y on a 2 x 2 map, real operands
 8 wm_layernorm2d_bwd, the 512-workgroup clamp   lfss.hip:411-415: min(512, ceil(B H W tpp / 256)), tpp = 2 for C >= 32 (pair kernel)
       (2, 32, 192, 192) 73728 x 2 / 256 = 576;  (2, 64, 160, 208) 66560 x 2 / 256 = 520;  (2, 16, 257, 257) ceil(132098 / 256) = 517
 9 wm_layernorm_tok_bwd / _fwd clamps   lfss.hip:416-420, 479-481: tokens per workgroup tpb = 256 / (C / 4); backward min(1024, ceil(T / tpb)),
     forward min(8192, ceil(T / tpb))
       C 32 (tpb 32): T = 33001 -> 1032;  C 64 (tpb 16): T = 16400 -> 1025;  C 8 (tpb 128): T = 131100 -> 1025;
       forward (262176, 32): 262176 / 32 = 8193 > 8192
10 wm_scale_add_bwd, a workgroup that walks its plane more than once   lfss.hip:589-594 (gates.hip.h:118): bpp = min(ceil(L / 1024),
     max(8, ceil(2048 / (B C))))
       (2, 32, 192, 192) ceil(36864 / 1024) = 36 > cap 32, L % 4 == 0;  (2, 32, 191, 193) L = 36863: 36 > 32, element-wise

Reduced gradients (sums of up to 2.6e5 products of both signs) are judged like every reduced gradient of this suite: against float64
at truth_bar(the error of PyTorch's fp32 result on the same inputs); both errors are printed.  The workgroup counts of rows 8 - 10 are
asserted through the *_det_workspace_bytes queries, so a retuned clamp fails here instead of moving a case back to the common form."""
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close, rel_err
from oracle import oracle
import wave_mamba_amd as wm
from wave_mamba_amd import _lib
from wave_mamba_amd.archs import wavemamba_arch as arch
from test_deterministic_gpu import _off16
from test_gpu_parity import GRAD_NAMES, TOL, cu, gen, random_scan_case, scan_grads_f64, truth_bar

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def assert_reduced(what, got, ref32, truth):
    """A reduced gradient: its error against float64 within truth_bar(the fp32 reference's own error); both are printed."""
    e_ref, e_got = max(rel_err(ref32, truth)), max(rel_err(got, truth))
    print(f"{what}: {e_got:.3e} vs float64 (fp32 reference: {e_ref:.3e})")
    assert e_got <= truth_bar(e_ref), f"{what}: {e_got:.3e} vs float64 (fp32 reference: {e_ref:.3e})"


# ------------------------------------------------------------------------------------------------
# 1. lfss_out_conv, the accumulating row-window form
# ------------------------------------------------------------------------------------------------
def _lfss_out_f64(f, w2, b2, tok1, w3, b3, sk, nchw):
    """Reference :226-230 in float64 (conv2 -> gelu(x1) * x2 -> conv3, then * skip + tok1), one image at a time."""
    B, D, H, W = f.shape
    C = D // 2
    outs = []
    for i in range(B):
        fc = F.conv2d(f[i:i + 1].double(), w2.double(), None if b2 is None else b2.double(), padding=1, groups=D)
        gv = F.gelu(fc[:, :C]) * fc[:, C:]
        outs.append((F.conv2d(gv, w3.double(), b3.double())
                     + (tok1[i:i + 1].double() * sk.double()).transpose(1, 2).reshape(1, C, H, W)).float())
    want = torch.cat(outs)
    return want if nchw else want.reshape(B, C, H * W).transpose(1, 2)


@pytest.mark.parametrize("B,H,W,bpw,last_rows,fp64", [(1, 4098, 64, 1, 2, True), (4, 259, 256, 1, 3, True), (3, 1370, 512, 3, 2, True),
                                                     (8, 2052, 512, 8, 4, False)])
@pytest.mark.parametrize("nchw", [False, True])
def test_lfss_out_conv_accumulating_form(B, H, W, bpw, last_rows, fp64, nchw):
    """test_lfss_out_with_depthwise_conv_folded_in's checks on lfss_out_conv_acc_kernel<4> where that test does not go: a last band
    of 2 and of 3 rows, a single strip, three bands per walk with a one-band last walk, and the clamp at eight bands per walk."""
    from wave_mamba_amd.ops import _ptr, _stream, check
    lib = _lib.load()
    C, D, L = 32, 64, H * W
    nbands, nstrips = (H + 3) // 4, W // 64
    assert W % 64 == 0 and B * L >= 1 << 18                                       # lfss.hip:328
    assert min(max((B * nbands * nstrips + 4095) // 4096, 1), 8) == bpw and H - 4 * (nbands - 1) == last_rows
    g = torch.Generator(device=DEV); g.manual_seed(B * 1000 + H * 10 + W)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    f, tok1 = rn(B, D, H, W), rn(B, L, C)
    w2, b2, w3, b3, sk = rn(D, 1, 3, 3) * 0.3, rn(D) * 0.2, rn(C, C, 1, 1) * 0.2, rn(C) * 0.2, rn(C) * 0.3 + 1
    shape = (B, C, H, W) if nchw else (B, L, C)
    # (NaN-filled: a position that either kernel leaves unwritten cannot compare equal)
    fused, unfused = torch.full(shape, float("nan"), device=DEV), torch.full(shape, float("nan"), device=DEV)
    check(lib.wm_lfss_out_conv_fwd(_ptr(f), _ptr(w2), _ptr(b2), _ptr(tok1), _ptr(w3), _ptr(b3), _ptr(sk), _ptr(fused),
                                   int(nchw), B, H, W, C, 0, _stream()), "wm_lfss_out_conv_fwd")
    fc = wm.ops.dwconv3x3(f, w2, b2, "none")
    check(lib.wm_lfss_out_fwd(_ptr(fc), _ptr(tok1), _ptr(w3), _ptr(b3), _ptr(sk), _ptr(unfused), int(nchw), B, L, C, 0,
                              _stream()), "wm_lfss_out_fwd")
    assert torch.equal(fused, unfused)
    if not fp64:                     # 8.4 M positions x 64 channels: bit-identity with the pair, which the smaller shapes hold to float64
        return
    del fc, unfused
    assert_close(fused, _lfss_out_f64(f, w2, b2, tok1, w3, b3, sk, nchw), 1e-5, "lfss_out with conv2 folded in vs fp64")
    fb16 = f.bfloat16()              # no bias, bf16 planes (fp32 arithmetic on the rounded input)
    fused.fill_(float("nan"))
    check(lib.wm_lfss_out_conv_fwd(_ptr(fb16), _ptr(w2), None, _ptr(tok1), _ptr(w3), _ptr(b3), _ptr(sk), _ptr(fused),
                                   int(nchw), B, H, W, C, 1, _stream()), "wm_lfss_out_conv_fwd bf16")
    assert_close(fused, _lfss_out_f64(fb16, w2, None, tok1, w3, b3, sk, nchw), 1e-5, "bf16 planes, no conv2 bias")


# ------------------------------------------------------------------------------------------------
# 2 and 3. selective scan: the gate inside the scan pass, and misaligned operands
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,dim,L,N,G,chunks", [(2, 64, 192, 16, 1, 3), (1, 64, 130, 16, 1, 3), (1, 96, 256, 16, 1, 4),
                                                    (1, 32, 128, 32, 2, 2), (3, 8, 4, 4, 2, 1)])
def test_scan_with_the_gate_fused_in(batch, dim, L, N, G, chunks):
    """selective_scan_fn(z=...) without autograd: wm_selscan_fwd gates y inside its scan pass, with 16-byte and element-wise
    accesses, over several chunks, at NP = 32 and with two waves per group."""
    rows = batch * G * ((dim // G + 63) // 64)
    want = (12288 + rows - 1) // rows                                             # scan_fwd.hip:54-59
    chunk = max(64, ((L + want - 1) // want + 15) // 16 * 16)
    assert (L + chunk - 1) // chunk == chunks
    assert (_lib.load().wm_selscan_fwd_workspace_bytes(batch, dim, L, N, G) > 0) == (chunks > 1)
    case = random_scan_case(batch, dim, L, N, G, seed=batch * 1000 + L)
    z = torch.randn(batch, dim, L, generator=gen(L + 1))
    with torch.no_grad():
        y, last = wm.ops.selective_scan_fn(*cu(*case[:6]), z.to(DEV), case[6].to(DEV), True, True)
    yr, lr = oracle.selscan_fwd_raw(*case[:6], z, case[6], True, True)
    assert_close(y, yr, TOL, "z-gated y")
    assert_close(last, lr, TOL, "last state")


def _scan_y_f64(u, delta, A, Bm, Cm, D, bias):
    """The ungated scan output in float64 (the recurrence of scan_grads_f64, forward only)."""
    u, delta, A, Bm, Cm, D, bias = (t.double() for t in (u, delta, A, Bm, Cm, D, bias))
    batch, dim, L = u.shape
    G = Bm.shape[1]
    dt = F.softplus(delta + bias.view(1, dim, 1))
    Bf, Cf = Bm.repeat_interleave(dim // G, dim=1), Cm.repeat_interleave(dim // G, dim=1)
    h = torch.zeros(batch, dim, A.shape[1], dtype=torch.float64)
    ys = []
    for t in range(L):
        h = torch.exp(dt[:, :, t, None] * A) * h + (dt[:, :, t] * u[:, :, t])[..., None] * Bf[..., t]
        ys.append((h * Cf[..., t]).sum(-1))
    return torch.stack(ys, 2) + u * D.view(1, dim, 1)


def test_scan_on_misaligned_operands():
    """u, delta, B, C, z and dy as contiguous views one float into a buffer: L % 4 == 0, yet wm_selscan_fwd and wm_selscan_bwd take
    their element-wise forms (three chunks).  Forward with the gate and the last state and the seven gradients under the rules of
    test_scan_backward_vs_oracle; y, the last state, du and ddelta are also bit-equal to the aligned call's (the two access forms
    run the same arithmetic per element).  The gradient through z is autograd on out * silu(z): one assertion against float64."""
    batch, dim, L, N, G = 2, 64, 192, 16, 1
    assert L % 4 == 0 and _lib.load().wm_selscan_fwd_workspace_bytes(batch, dim, L, N, G) > 0
    case = random_scan_case(batch, dim, L, N, G, seed=7 + L)
    z, dy = torch.randn(batch, dim, L, generator=gen(L + 1)), torch.randn(batch, dim, L, generator=gen(L))
    planes = (0, 1, 3, 4)                                                         # u, delta, B, C: the operands the kernels read in quads

    def operands(misaligned):
        return [_off16(t) if misaligned and i in planes else t.to(DEV) for i, t in enumerate(case)]
    ops_m, ops_a = operands(True), operands(False)
    with torch.no_grad():
        y_m, last_m = wm.ops.selective_scan_fn(*ops_m[:6], _off16(z), ops_m[6], True, True)
        y_a, last_a = wm.ops.selective_scan_fn(*ops_a[:6], z.to(DEV), ops_a[6], True, True)
    yr, lr = oracle.selscan_fwd_raw(*case[:6], z, case[6], True, True)
    assert_close(y_m, yr, TOL, "z-gated y, misaligned")
    assert_close(last_m, lr, TOL, "last state, misaligned")
    assert torch.equal(y_m, y_a) and torch.equal(last_m, last_a)

    def grads(leaves, dyd):
        leaves = [t.requires_grad_(True) for t in leaves]
        y = wm.ops.selective_scan_fn(*leaves[:6], None, leaves[6], True)
        return torch.autograd.grad(y, leaves, dyd)
    g_m, g_a = grads(ops_m, _off16(dy)), grads(ops_a, dy.to(DEV))
    want = oracle.selscan_bwd_raw(*case, dy, True)
    truth = scan_grads_f64(*case, dy)
    for name, got, ref in zip(GRAD_NAMES, g_m, want):
        if name in ("dA", "dD", "dbias"):
            assert_reduced(f"scan {name}, misaligned", got, ref, truth[name])
        else:
            assert_close(got, ref, TOL, f"{name}, misaligned")
    assert torch.equal(g_m[0], g_a[0]) and torch.equal(g_m[1], g_a[1])

    zl = _off16(z).requires_grad_(True)
    (dz,) = torch.autograd.grad(wm.ops.selective_scan_fn(*[t.detach() for t in ops_m[:6]], zl, ops_m[6].detach(), True), (zl,), _off16(dy))
    z64 = z.double().requires_grad_(True)
    (dz64,) = torch.autograd.grad(_scan_y_f64(*case) * F.silu(z64), (z64,), dy.double())
    assert_close(dz, dz64.float(), TOL, "dz")


# ------------------------------------------------------------------------------------------------
# 4. gates, element-wise form
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 5, 3, 3), (1, 3, 7, 9), (2, 64, 5, 5)])
@pytest.mark.parametrize("act", ["silu", "gelu", "sigmoid"])
def test_gate_elementwise_form_and_ragged_last_quads(shape, act):
    """test_gate_and_glu_gate_vs_fp64_autograd where per_b = C H W is no multiple of 4 (45, 189: gate_act, glu_gate on (B, 2C, H, W)
    and gate_act on its chunk(2, 1) views - the second starts 4 per_b bytes in - all element-wise), and at per_b = 1600: 16-byte
    accesses, two workgroups per image, the second partly filled."""
    B, C, H, W = shape
    per_b = C * H * W
    assert per_b % 4 != 0 or (per_b % 1024 != 0 and per_b > 1024)
    gg = gen(C * H + W)
    a, b, g = (torch.randn(B, C, H, W, generator=gg) * 2 for _ in range(3))
    f = {"silu": F.silu, "gelu": F.gelu, "sigmoid": torch.sigmoid}[act]
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = f(a64) * b64
    ra, rb = torch.autograd.grad(ref, (a64, b64), g.double())
    ad, bd = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    out = wm.ops.gate_act(ad, bd, act)
    ga, gb = torch.autograd.grad(out, (ad, bd), g.to(DEV))
    assert_close(out.detach(), ref.detach().float(), 2e-6, f"{act} gate")
    assert_close(ga, ra.float(), 2e-6, f"{act} gate d/da"); assert_close(gb, rb.float(), 2e-6, f"{act} gate d/db")
    t = torch.cat([a, b], 1).to(DEV).requires_grad_(True)
    out2 = wm.ops.glu_gate(t, act)
    (gt,) = torch.autograd.grad(out2, t, g.to(DEV))
    assert torch.equal(out2, out) and torch.equal(gt[:, :C], ga) and torch.equal(gt[:, C:], gb)
    v1, v2 = (v.requires_grad_(True) for v in t.detach().chunk(2, dim=1))
    assert (v2.data_ptr() - v1.data_ptr()) == 4 * per_b and v1.stride(0) == 2 * per_b
    out3 = wm.ops.gate_act(v1, v2, act)
    g1, g2 = torch.autograd.grad(out3, (v1, v2), g.to(DEV))
    assert torch.equal(out3, out) and torch.equal(g1, ga) and torch.equal(g2, gb)


# ------------------------------------------------------------------------------------------------
# 5. depth-wise 3x3 past 65535 plane groups
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,ppw", [((4097, 64, 2, 4), 4), ((1025, 64, 3, 3), 1)])
def test_dwconv3x3_more_plane_groups_than_grid_z(shape, ppw):
    """More groups of planes than gridDim.z holds: the kernels' `pg += gridDim.z` loops, four planes per wave (16-byte form) and one
    (element-wise).  Forward ("none" / "silu", with and without bias) and dx at the bars of test_dwconv3x3_vs_torch /
    test_dwconv3x3_gradients_vs_torch_autograd; dW and db sum over B = 4097 / 1025 images: truth_bar of PyTorch's fp32 error."""
    B, C, H, W = shape
    assert (W % 4 == 0 and W <= 64) == (ppw == 4) and (B * C + ppw - 1) // ppw > 65535        # lfss.hip:49-54
    gg = gen(B * 1000 + W)
    x, w, b, gy = (torch.randn(*shape, generator=gg), torch.randn(C, 1, 3, 3, generator=gg) * 0.3, torch.randn(C, generator=gg),
                   torch.randn(*shape, generator=gg))
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    ref = F.conv2d(xr, wr, br, padding=1, groups=C)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    for act in ("none", "silu"):
        for with_bias in (True, False):
            r = ref.detach() if with_bias else F.conv2d(x.double(), w.double(), None, padding=1, groups=C)
            got = wm.ops.dwconv3x3(xd, wd, bd if with_bias else None, act)
            assert_close(got, (F.silu(r) if act == "silu" else r).float(), 1e-5, f"dwconv {shape} {act} bias={with_bias}")
    truth = torch.autograd.grad(ref, (xr, wr, br), gy.double())
    x32, w32, b32 = (t.clone().requires_grad_(True) for t in (x, w, b))
    ref32 = torch.autograd.grad(F.conv2d(x32, w32, b32, padding=1, groups=C), (x32, w32, b32), gy)
    xg, wg, bg = (t.requires_grad_(True) for t in (xd, wd, bd))
    out = wm.ops.dwconv3x3_train(xg, wg, bg)
    assert_close(out.detach(), ref.detach().float(), 1e-5, f"dwconv3x3_train {shape}")
    got = torch.autograd.grad(out, (xg, wg, bg), gy.to(DEV))
    assert_close(got[0], truth[0].float(), 2e-5, f"dwconv dx {shape}")
    assert_reduced(f"dwconv dW {shape}", got[1], ref32[1], truth[1])
    assert_reduced(f"dwconv db {shape}", got[2], ref32[2], truth[2])


# ------------------------------------------------------------------------------------------------
# 6. SKFF with several workgroups per plane
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,H,W,bpp", [(1, 32, 96, 96, 2), (2, 16, 91, 91, 2), (1, 64, 192, 256, 6)])
def test_skff_several_workgroups_per_plane(B, C, H, W, bpp):
    """test_skff_vs_module_path with H W > 8192: chansum3's per-workgroup partials and skff_apply at bpp > 1, with 16-byte accesses
    and (91 x 91) without.  (1, 64, 128, 192) would give ceil(6144 / 2048) = 3 workgroups; six need 10240 < H W / 4 <= 12288.)"""
    assert min((H * W // 4 + 2047) // 2048, (4096 + B * C - 1) // (B * C)) == bpp                 # hfe_wgrad.hip:225-227
    torch.manual_seed(11)
    m = arch.SKFF(C, height=3, reduction=8).eval()
    with torch.no_grad():
        m.conv_du[1].weight.fill_(0.2)
    # Plane means of O(1) that differ from plane to plane, on a vertical ramp: the band weights then depend on every workgroup's
    # partial sum, and the partials of one plane differ (zero-mean noise alone gives weights of 1/3 whatever the sums are).
    ramp = torch.linspace(-1.0, 1.0, H).view(1, 1, H, 1)
    feats = [torch.randn(B, C, H, W, generator=gen(i + 3)) + torch.randn(B, C, 1, 1, generator=gen(i + 13)) * 2
             + ramp * torch.randn(B, C, 1, 1, generator=gen(i + 23)) * 3 for i in range(3)]
    with torch.no_grad():
        ref = m.double()([f.double() for f in feats]).float()      # CPU: no ops backend kernel applies -> PyTorch path
        got = m.float().to(DEV)([f.to(DEV) for f in feats])
    assert_close(got, ref, 1e-5, "SKFF")


# ------------------------------------------------------------------------------------------------
# 7. dense convolutions past 96 output channels
# ------------------------------------------------------------------------------------------------
@pytest.fixture(params=["first_gen", "wave_specialised"])
def conv3x3_impl(request):
    """Run the test once per 3x3 kernel (test_gpu_parity.py's fixture of the same name)."""
    wm.ops.conv2d_select(wm.ops.CONV3X3_FIRST_GEN if request.param == "first_gen" else wm.ops.CONV3X3_WAVE_SPECIALISED)
    yield request.param
    wm.ops.conv2d_select(wm.ops.CONV3X3_AUTO)


@pytest.mark.parametrize("ks", [3, 1])
@pytest.mark.parametrize("B,Ca,Cb,Cout,H,W,bias,res", [(1, 32, 0, 128, 17, 33, True, False), (1, 64, 0, 160, 9, 40, False, False),
                                                      (2, 32, 32, 136, 8, 16, True, False), (2, 32, 32, 136, 8, 16, True, True)])
def test_conv2d_more_than_three_row_tiles(conv3x3_impl, ks, B, Ca, Cb, Cout, H, W, bias, res):
    """test_conv2d_vs_torch past 96 output channels: a second launch at mbase = 3 (1x1) / mbase = 2 (3x3, both kernels), a last row
    tile of 8 channels, and the epilogue's residual read at mbase > 0."""
    assert (Cout + 31) // 32 > 3                                                  # conv.hip, conv2d_walk
    gg = gen(Ca * 100 + Cout + H + ks)
    xa = torch.randn(B, Ca, H, W, generator=gg)
    xb = torch.randn(B, Cb, H, W, generator=gg) if Cb else None
    w = torch.randn(Cout, Ca + Cb, ks, ks, generator=gg) / (ks * (Ca + Cb) ** 0.5)
    b = torch.randn(Cout, generator=gg) if bias else None
    r = torch.randn(B, Cout, H, W, generator=gg) if res else None
    xin = xa if xb is None else torch.cat([xa, xb], 1)
    ref = F.conv2d(xin.double(), w.double(), None if b is None else b.double(), padding=ks // 2)
    if res:
        ref = ref + r.double()
    got = wm.ops.conv2d(*cu(xa, w, b, xb), residual=None if r is None else r.to(DEV))
    assert_close(got, ref.float(), 2e-5, f"conv2d ks={ks} {(B, Ca, Cb, Cout, H, W)} residual={res}")


def test_conv2d_entries_refuse_a_batch_past_grid_y():
    """Every entry over Conv2dArgs ends its checks with the same pair (conv.hip, conv_tail_check): B = 65536 on a 2 x 2 map is
    WM_EUNSUPPORTED from each of them.  Every operand is a real tensor of the size the call describes, so an entry that lost the
    check would compute or be refused by the runtime - it could not fault."""
    B, C = 65536, 32
    z = lambda *shape: torch.zeros(shape, device=DEV)
    frag = lambda ks: torch.zeros(_lib.load().wm_conv2d_wfrag_bytes(C, C, ks), dtype=torch.uint8, device=DEV)
    x, y, vec = z(B, C, 2, 2), z(B, C, 2, 2), z(C)
    go = lambda name, *args: wm.ops._launch(x.device, name, *args, status=True)
    for ks in (1, 3):
        assert go("wm_conv2d_fwd", x, None, None, frag(ks), vec, None, None, y, B, C, 0, 0, C, 2, 2, ks) == _lib.WM_EUNSUPPORTED, ks
        assert go("wm_conv2d_f16_steps", x, z(C, C, ks, ks), vec, y, z(2), frag(ks), B, C, C, 2, 2, ks, 0) == _lib.WM_EUNSUPPORTED, ks
    assert go("wm_conv2d_ln_fwd", x, vec, vec, 1e-6, frag(1), vec, None, y, B, C, C, 2, 2) == _lib.WM_EUNSUPPORTED
    assert go("wm_conv2d_gated_fwd", x, None, None, frag(3), frag(1), vec, y, B, C, 0, 0, C, 2, 2) == _lib.WM_EUNSUPPORTED
    bands = [z(B, C, 1, 1) for _ in range(4)]
    assert go("wm_conv2d_dwt_fwd", x, frag(3), vec, *bands, B, C, C, 2, 2, _lib.WM_F32) == _lib.WM_EUNSUPPORTED
    assert go("wm_idwt_conv2d_fwd", bands[0], z(B, 3 * C, 1, 1), frag(3), vec, None, y, B, C, C, 2, 2, _lib.WM_F32) == _lib.WM_EUNSUPPORTED
    torch.cuda.synchronize()                  # (wm_conv2d_f16_steps takes the operands' magnitudes before it reaches the check)


# ------------------------------------------------------------------------------------------------
# 8 to 10. reduction clamps
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,unclamped", [((2, 32, 192, 192), 576), ((2, 64, 160, 208), 520), ((2, 16, 257, 257), 517)])
def test_layernorm2d_backward_grid_stride(shape, unclamped):
    """layernorm2d_train where ceil(B H W tpp / 256) exceeds the 512 workgroups of the backward launch: its grid-stride loop, pair
    kernel (C = 32, 64) and single kernel (C = 16).  Forward and gx at the bars of test_layernorm2d_vs_torch /
    test_layernorm2d_gradients_vs_torch_autograd; dweight and dbias sum over up to 132098 positions: truth_bar of PyTorch's fp32 error."""
    B, C, H, W = shape
    assert (B * H * W * (2 if C >= 32 else 1) + 255) // 256 == unclamped > 512    # lfss.hip:411-415
    assert _lib.load().wm_layernorm2d_bwd_det_workspace_bytes(B, H * W, C) == 512 * 2 * C * 4
    x, w, b, gy = (torch.randn(*shape, generator=gen(1)) * 2 + 0.5, torch.randn(C, generator=gen(2)), torch.randn(C, generator=gen(3)),
                   torch.randn(*shape, generator=gen(4)))

    def ref(x_, w_, b_):
        mu = x_.mean(1, keepdim=True)
        var = (x_ - mu).pow(2).mean(1, keepdim=True)
        return w_.view(1, -1, 1, 1) * ((x_ - mu) / (var + 1e-6).sqrt()) + b_.view(1, -1, 1, 1)
    l64 = [t.double().requires_grad_(True) for t in (x, w, b)]
    y64 = ref(*l64)
    truth = torch.autograd.grad(y64, l64, gy.double())
    l32 = [t.clone().requires_grad_(True) for t in (x, w, b)]
    ref32 = torch.autograd.grad(ref(*l32), l32, gy)
    ld = [t.to(DEV).requires_grad_(True) for t in (x, w, b)]
    y = wm.ops.layernorm2d_train(*ld, 1e-6)
    got = torch.autograd.grad(y, ld, gy.to(DEV))
    assert_close(y.detach(), y64.detach().float(), 1e-5, f"LayerNorm2d {shape}")
    assert_close(got[0], truth[0].float(), 5e-5, f"LayerNorm2d gx {shape}")
    assert_reduced(f"LayerNorm2d dweight {shape}", got[1], ref32[1], truth[1])
    assert_reduced(f"LayerNorm2d dbias {shape}", got[2], ref32[2], truth[2])


@pytest.mark.parametrize("T,C,unclamped", [(33001, 32, 1032), (16400, 64, 1025), (131100, 8, 1025)])
def test_layernorm_tok_backward_grid_stride(T, C, unclamped):
    """layernorm_tok where ceil(T / tpb) exceeds the 1024 workgroups of the backward launch.  Forward and gx at the bars of
    test_layernorm_tok_forward_backward_vs_torch; dweight and dbias by truth_bar of PyTorch's fp32 error."""
    assert (T + 256 // (C // 4) - 1) // (256 // (C // 4)) == unclamped > 1024     # lfss.hip:416-420
    assert _lib.load().wm_layernorm_tok_bwd_det_workspace_bytes(T, C) == 1024 * 2 * C * 4
    gg = gen(C + 2)
    x, w, b, gy = (torch.randn(T, C, generator=gg) * 2.0 + 0.5, torch.randn(C, generator=gg) * 0.5 + 1.0, torch.randn(C, generator=gg),
                   torch.randn(T, C, generator=gg))
    l64 = [t.double().requires_grad_(True) for t in (x, w, b)]
    y64 = F.layer_norm(l64[0], (C,), l64[1], l64[2], 1e-5)
    truth = torch.autograd.grad(y64, l64, gy.double())
    l32 = [t.clone().requires_grad_(True) for t in (x, w, b)]
    ref32 = torch.autograd.grad(F.layer_norm(l32[0], (C,), l32[1], l32[2], 1e-5), l32, gy)
    ld = [t.to(DEV).requires_grad_(True) for t in (x, w, b)]
    y = wm.ops.layernorm_tok(*ld, 1e-5)
    got = torch.autograd.grad(y, ld, gy.to(DEV))
    assert_close(y.detach(), y64.detach().float(), 1e-5, f"layernorm_tok {(T, C)}")
    assert_close(got[0], truth[0].float(), 2e-5, f"layernorm_tok gx {(T, C)}")
    assert_reduced(f"layernorm_tok dweight {(T, C)}", got[1], ref32[1], truth[1])
    assert_reduced(f"layernorm_tok dbias {(T, C)}", got[2], ref32[2], truth[2])


def test_layernorm_tok_forward_grid_stride():
    """The forward launch's clamp at 8192 workgroups: (262176, 32) is 8193 workgroups of 32 tokens, so the last 32 tokens are reached
    by the grid-stride loop only (checked on their own as well: they are 1e-4 of the tensor)."""
    T, C = 262145 + 31, 32
    assert (T + 31) // 32 == 8193 > 256 * 32                                      # lfss.hip:479-481
    gg = gen(C + 2)
    x, w, b = torch.randn(T, C, generator=gg) * 2.0 + 0.5, torch.randn(C, generator=gg) * 0.5 + 1.0, torch.randn(C, generator=gg)
    with torch.no_grad():
        got = wm.ops.layernorm_tok(*cu(x, w, b), 1e-5)
    assert_close(got, F.layer_norm(x.double(), (C,), w.double(), b.double(), 1e-5).float(), 1e-5, f"layernorm_tok {(T, C)}")
    assert_close(got[8192 * 32:], F.layer_norm(x[8192 * 32:].double(), (C,), w.double(), b.double(), 1e-5).float(), 1e-5, "the strided tail")


@pytest.mark.parametrize("shape", [(2, 32, 192, 192), (2, 32, 191, 193)])
def test_scale_add_backward_walks_its_plane_more_than_once(shape):
    """scale_add where ceil(H W / 1024) = 36 exceeds the 32 workgroups a plane gets: workgroups 0 .. 3 walk their plane twice, with
    16-byte accesses (192 x 192) and element-wise (191 x 193, a ragged last quad).  Forward, gx and go at test_scale_add_vs_fp64_autograd's
    1e-6; d/dscale sums 73728 products: truth_bar of PyTorch's fp32 error."""
    B, C, H, W = shape
    L = H * W
    cap = max(8, (2048 + B * C - 1) // (B * C))                                   # lfss.hip:589-594
    assert (L + 1023) // 1024 == 36 > cap == 32
    assert _lib.load().wm_scale_add_bwd_det_workspace_bytes(B, C, L) == B * 32 * C * 4
    gg = gen(B * 100 + W)
    x, o, g = (torch.randn(B, C, H, W, generator=gg) for _ in range(3))
    s = torch.randn(C, generator=gg) * 0.3 + 1
    l64 = [t.double().requires_grad_(True) for t in (x, s, o)]
    ref = l64[0] * l64[1].view(1, -1, 1, 1) + l64[2]
    rx, rs, ro = torch.autograd.grad(ref, l64, g.double())
    l32 = [t.clone().requires_grad_(True) for t in (x, s, o)]
    _, rs32, _ = torch.autograd.grad(l32[0] * l32[1].view(1, -1, 1, 1) + l32[2], l32, g)
    xd, sd, od = (t.to(DEV).requires_grad_(True) for t in (x, s, o))
    out = wm.ops.scale_add(xd, sd, od)
    gx, gs, go = torch.autograd.grad(out, (xd, sd, od), g.to(DEV))
    assert_close(out.detach(), ref.detach().float(), 1e-6, "scale_add")
    assert_close(gx, rx.float(), 1e-6, "scale_add d/dx"); assert_close(go, ro.float(), 1e-6, "scale_add d/do")
    assert_reduced(f"scale_add d/dscale {shape}", gs, rs32, rs)
