"""Host-side mirror of the reference's operator surface for the Wave-Mamba hot path.

Same names, argument meaning and error behaviour as the reference
(/root/reference/basicsr/archs/wavemamba_arch.py):

    dwt_init(x) -> (x_LL, x_HL, x_LH, x_HH)                                   :97-110
    iwt_init(x) -> h                                                          :113-130
    selective_scan_fn(u, delta, A, B, C, D=None, z=None, delta_bias=None,
                      delta_softplus=False, return_last_state=False)          :6, :465-471

Every op is a torch.autograd.Function over the C ABI of libwavemamba_hip.so (hand-written HIP for
gfx950).  PyTorch only supplies device memory, the current stream and autograd plumbing.  There is
NO CPU / eager fallback: a non-CUDA tensor or a missing library raises.
"""
import ctypes
import os
import weakref

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import WM_BF16, WM_F32, check


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _require_cuda(name, *tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                f"{name}: expected a CUDA (ROCm) tensor, got device '{t.device}'. The Wave-Mamba hot "
                "path is HIP-only (dwt_init / iwt_init / selective_scan_fn alone have a CPU twin, for inputs that are ALL "
                "on the CPU); nothing falls back to the CPU.")


def _dtype_code(t, name):
    if t.dtype == torch.float32:
        return WM_F32
    if t.dtype == torch.bfloat16:
        return WM_BF16
    raise RuntimeError(f"{name}: unsupported dtype {t.dtype} (float32 and bfloat16 are implemented)")


def _ptr(t):                # (for tests and tools that call the library directly; the operators below go through _launch)
    return None if t is None else t.data_ptr()


def _launch(dev, name, *args, status=False):
    """The one way a kernel-launching entry point of the library is called: on device `dev`, on that device's current stream
    (every launching entry point takes `void* stream` last), tensors passed as their data pointers (None and raw integer
    addresses - sub-band and GLU-half offsets - go through as they are), a non-zero status raised under the entry point's
    own name.  status=True: the status is returned instead, for a caller that tells a refusal from an error."""
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = _stream()
        rc = getattr(lib, name)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], stream)
    if status:
        return rc
    check(rc, name)


# ------------------------------------------------------------------------------------------------
# Zeroed accumulator outputs (training): parameter gradients the kernels add into with atomics and the running maxima of the
# fp16-split convolutions are a few hundred bytes each, and the library's memset node in front of each of them was 4.2 us of
# stream time, 323 times per BASELINE config-3 step.  They are handed out of a 4-MB block zeroed ONCE (per device and stream,
# bump allocation, no slice is ever handed out twice); the block is registered with the library (wm_zero_arena_register), which
# then skips its memset for buffers inside it.  A block lives as long as any slice of it does (the slices are views of its
# storage); it is unregistered when the next block replaces it.
# ------------------------------------------------------------------------------------------------
# ONE-SHOT RULE: a slice is zero exactly once - when it is handed out.  Whoever receives it (a library call that accumulates into
# it, then autograd, which may keep it as a parameter's .grad) must never pass it to an accumulate-into entry point again: the
# library would take it for zero (it lies in a registered range) and add onto the old contents.  Nothing in this package does;
# a caller that keeps such tensors and wants to be safe calls zero_arena_clear() (new slices then come from a fresh block, and
# the old block, once its last slice is gone, is unregistered and freed).
_ZERO_ARENA_FLOATS = 1 << 20
_ZERO_ARENAS = {}            # (device index, stream handle) -> [block, floats handed out]
_ZERO_ARENA_LOCK = __import__("threading").Lock()


def _zeros_small(n, device):
    """A zeroed float32 vector of n elements on `device` for an accumulate-into output of the library, valid on the current
    stream.  Larger than 64 KB, or under graph capture: uninitialised memory (the library zeroes it itself)."""
    if n > 16384 or torch.cuda.is_current_stream_capturing():
        return torch.empty(n, dtype=torch.float32, device=device)
    lib = _lib.load()
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(device).cuda_stream)
    step = (n + 63) & ~63                                  # 256-byte slots
    with _ZERO_ARENA_LOCK:
        ent = _ZERO_ARENAS.get(key)
        if ent is None or ent[1] + step > _ZERO_ARENA_FLOATS:
            block = torch.zeros(_ZERO_ARENA_FLOATS, dtype=torch.float32, device=device)
            if ent is not None:
                ent[2]()                                   # the exhausted block: unregistered now, freed with its last slice
            check(lib.wm_zero_arena_register(block.data_ptr(), 4 * _ZERO_ARENA_FLOATS), "wm_zero_arena_register")
            ent = _ZERO_ARENAS[key] = [block, 0, weakref.finalize(block, lib.wm_zero_arena_unregister, block.data_ptr())]
        out = ent[0][ent[1]:ent[1] + n]
        ent[1] += step
    return out


def zero_arena_clear():
    """Drop every zeroed arena block (all devices, all streams): each is unregistered from the library now and freed with its last
    slice.  For long-running processes that create and destroy streams (an entry per (device, stream) would otherwise keep a 4-MB
    block registered for ever - ADVICE r5), and for callers that re-use gradient tensors handed out of an arena (see the one-shot
    rule above).  Must not run concurrently with training steps on other threads (their next small output simply opens a new block)."""
    with _ZERO_ARENA_LOCK:
        for ent in _ZERO_ARENAS.values():
            ent[2]()                                       # weakref.finalize: unregister (idempotent)
        _ZERO_ARENAS.clear()


# ------------------------------------------------------------------------------------------------
# Deterministic training mode: every gradient and the loss value bit-equal run to run.  Off by default.  With it on, the autograd
# functions whose kernels leave a sum through float atomics - the depth-wise weight gradient, the three LayerNorm backward kernels,
# the linear weight gradient, plane_sums, the scale_add backward, the L1 mean and the selective-scan backward - call the library's
# wm_*_det forms (same kernels, same grid, per-workgroup partials in a torch.empty workspace, a fixed-order finish that overwrites
# torch.empty outputs: no zero arena), and the two channel gathers of the HFE branch go through channel_gather, whose backward is
# the library's ordered kernel instead of ATen's scatter-add.  The mode is read when an operator is CALLED: a graph captured with
# it on replays the deterministic kernels whatever the mode is at replay.  WM_DETERMINISTIC=1 in the environment sets the
# initial value (read at import, like WM_TRAIN_CONV).
# The dense convolutions' weight gradient (_conv_weight_grad) goes to wm_conv2d_wgrad at every map width in the mode (zero-padded on
# the right to a multiple of 32 columns).  What stays on ATen's unordered weight gradient even then: output channels whose count,
# rounded up to 16s, is not 1, 2, 4 or 6 - 33 .. 48, 65 .. 80 and more than 96 output channels, 3x3 and 1x1 alike - for which the
# kernel has no form at any width (conv2d_wgrad_supported, whose `ks == 3 and 64 < Cout <= 80` clause that rule contains).  The
# shipped configuration (wf = 32) has no such convolution; a network of wf = 48 has them throughout.
# ------------------------------------------------------------------------------------------------
_DETERMINISTIC = os.environ.get("WM_DETERMINISTIC", "0")
if _DETERMINISTIC not in ("0", "1"):
    raise RuntimeError(f"WM_DETERMINISTIC={_DETERMINISTIC!r}: 0 or 1")
_DETERMINISTIC = _DETERMINISTIC == "1"


def set_deterministic(on):
    """Switch the deterministic training mode (see above).  Returns the previous setting."""
    global _DETERMINISTIC
    prev, _DETERMINISTIC = _DETERMINISTIC, bool(on)
    return prev


def is_deterministic():
    return _DETERMINISTIC


def _det_workspace(nbytes, device):
    """The uninitialised workspace of a wm_*_det call (None for 0 bytes: an empty problem)."""
    return torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None


# ------------------------------------------------------------------------------------------------
# bf16-storage mode (BASELINE config 2 as worded): the plane tensors an LFSSBlock hands from kernel to kernel - x, z,
# the conv outputs, the four scan outputs, f, fc - are stored as bfloat16; every kernel computes in fp32 (tiles,
# projections, scan state, LayerNorm statistics) and the token tensors between blocks stay fp32.  Off by default:
# the parity bars of the fp32 path (1e-4 per tensor) cannot hold at 8 mantissa bits; bench.py --bf16 and
# tests/test_gpu_parity.py report the PSNR against the fp32 output.
# ------------------------------------------------------------------------------------------------
_PLANE_DTYPE = torch.float32


def set_plane_dtype(dtype):
    """torch.float32 (default) or torch.bfloat16: storage of the LFSSBlock-internal plane tensors on the fused inference
    path (shipped width C = 32 only).  Returns the previous setting."""
    global _PLANE_DTYPE
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("plane dtype must be torch.float32 or torch.bfloat16")
    prev, _PLANE_DTYPE = _PLANE_DTYPE, dtype
    return prev


def get_plane_dtype():
    return _PLANE_DTYPE


# ------------------------------------------------------------------------------------------------
# Haar DWT / IWT
# ------------------------------------------------------------------------------------------------
class _DWT(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _require_cuda("dwt_init", x)
        if x.dim() != 4:
            raise RuntimeError(f"dwt_init: expected a 4-D NCHW tensor, got {tuple(x.shape)}")
        B, C, H, W = x.shape
        if H % 2 or W % 2:
            # the reference's strided slices disagree in size for odd H/W -> RuntimeError
            raise RuntimeError(f"dwt_init: H and W must be even, got {H}x{W}")
        code = _dtype_code(x, "dwt_init")
        x = x.contiguous()
        outs = [torch.empty((B, C, H // 2, W // 2), dtype=x.dtype, device=x.device) for _ in range(4)]
        _launch(x.device, "wm_dwt2d_fwd", x, *outs, B, C, H, W, code)
        ctx.shape = (B, C, H, W)
        return tuple(outs)

    @staticmethod
    def backward(ctx, g_ll, g_hl, g_lh, g_hh):
        B, C, H, W = ctx.shape
        gs = [g.contiguous() for g in (g_ll, g_hl, g_lh, g_hh)]
        code = _dtype_code(gs[0], "dwt_init.backward")
        dx = torch.empty((B, C, H, W), dtype=gs[0].dtype, device=gs[0].device)
        _launch(dx.device, "wm_dwt2d_bwd", *gs, dx, B, C, H, W, code)
        return dx


class _IWT(torch.autograd.Function):
    """Synthesis from four sub-band blocks given as (tensor, channel offset) views of 1 or 2 tensors."""

    @staticmethod
    def forward(ctx, x_l, x_h):
        # x_h is None: x_l is the reference's concatenated (B, 4C, h, w) tensor.
        # else: x_l (B, C, h, w) and x_h (B, 3C, h, w) - upFRG's un-concatenated pair (:1006).
        _require_cuda("iwt_init", x_l, x_h)
        x_l = x_l.contiguous()
        if x_h is None:
            B, C4, h, w = x_l.shape
            if C4 % 4:
                raise RuntimeError(f"iwt_init: channel count {C4} is not a multiple of 4")
            C = C4 // 4
            hw = h * w
            es = x_l.element_size()
            ptrs = [x_l.data_ptr() + k * C * hw * es for k in range(4)]
            strides = [4 * C * hw] * 4
            code = _dtype_code(x_l, "iwt_init")
        else:
            x_h = x_h.contiguous()
            if x_h.dtype != x_l.dtype:           # mixed precision (autocast): the output is fp32 anyway
                x_l, x_h = x_l.float(), x_h.float()
            B, C, h, w = x_l.shape
            if x_h.shape != (B, 3 * C, h, w):
                raise RuntimeError(f"iwt_init: x_h shape {tuple(x_h.shape)} != {(B, 3 * C, h, w)}")
            hw = h * w
            es = x_h.element_size()
            ptrs = [x_l.data_ptr()] + [x_h.data_ptr() + k * C * hw * es for k in range(3)]
            strides = [C * hw] + [3 * C * hw] * 3
            code = _dtype_code(x_l, "iwt_init")
        out = torch.empty((B, C, 2 * h, 2 * w), dtype=torch.float32, device=x_l.device)  # always fp32
        _launch(out.device, "wm_idwt2d_fwd", *ptrs, *strides, out, B, C, h, w, code)
        ctx.geom = (B, C, h, w, x_h is None, x_l.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        B, C, h, w, cat, dt = ctx.geom
        g = g.contiguous().float()
        hw = h * w
        code = WM_F32 if dt == torch.float32 else WM_BF16
        if cat:
            d_l = torch.empty((B, 4 * C, h, w), dtype=dt, device=g.device)
            d_h = None
            es = d_l.element_size()
            ptrs = [d_l.data_ptr() + k * C * hw * es for k in range(4)]
            strides = [4 * C * hw] * 4
        else:
            d_l = torch.empty((B, C, h, w), dtype=dt, device=g.device)
            d_h = torch.empty((B, 3 * C, h, w), dtype=dt, device=g.device)
            es = d_l.element_size()
            ptrs = [d_l.data_ptr()] + [d_h.data_ptr() + k * C * hw * es for k in range(3)]
            strides = [C * hw] + [3 * C * hw] * 3
        _launch(g.device, "wm_idwt2d_bwd", g, *ptrs, *strides, B, C, h, w, code)
        return d_l, d_h


# The three operators of the drop-in boundary have a CPU twin (cpu_twin.py: plain PyTorch, SURVEY.md 8b "each with CPU + HIP
# implementations", BASELINE config 1 "CPU-only PyTorch forward").  The dispatch key is the DEVICE OF THE INPUT, as for any torch
# operator - never the presence of the library: a CUDA tensor goes to the HIP kernels below and raises if they cannot be loaded.
def _on_cpu(*tensors):
    ts = [t for t in tensors if t is not None]
    return bool(ts) and all(t.device.type == "cpu" for t in ts)


def dwt_init(x):
    """Haar analysis of an NCHW map -> (x_LL, x_HL, x_LH, x_HH), each (B, C, H/2, W/2), dtype of x."""
    if _on_cpu(x):
        from . import cpu_twin
        return cpu_twin.dwt_init(x)
    return _DWT.apply(x)


def iwt_init(x):
    """Haar synthesis of a (B, 4C, h, w) tensor [x1|x2|x3|x4] -> (B, C, 2h, 2w), always float32."""
    if _on_cpu(x):
        from . import cpu_twin
        return cpu_twin.iwt_init(x)
    return _IWT.apply(x, None)


def iwt_init_pair(x_l, x_h):
    """iwt_init(torch.cat([x_l, x_h], dim=1)) without materialising the concatenation."""
    if _on_cpu(x_l, x_h):
        from . import cpu_twin
        return cpu_twin.iwt_init_pair(x_l, x_h)
    return _IWT.apply(x_l, x_h)


# ------------------------------------------------------------------------------------------------
# selective scan
# ------------------------------------------------------------------------------------------------
def _scan_shapes(u, delta, A, B, C, D, z, delta_bias):
    if u.dim() != 3:
        raise RuntimeError(f"selective_scan_fn: u must be (batch, dim, L), got {tuple(u.shape)}")
    batch, dim, L = u.shape
    if delta.shape != u.shape:
        raise RuntimeError(f"selective_scan_fn: delta shape {tuple(delta.shape)} != u shape {tuple(u.shape)}")
    if A.dim() != 2 or A.shape[0] != dim:
        raise RuntimeError(f"selective_scan_fn: A must be (dim, N) with dim={dim}, got {tuple(A.shape)}")
    N = A.shape[1]
    if B.dim() == 2 or C.dim() == 2:
        raise NotImplementedError("selective_scan_fn: time-invariant (dim, N) B/C are not implemented; "
                                  "the reference only uses (batch, G, N, L) B/C (wavemamba_arch.py:459-460)")
    if B.dim() == 3:
        B = B.unsqueeze(1)
    if C.dim() == 3:
        C = C.unsqueeze(1)
    G = B.shape[1]
    if B.shape != (batch, G, N, L) or C.shape != (batch, G, N, L):
        raise RuntimeError(f"selective_scan_fn: B/C must be (batch, G, N, L) = ({batch}, G, {N}, {L}), "
                           f"got {tuple(B.shape)} / {tuple(C.shape)}")
    if dim % G:
        raise RuntimeError(f"selective_scan_fn: dim {dim} not divisible by the number of groups {G}")
    for name, t in (("D", D), ("delta_bias", delta_bias)):
        if t is not None and t.shape != (dim,):
            raise RuntimeError(f"selective_scan_fn: {name} must be ({dim},), got {tuple(t.shape)}")
    if z is not None and z.shape != u.shape:
        raise RuntimeError("selective_scan_fn: z shape must match u")
    return batch, dim, L, N, G, B, C


def _f32c(t):
    return None if t is None else t.contiguous().float()


def _scan_forward(u, delta, A, B, C, D, z, delta_bias, delta_softplus, want_last):
    lib = _lib.load()
    batch, dim, L, N, G = u.shape[0], u.shape[1], u.shape[2], A.shape[1], B.shape[1]
    out = torch.empty_like(u)
    last = torch.empty((batch, dim, N), dtype=torch.float32, device=u.device) if want_last else None
    ws_bytes = lib.wm_selscan_fwd_workspace_bytes(batch, dim, L, N, G)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=u.device) if ws_bytes else None
    _launch(u.device, "wm_selscan_fwd", u, delta, A, B, C, D, z, delta_bias, out, last, ws, ws_bytes,
            batch, dim, L, N, G, int(bool(delta_softplus)))
    return out, last


class _SelectiveScan(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, delta, A, B, C, D, delta_bias, delta_softplus, want_last):
        out, last = _scan_forward(u, delta, A, B, C, D, None, delta_bias, delta_softplus, want_last)
        ctx.save_for_backward(u, delta, A, B, C, D, delta_bias)
        ctx.delta_softplus = bool(delta_softplus)
        if want_last:
            ctx.mark_non_differentiable(last)
            return out, last
        return out

    @staticmethod
    def backward(ctx, dout, *unused):
        lib = _lib.load()
        u, delta, A, B, C, D, delta_bias = ctx.saved_tensors
        batch, dim, L = u.shape
        N, G = A.shape[1], B.shape[1]
        dout = dout.contiguous().float()
        du = torch.empty_like(u)
        ddelta = torch.empty_like(delta)
        dA = torch.empty_like(A)
        dB = torch.empty_like(B)
        dC = torch.empty_like(C)
        dD = torch.empty_like(D) if D is not None else None
        dbias = torch.empty_like(delta_bias) if delta_bias is not None else None
        if _DETERMINISTIC:
            ws_bytes = lib.wm_selscan_bwd_det_workspace_bytes(batch, dim, L, N, G)
            ws = _det_workspace(ws_bytes, u.device)
            _launch(u.device, "wm_selscan_bwd_det", u, delta, A, B, C, D, delta_bias, dout, du, ddelta, dA, dB, dC, dD, dbias,
                    ws, ws_bytes, batch, dim, L, N, G, int(ctx.delta_softplus))
            return du, ddelta, dA, dB, dC, dD, dbias, None, None
        ws_bytes = lib.wm_selscan_bwd_workspace_bytes(batch, dim, L, N, G)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=u.device) if ws_bytes else None
        _launch(u.device, "wm_selscan_bwd", u, delta, A, B, C, D, delta_bias, dout, du, ddelta, dA, dB, dC, dD, dbias,
                ws, ws_bytes, batch, dim, L, N, G, int(ctx.delta_softplus))
        return du, ddelta, dA, dB, dC, dD, dbias, None, None


def selective_scan_fn(u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False,
                      return_last_state=False):
    """Drop-in for mamba_ssm.ops.selective_scan_interface.selective_scan_fn (reference call site
    wavemamba_arch.py:465-471).  u, delta: (batch, dim, L); A: (dim, N); B, C: (batch, [G,] N, L);
    D, delta_bias: (dim,).  Computes in fp32, returns `out` in u's dtype (and the fp32 last state
    (batch, dim, N) when return_last_state).  Differentiable w.r.t. u, delta, A, B, C, D, delta_bias
    (and z, through eager gating).  CPU tensors: cpu_twin.selective_scan_fn (plain PyTorch, same signature)."""
    if _on_cpu(u, delta, A, B, C, D, z, delta_bias):
        from . import cpu_twin
        return cpu_twin.selective_scan_fn(u, delta, A, B, C, D, z, delta_bias, delta_softplus, return_last_state)
    _require_cuda("selective_scan_fn", u, delta, A, B, C, D, z, delta_bias)
    batch, dim, L, N, G, B4, C4 = _scan_shapes(u, delta, A, B, C, D, z, delta_bias)
    squeeze_B, squeeze_C = B.dim() == 3, C.dim() == 3
    in_dtype = u.dtype
    args = [_f32c(t) for t in (u, delta, A, B4, C4, D, delta_bias)]
    need_grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad
                                                for t in (u, delta, A, B, C, D, z, delta_bias))
    if not need_grad:
        out, last = _scan_forward(args[0], args[1], args[2], args[3], args[4], args[5], _f32c(z),
                                  args[6], delta_softplus, return_last_state)
    else:
        res = _SelectiveScan.apply(*args, bool(delta_softplus), bool(return_last_state))
        out, last = res if return_last_state else (res, None)
        if z is not None:
            out = out * F.silu(z.float())
    out = out.to(in_dtype)
    return (out, last) if return_last_state else out


# ------------------------------------------------------------------------------------------------
# fused SS2D four-direction core (forward / inference)
# ------------------------------------------------------------------------------------------------
def ss2d_core_supported(d_inner, d_state, dt_rank, width=None, height=None):
    """Shapes the fused HIP core covers (else: direction glue + selective_scan_fn).  Any map size (widths that are not
    a multiple of 4 take the kernels' element-wise tile accesses); with `width` and `height`, maps beyond the kernels'
    32-bit element offsets (d_inner * H * W >= 2^31, csrc/scan_fwd.hip: core_plan) are refused here instead of at the
    call."""
    if d_inner > 64 or dt_rank > 4 or d_state > 32:
        return False
    if width is not None and height is not None and d_inner * width * height > 2 ** 31 - 1:
        return False
    return True


def ss2d_core_bwd_supported(d_inner, d_state, dt_rank):
    """Shapes wm_ss2d_core_bwd covers (training): d_state <= 32 (BASELINE config 5's block included)."""
    return d_inner <= 64 and d_state <= 32 and dt_rank <= 4


def _ss2d_core_shapes(x, x_proj_weight, dt_projs_weight, A_logs):
    B, D, H, W = x.shape
    K, C, D2 = x_proj_weight.shape
    R, N = dt_projs_weight.shape[2], A_logs.shape[1]
    if K != 4 or D2 != D or C != R + 2 * N or dt_projs_weight.shape != (4, D, R) or A_logs.shape[0] != 4 * D:
        raise RuntimeError("ss2d_core: inconsistent parameter shapes")
    if not ss2d_core_supported(D, N, R, W, H):
        raise NotImplementedError(f"ss2d_core: d_inner={D}, d_state={N}, dt_rank={R} outside the fused kernel's range")
    return B, D, H, W, N, R


def _host_wait_under_capture(event):
    """Block the host until `event` (recorded before the capture began) has completed.  event.synchronize() is one of the
    calls that invalidate a capture in the global capture mode (hipErrorStreamCaptureUnsupported, then
    hipErrorStreamCaptureInvalidated at the next launch - torch.cuda.graph's default mode): the library does it under a
    thread-local relaxed mode (wm_event_synchronize_relaxed)."""
    check(_lib.load().wm_event_synchronize_relaxed(event.cuda_event), "wm_event_synchronize_relaxed")


class _PreparedCache:
    """Prepared device copies of parameters (the SS2D core's constants, the convolutions' weight fragments), one per tuple of
    parameter objects, keyed by the first of them.  An entry is valid while every object is the same one with the same
    `data_ptr`, `_version` and dtype - a write through `.data` bumps no version: see conv2d_cache_clear - and leaves when its
    first parameter dies.  It remembers the stream it was built on and an event recorded behind the preparation kernel, so a
    use from another stream never reads the copy before it is complete nor sees it freed under a pending launch."""

    def __init__(self):
        self._ent = {}      # id(params[0]) -> (weakrefs, signature, buffer, done event, producer stream, eviction hook)

    @staticmethod
    def _sig(params):
        return tuple((p.data_ptr(), p._version, p.dtype) for p in params)

    def get(self, params):
        """The valid cached copy for `params`, made safe to use on the current stream - or None."""
        ent = self._ent.get(id(params[0]))
        if ent is None or not all(r() is p for r, p in zip(ent[0], params)) or ent[1] != self._sig(params):
            return None
        buf, ev, stream = ent[2:5]
        cur = torch.cuda.current_stream(params[0].device)
        if stream != cur.cuda_stream:
            if torch.cuda.is_current_stream_capturing():
                # an event recorded outside the capture cannot be waited for inside it: block the HOST until the producer
                # (a warm-up forward on another stream that was never joined) is done, then the buffer is simply there
                _host_wait_under_capture(ev)
            else:
                cur.wait_event(ev)
                buf.record_stream(cur)
        return buf

    def put(self, params, buf):
        """`buf` was just prepared from `params` on the current stream: keep it."""
        key = id(params[0])
        cur = torch.cuda.current_stream(params[0].device)
        ev = torch.cuda.Event()
        ev.record(cur)
        old = self._ent.get(key)        # an entry under this key is this object's (a dead object's entry is gone): one hook per object
        hook = old[5] if old is not None else weakref.finalize(params[0], self._ent.pop, key, None)
        self._ent[key] = ([weakref.ref(p) for p in params], self._sig(params), buf, ev, cur.cuda_stream, hook)

    def clear(self):
        for ent in self._ent.values():
            ent[5].detach()
        self._ent.clear()


_CORE_PREP_CACHE = _PreparedCache()
_WFRAG_CACHE = _PreparedCache()


def _ss2d_core_prepared(params):
    """The prepared copy (wm_ss2d_core_prep: bf16-split x_proj fragments, A * log2(e), per-channel constants) of the five
    SS2D parameters `params` = (x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds), kept per module while the
    parameters are unchanged (`_version`, storage) - inference runs the core 14 times per image with static parameters.
    Returns None (the call prepares for itself) for parameters that require grad (training updates them every step),
    under graph capture, and for temporaries."""
    if any((not isinstance(p, torch.nn.Parameter)) or p.requires_grad and torch.is_grad_enabled() for p in params):
        return None
    buf = _CORE_PREP_CACHE.get(params)
    if buf is not None or torch.cuda.is_current_stream_capturing():
        return buf                                   # cold cache under capture: None, the call prepares for itself inside the graph
    f = [_w(p) for p in params]
    D, R, N = f[1].shape[1], f[1].shape[2], f[3].shape[1]
    buf = torch.empty(_lib.load().wm_ss2d_core_prep_bytes(N), dtype=torch.uint8, device=f[0].device)
    _launch(buf.device, "wm_ss2d_core_prep", *f, buf, D, N, R)
    _CORE_PREP_CACHE.put(params, buf)
    return buf


def _ss2d_core_fwd(f, merged, prepared=None, separate=False):
    """f[0] = x (fp32 or bf16 planes: the outputs take the same storage type), f[1:] fp32 parameters; `prepared`: the
    buffer of _ss2d_core_prepared for these parameters, or None.  separate: four allocations instead of one (4, B, D, L)
    block (torch.library ops must not return tensors that share a storage)."""
    lib = _lib.load()
    x = f[0]
    B, D, H, W, N, R = _ss2d_core_shapes(x, f[1], f[2], f[4])
    L = H * W
    if merged:
        outs = [torch.empty((B, D, L), dtype=x.dtype, device=x.device)]
    elif separate:
        outs = [torch.empty((B, D, L), dtype=x.dtype, device=x.device) for _ in range(4)]
    else:       # one allocation, reference return order: a consumer can add the four with one base pointer + stride
        outs = list(torch.empty((4, B, D, L), dtype=x.dtype, device=x.device).unbind(0))
    ws_bytes = lib.wm_ss2d_core_fwd_workspace_bytes(B, D, H, W, N, R, int(merged))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    _launch(x.device, "wm_ss2d_core_fwd", *f, *outs, *[None] * (4 - len(outs)), int(merged), ws, ws_bytes, prepared,
            B, D, H, W, N, R, _dtype_code(x, "ss2d_core"))
    return outs


class _SS2DCoreFn(torch.autograd.Function):
    """SS2D.forward_core with HIP forward (wm_ss2d_core_fwd) and HIP backward (wm_ss2d_core_bwd).  Nothing but x and
    the parameters is saved: the backward re-runs the projection and the chunked scan from them."""

    @staticmethod
    def forward(ctx, merged, x, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds):
        f = [t.detach().contiguous().float() for t in (x, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds)]
        ctx.save_for_backward(*f)
        ctx.merged = merged
        outs = _ss2d_core_fwd(f, merged)
        return outs[0] if merged else tuple(outs)

    @staticmethod
    def backward(ctx, *dys):
        lib = _lib.load()
        f = ctx.saved_tensors
        x = f[0]
        B, D, H, W, N, R = _ss2d_core_shapes(x, f[1], f[2], f[4])
        if ctx.merged:
            g = dys[0].contiguous().float()
            dy = [g, g, g, g]
        else:
            dy = [(torch.zeros((B, D, H * W), dtype=torch.float32, device=x.device) if g is None else g.contiguous().float())
                  for g in dys]
        outs = [torch.empty_like(x), torch.empty_like(f[1]), torch.empty_like(f[2]), torch.empty_like(f[3]),
                torch.empty_like(f[4]), torch.empty_like(f[5])]
        ws_bytes = lib.wm_ss2d_core_bwd_workspace_bytes(B, D, H, W, N, R)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
        _launch(x.device, "wm_ss2d_core_bwd", *f, *dy, *outs, ws, ws_bytes, B, D, H, W, N, R)
        return (None, *outs)


def ss2d_core(x, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds, merged=False):
    """SS2D.forward_core (reference wavemamba_arch.py:446-478) in one call.
    x (B, D, H, W) fp32 -> (y_row_fwd, y_row_rev, y_col_fwd, y_col_rev), each (B, D, H*W) in
    row-major l - the reference's return order; merged=True returns their sum (what :490 computes).
    Differentiable w.r.t. x and the five parameters (HIP backward, wm_ss2d_core_bwd)."""
    _require_cuda("ss2d_core", x, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds)
    _ss2d_core_shapes(x, x_proj_weight, dt_projs_weight, A_logs)
    args = (x, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds)
    if torch.is_grad_enabled() and any(t.requires_grad for t in args):
        return _SS2DCoreFn.apply(bool(merged), *args)
    xin = x.detach().contiguous()
    if xin.dtype != torch.bfloat16:                # bf16 planes stay bf16 (outputs too); anything else computes in fp32
        xin = xin.float()
    outs = _ss2d_core_fwd([xin] + [t.detach().contiguous().float() for t in args[1:]], int(bool(merged)),
                          _ss2d_core_prepared(args[1:]))
    return outs[0] if merged else tuple(outs)


# ------------------------------------------------------------------------------------------------
# LFSSBlock forward, fused (inference): lfss_in -> dwconv+SiLU -> ss2d core -> lfss_mid -> dwconv -> lfss_out
# ------------------------------------------------------------------------------------------------
def lfss_block_supported(C, d_inner, d_state, dt_rank, ffn_hidden, width=None, height=None):
    return (C in (8, 16, 32) and d_inner == 2 * C and ffn_hidden == 2 * C
            and ss2d_core_supported(d_inner, d_state, dt_rank, width, height))


def _w(t):
    return t.detach().contiguous().float()


_FUSE_OUT_CONV = True      # tests / tools: False takes wm_dwconv3x3_fwd + wm_lfss_out_fwd (bit-identical on fp32 planes)
# ln_1 -> in_proj -> depth-wise 3x3 -> SiLU as ONE kernel (wm_lfss_in_conv_fwd: x = in_proj(ln_1(tok))[:D] never reaches HBM, 512 B
# per position fewer; bit-identical on fp32 planes).  It needs the recomputed gate (nothing writes z on that path) and fp32 planes
# (bf16-plane mode rounds x after lfss_in: tests/test_bf16_planes.py).  False: wm_lfss_in_fwd + wm_dwconv3x3_fwd, tests and tools.
_FUSE_IN_CONV = True
# The maps the one-kernel prologue takes: those the entry supports (W % 32 == 0, H W <= 2^23) with at least as many positions PER IMAGE
# as the smallest map at which it measured faster (UHD level 2; the kernel's bands and strips are laid out per image, and only B = 1
# was measured).  Per call, pair -> fused, median of 7 x 20 calls with [slowest fused, fastest pair], NCHW / token-row input
# (tools/bench_lfss_in_conv.py, profiles/lfss_in_conv/per_call.txt):
#   UHD level 1 (1088 x 1920)  0.431 -> 0.297 ms [0.323, 0.431] / 0.455 -> 0.277 ms [0.292, 0.452]
#   UHD level 2 ( 544 x  960)  0.119 -> 0.091 ms [0.093, 0.119] / 0.126 -> 0.088 ms [0.088, 0.126]
#   UHD level 3 ( 272 x  480)  0.037 -> 0.049 ms: 136 workgroups of long-lived waves leave half the chip idle - the pair stays
# No map between levels 3 and 2 was measured: those keep the pair until one is.
_FUSE_IN_CONV_MIN_POSITIONS = 544 * 960
# The gate z = in_proj(ln_1(x))[D:] recomputed by lfss_mid from the tokens instead of written by lfss_in and read back
# (512 of the block's 3456 B per position; bit-identical in fp32 planes: tests/test_gpu_parity.py).  0: round-3 data flow.
_RECOMPUTE_Z = True
# ln_2 -> conv1 -> depth-wise 3x3 -> GELU gate -> conv3 -> skip as ONE kernel behind a middle kernel that ends at tok1
# (wm_lfss_mid_rz_tok_fwd + wm_lfss_ffn_fwd: f = conv1(ln_2(tok1)) never reaches HBM; bit-identical on fp32 planes).  It needs the
# recomputed gate, fp32 planes and inference.  False: wm_lfss_mid_rz_fwd + wm_lfss_out_conv_fwd, tests and tools.
_FUSE_FFN = True
# The maps the new pair takes: those the entry supports with at least as many positions PER IMAGE as the smallest map at which it
# measured faster than the old pair (tools/bench_lfss_ffn.py, profiles/lfss_ffn/per_call.txt; only B = 1 was measured): the new pair's
# slowest repetition is below the old pair's fastest at UHD level 1 (1088 x 1920, about 0.13 ms per call) and level 2 (544 x 960,
# about 0.02 ms); at level 3 (272 x 480) the new pair is 0.01 ms SLOWER - 1088 four-row walks fill half the chip - and the old pair
# stays.  No map between levels 3 and 2 was measured: those keep the old pair until one is.
_FUSE_FFN_MIN_POSITIONS = 544 * 960


def _fuse_ffn_map(B, H, W):
    """Maps on which lfss_block_forward takes wm_lfss_mid_rz_tok_fwd + wm_lfss_ffn_fwd: inside the entry's domain and, per image, at
    least as large as the smallest map at which the pair measured faster than wm_lfss_mid_rz_fwd + wm_lfss_out_conv_fwd."""
    return B > 0 and W % 32 == 0 and _FUSE_FFN_MIN_POSITIONS <= H * W <= (1 << 23)


def _fuse_in_conv_map(B, H, W):
    """Maps on which lfss_block_forward takes wm_lfss_in_conv_fwd: inside the entry's domain and, per image, at least as large as
    the smallest map at which it measured faster than the pair."""
    return B > 0 and W % 32 == 0 and _FUSE_IN_CONV_MIN_POSITIONS <= H * W <= (1 << 23)


def lfss_block_forward(tok, x_size, blk, tok_nchw=False, out_nchw=False):
    """LFSSBlock.forward (reference wavemamba_arch.py:520-528) on the HIP path, forward only.
    tok: (B, L, C) tokens, or (B, C, H, W) when tok_nchw.  `blk` supplies the parameters (an LFSSBlock
    module: ln_1, self_attention, skip_scale, conv_blk, ln_2, skip_scale2).  Returns (B, L, C) tokens or
    (B, C, H, W) when out_nchw."""
    _require_cuda("lfss_block_forward", tok)
    H, W = x_size
    L = H * W
    ss, ff = blk.self_attention, blk.conv_blk
    C, D = ss.d_model, ss.d_inner
    B = tok.shape[0]
    tok = tok.contiguous().float()
    dev = tok.device
    # bf16 planes: the C = 32 kernels on maps with 16-byte tile accesses (W % 4 == 0); else fp32 planes
    pd = _PLANE_DTYPE if (C == 32 and W % 4 == 0) else torch.float32
    code = WM_F32 if pd == torch.float32 else WM_BF16
    # C == 32: the gate z is recomputed by the block's middle kernel from the tokens it reads anyway (wm_lfss_mid_rz_fwd, bit-identical
    # in fp32 planes) - lfss_in writes the x half only (ops._RECOMPUTE_Z = False: the written / re-read z, tests and tools)
    rz = C == 32 and _RECOMPUTE_Z
    # SS2D's prologue as one kernel: x (in_proj's first half) never reaches HBM
    fuse_in = rz and _FUSE_IN_CONV and pd == torch.float32 and _fuse_in_conv_map(B, H, W)
    # the ffn's depth-wise 3x3 inside the closing kernel: fc (conv2's output) never reaches HBM
    fuse_out = C == 32 and W % 32 == 0 and _FUSE_OUT_CONV
    # the parameters the block's own launches read, each normalised once per call (nothing is kept across calls: a write through
    # `.data` shows in the next forward); the depth-wise convolutions outside the fused closing kernel normalise their own
    ln1 = (_w(blk.ln_1.weight), _w(blk.ln_1.bias), float(blk.ln_1.eps), _w(ss.in_proj.weight))
    core_params = (ss.x_proj_weight, ss.dt_projs_weight, ss.dt_projs_bias, ss.A_logs, ss.Ds)
    core_w = [_w(t) for t in core_params]
    mid = (_w(ss.out_norm.weight), _w(ss.out_norm.bias), float(ss.out_norm.eps), _w(ss.out_proj.weight), _w(blk.skip_scale),
           _w(blk.ln_2.weight), _w(blk.ln_2.bias), float(blk.ln_2.eps), _w(ff.conv1.weight), _w(ff.conv1.bias))
    conv2 = (_w(ff.conv2.weight), None if ff.conv2.bias is None else _w(ff.conv2.bias)) if fuse_out else None
    tail = (_w(ff.conv3.weight), _w(ff.conv3.bias), _w(blk.skip_scale2))

    z = None if rz else torch.empty((B, D, L), dtype=pd, device=dev)
    if fuse_in:
        xc = torch.empty((B, D, H, W), dtype=pd, device=dev)
        _launch(dev, "wm_lfss_in_conv_fwd", tok, int(tok_nchw), *ln1, _w(ss.conv2d.weight),
                None if ss.conv2d.bias is None else _w(ss.conv2d.bias), xc, B, H, W, C, code)
    else:
        x = torch.empty((B, D, H, W), dtype=pd, device=dev)
        _launch(dev, "wm_lfss_in_fwd", tok, int(tok_nchw), *ln1, x, z, B, L, C, code)
        xc = dwconv3x3(x, ss.conv2d.weight, ss.conv2d.bias, "silu")
    # the four directions' outputs stay separate (one (4, B, D, L) allocation); lfss_mid adds them as it loads (:490)
    ny = 4
    y4 = _ss2d_core_fwd([xc] + core_w, merged=0, prepared=_ss2d_core_prepared(core_params))
    tok1 = torch.empty((B, L, C), dtype=torch.float32, device=dev)
    out = torch.empty((B, C, H, W) if out_nchw else (B, L, C), dtype=torch.float32, device=dev)
    # the gated ffn as one kernel: f (conv1's output) never reaches HBM
    if rz and _FUSE_FFN and pd == torch.float32 and _fuse_ffn_map(B, H, W):
        _launch(dev, "wm_lfss_mid_rz_tok_fwd", y4[0], ny, B * D * L, tok, int(tok_nchw), *ln1, *mid[:5], tok1, B, L, C, code)
        _launch(dev, "wm_lfss_ffn_fwd", tok1, *mid[5:], _w(ff.conv2.weight), None if ff.conv2.bias is None else _w(ff.conv2.bias),
                *tail, out, int(out_nchw), B, H, W, C, code, 0)
        return out
    f = torch.empty((B, D, H, W), dtype=pd, device=dev)
    if rz:
        _launch(dev, "wm_lfss_mid_rz_fwd", y4[0], ny, B * D * L, tok, int(tok_nchw), *ln1, *mid, tok1, f, B, L, C, code)
    else:
        _launch(dev, "wm_lfss_mid_fwd", y4[0], ny, B * D * L, z, tok, int(tok_nchw), *mid, tok1, f, B, L, C, code)
    if fuse_out:
        _launch(dev, "wm_lfss_out_conv_fwd", f, *conv2, tok1, *tail, out, int(out_nchw), B, H, W, C, code)
        return out
    fc = dwconv3x3(f, ff.conv2.weight, ff.conv2.bias, "none")
    _launch(dev, "wm_lfss_out_fwd", fc, tok1, *tail, out, int(out_nchw), B, L, C, code)
    return out


# ------------------------------------------------------------------------------------------------
# LayerNorm2d (HFE branch, forward only)
# ------------------------------------------------------------------------------------------------
def layernorm2d_supported(x):
    """Maps wm_layernorm2d_fwd / _bwd cover (layernorm2d, layernorm2d_train): fp32 NCHW, C in {8, 16, 32, 64}."""
    return x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] in (8, 16, 32, 64)


def layernorm2d(x, weight, bias, eps):
    """Per-pixel LayerNorm over channels of an NCHW fp32 map (reference LayerNorm2d, :532-569)."""
    _require_cuda("layernorm2d", x, weight, bias)
    B, C, H, W = x.shape
    if not layernorm2d_supported(x):
        raise NotImplementedError("layernorm2d: fp32, C in {8, 16, 32, 64}")
    x = x.contiguous()
    y = torch.empty_like(x)
    _launch(x.device, "wm_layernorm2d_fwd", x, _w(weight), _w(bias), float(eps), y, B, H * W, C)
    return y


# ------------------------------------------------------------------------------------------------
# channel Gram matrix over pixels (HFE branch, forward only)
# ------------------------------------------------------------------------------------------------
def gram_supported(x, y):
    """Pairs wm_gram_fwd covers (gram, gram_train): two fp32 (B, C <= 32, L) tensors of equal shape."""
    return (x.is_cuda and x.dtype == torch.float32 and y.dtype == torch.float32 and x.shape == y.shape
            and x.shape[1] <= 32)


def gram(x, y):
    """x, y (B, C, L) fp32, C <= 32 -> (G (B, C, C) = x @ y^T over L, |x_i|^2 (B, C), |y_j|^2 (B, C))."""
    lib = _lib.load()
    _require_cuda("gram", x, y)
    B, C, L = x.shape
    if not gram_supported(x, y):
        raise NotImplementedError("gram: two fp32 (B, C<=32, L) tensors of equal shape")
    x, y = x.contiguous(), y.contiguous()
    buf = torch.empty(B * C * (C + 2), dtype=torch.float32, device=x.device)
    G = buf[:B * C * C].view(B, C, C)
    nx = buf[B * C * C:B * C * (C + 1)].view(B, C)
    ny = buf[B * C * (C + 1):].view(B, C)
    nws = int(lib.wm_gram_workspace_bytes(B, C, L))
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=x.device)
    _launch(x.device, "wm_gram_fwd", x, y, G, nx, ny, ws, nws, B, C, L)
    return G, nx, ny


class _GramTrain(torch.autograd.Function):
    """gram() under autograd: (G, |x|^2, |y|^2) of x, y (B, C, L).  Backward: dx = dG y + 2 d|x|^2 x, dy = dG^T x + 2 d|y|^2 y
    (two batched GEMMs and two scaled adds).  The training-side form of the transposed attention's
    normalize(q) @ normalize(k)^T (reference :783-786): one pass over q and k instead of two normalisations and a batched
    product, and the division by the norms happens on the (B, C, C) result."""

    @staticmethod
    def forward(ctx, x, y):
        x, y = x.contiguous(), y.contiguous()
        ctx.save_for_backward(x, y)
        G, nx, ny = gram(x, y)
        return G, nx, ny

    @staticmethod
    def backward(ctx, dG, dnx, dny):
        x, y = ctx.saved_tensors
        dx = dy = None
        if ctx.needs_input_grad[0]:
            dx = torch.bmm(dG, y) if dG is not None else torch.zeros_like(x)
            if dnx is not None:
                dx.addcmul_(x, dnx.unsqueeze(2), value=2.0)
        if ctx.needs_input_grad[1]:
            dy = torch.bmm(dG.transpose(1, 2), x) if dG is not None else torch.zeros_like(y)
            if dny is not None:
                dy.addcmul_(y, dny.unsqueeze(2), value=2.0)
        return dx, dy


def gram_train(x, y):
    """gram(x, y) with gradients (x, y (B, C <= 32, L) fp32 HIP tensors)."""
    return _GramTrain.apply(x, y)


class _DWConvTrain(torch.autograd.Function):
    """Depth-wise 3x3 conv (+bias) with HIP forward, input gradient (the same kernel on the flipped weight) and
    weight / bias gradient (strip reduction).  Training-side replacement of MIOpen's naive depth-wise kernels."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return dwconv3x3(x, weight, bias, "none")

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gy = gy.contiguous().float()
        B, C, H, W = x.shape
        gx = dwconv3x3(gy, weight, None, "none", flip=True)
        if _DETERMINISTIC:
            dW = torch.empty_like(weight, dtype=torch.float32, memory_format=torch.contiguous_format)
            db = torch.empty(C, dtype=torch.float32, device=x.device) if ctx.has_bias else None
            nb = _lib.load().wm_dwconv3x3_wgrad_det_workspace_bytes(B, C, H, W)
            _launch(x.device, "wm_dwconv3x3_wgrad_det", x.contiguous(), gy, dW, db, _det_workspace(nb, x.device), nb, B, C, H, W)
            return gx, dW, db
        buf = _zeros_small(10 * C, x.device)                                    # dW | db back to back, zeroed
        dW = buf[:9 * C].view(weight.shape)
        db = buf[9 * C:] if ctx.has_bias else None
        _launch(x.device, "wm_dwconv3x3_wgrad", x.contiguous(), gy, dW, db, B, C, H, W)
        return gx, dW, db


def dwconv3x3_train(x, weight, bias=None):
    """Differentiable depth-wise 3x3 conv (stride 1, padding 1) on the HIP path (fp32 NCHW)."""
    _require_cuda("dwconv3x3_train", x, weight, bias)
    return _DWConvTrain.apply(x.contiguous().float(), weight, bias)


class _LayerNorm2dTrain(torch.autograd.Function):
    """LayerNorm2d with HIP forward and backward (reference LayerNormFunction, wavemamba_arch.py:532-557)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        ctx.save_for_backward(x, weight)
        ctx.eps = float(eps)
        return layernorm2d(x, weight, bias, eps)

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        B, C, H, W = x.shape
        gy = gy.contiguous().float()
        gx = torch.empty_like(x)
        if _DETERMINISTIC:
            buf = torch.empty(2 * C, dtype=torch.float32, device=x.device)
            nb = _lib.load().wm_layernorm2d_bwd_det_workspace_bytes(B, H * W, C)
            _launch(x.device, "wm_layernorm2d_bwd_det", x, _w(weight), gy, ctx.eps, gx, buf[:C], buf[C:], _det_workspace(nb, x.device),
                    nb, B, H * W, C)
            return gx, buf[:C], buf[C:], None
        buf = _zeros_small(2 * C, x.device)                                     # dweight | dbias back to back, zeroed
        dw, db = buf[:C], buf[C:]
        _launch(x.device, "wm_layernorm2d_bwd", x, _w(weight), gy, ctx.eps, gx, dw, db, B, H * W, C)
        return gx, dw, db, None


def layernorm2d_train(x, weight, bias, eps):
    _require_cuda("layernorm2d_train", x, weight, bias)
    return _LayerNorm2dTrain.apply(x.contiguous().float(), weight, bias, eps)


class _LayerNormTok(torch.autograd.Function):
    """nn.LayerNorm(C) over the last axis of a contiguous (..., C) fp32 tensor: HIP forward and backward."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        C = x.shape[-1]
        w, b = _w(weight), _w(bias)
        y = torch.empty_like(x)
        _launch(x.device, "wm_layernorm_tok_fwd", x, w, b, float(eps), y, x.numel() // C, C)
        ctx.save_for_backward(x, w)
        ctx.eps = float(eps)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        C = x.shape[-1]
        gy = gy.contiguous().float()
        gx = torch.empty_like(x)
        if _DETERMINISTIC:
            buf = torch.empty(2 * C, dtype=torch.float32, device=x.device)
            T = x.numel() // C
            nb = _lib.load().wm_layernorm_tok_bwd_det_workspace_bytes(T, C)
            _launch(x.device, "wm_layernorm_tok_bwd_det", x, w, gy, ctx.eps, gx, buf[:C], buf[C:], _det_workspace(nb, x.device), nb, T, C)
            return gx, buf[:C], buf[C:], None
        buf = _zeros_small(2 * C, x.device)
        dw, db = buf[:C], buf[C:]
        _launch(x.device, "wm_layernorm_tok_bwd", x, w, gy, ctx.eps, gx, dw, db, x.numel() // C, C)
        return gx, dw, db, None


def layernorm_tok_supported(x, C):
    return x.is_cuda and x.dtype == torch.float32 and x.shape[-1] == C and C in (8, 16, 32, 64)


def layernorm_tok(x, weight, bias, eps):
    """F.layer_norm(x, (C,), weight, bias, eps) for a (..., C) fp32 tensor, C in {8, 16, 32, 64}; differentiable
    (HIP backward: input gradient + weight / bias gradients in one pass)."""
    _require_cuda("layernorm_tok", x, weight, bias)
    x = x.contiguous().float()
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or bias.requires_grad):
        return _LayerNormTok.apply(x, weight, bias, eps)
    return _LayerNormTok.forward(_NoCtx(), x, weight, bias, eps)


class _NoCtx:
    def save_for_backward(self, *a):
        pass


# ------------------------------------------------------------------------------------------------
# element-wise gates and scaled skips of the LFSSBlock training path (forward + backward in HIP)
# ------------------------------------------------------------------------------------------------
_ACTS = {"silu": 1, "gelu": 2, "sigmoid": 3}


def _batch_strided(t):
    """(B, ...) tensor whose batch items are dense: -> batch stride in elements, or None."""
    if t.dim() < 2 or t.dtype != torch.float32:
        return None
    inner = t[0]
    return t.stride(0) if inner.is_contiguous() else None


class _Gate(torch.autograd.Function):
    """out = act(a) * b (wm_gate_fwd / wm_gate_bwd): SS2D's `y * F.silu(z)` (reference :493) and the ffn's
    `F.gelu(x1) * x2` (:228-229).  a, b: (B, C, H, W) fp32, each dense per batch item (channel-chunk views are fine)."""

    @staticmethod
    def forward(ctx, a, b, act):
        B, per_b = a.shape[0], a[0].numel()
        out = torch.empty(a.shape, dtype=torch.float32, device=a.device)
        _launch(a.device, "wm_gate_fwd", a, b, out, act, B, per_b, a.stride(0), b.stride(0), out.stride(0) if B else 0)
        ctx.save_for_backward(a, b)
        ctx.act = act
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous().float()
        B, per_b = a.shape[0], a[0].numel()
        ga, gb = torch.empty_like(g), torch.empty_like(g)
        _launch(a.device, "wm_gate_bwd", a, b, g, ga, gb, ctx.act, B, per_b, a.stride(0), b.stride(0),
                g.stride(0) if B else 0, ga.stride(0) if B else 0, gb.stride(0) if B else 0)
        return ga, gb, None


class _GluGate(torch.autograd.Function):
    """out = act(t[:, :C]) * t[:, C:] for t (B, 2C, H, W): the gated ffn's chunk + gate as one node, so that the backward
    writes ONE gradient tensor in t's layout (autograd's backward of a chunk would concatenate two)."""

    @staticmethod
    def forward(ctx, t, act):
        t = t.contiguous().float()
        B, C2 = t.shape[:2]
        C = C2 // 2
        per_b = C * t[0, 0].numel()
        out = torch.empty((B, C) + tuple(t.shape[2:]), dtype=torch.float32, device=t.device)
        _launch(t.device, "wm_gate_fwd", t, t.data_ptr() + 4 * per_b, out, act, B, per_b, 2 * per_b, 2 * per_b, per_b)
        ctx.save_for_backward(t)
        ctx.act = act
        return out

    @staticmethod
    def backward(ctx, g):
        (t,) = ctx.saved_tensors
        g = g.contiguous().float()
        B, per_b = t.shape[0], g[0].numel()
        gt = torch.empty_like(t)
        _launch(t.device, "wm_gate_bwd", t, t.data_ptr() + 4 * per_b, g, gt, gt.data_ptr() + 4 * per_b, ctx.act, B,
                per_b, 2 * per_b, 2 * per_b, per_b, 2 * per_b, 2 * per_b)
        return gt, None


def glu_gate_supported(t):
    """Tensors _GluGate covers: fp32 (B, 2C, H, W) with B <= 65535 (the batch is a grid dimension of wm_gate_fwd / _bwd)."""
    return t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.shape[1] % 2 == 0 and t.shape[0] <= 65535


def glu_gate(t, act):
    """act(t[:, :C]) * t[:, C:] for a (B, 2C, H, W) fp32 tensor, act in {"silu", "gelu"}, differentiable (_GluGate)."""
    _require_cuda("glu_gate", t)
    if not glu_gate_supported(t):
        raise NotImplementedError("glu_gate: a (B, 2C, H, W) tensor")
    return _GluGate.apply(t, _ACTS[act])


def gate_supported(a, b):
    return (a.is_cuda and b.is_cuda and a.shape == b.shape and a.dim() == 4 and _batch_strided(a) is not None
            and _batch_strided(b) is not None and a.shape[0] <= 65535)


def gate_act(a, b, act):
    """act(a) * b with act in {"silu", "gelu", "sigmoid"} (exact erf GELU), differentiable; see _Gate."""
    _require_cuda("gate_act", a, b)
    if not gate_supported(a, b):
        raise NotImplementedError("gate_act: two fp32 (B, C, H, W) tensors, dense per batch item")
    return _Gate.apply(a, b, _ACTS[act])


class _ScaleAdd(torch.autograd.Function):
    """out = x * scale[c] + o over (B, C, H, W) (wm_scale_add_fwd / _bwd): LFSSBlock's scaled skips (reference :525-526)."""

    @staticmethod
    def forward(ctx, x, scale, o):
        x, o, sc = x.contiguous().float(), o.contiguous().float(), _w(scale)
        B, C = x.shape[:2]
        L = x.shape[2:].numel()                                                 # (not x[0, 0].numel(): an empty batch has no x[0])
        out = torch.empty_like(x)
        _launch(x.device, "wm_scale_add_fwd", x, sc, o, out, B, C, L)
        ctx.save_for_backward(x, sc)
        ctx.scale_shape = scale.shape
        return out

    @staticmethod
    def backward(ctx, g):
        x, sc = ctx.saved_tensors
        g = g.contiguous().float()
        B, C = x.shape[:2]
        L = x.shape[2:].numel()
        if _DETERMINISTIC:
            gx, gs = torch.empty_like(x), torch.empty(C, dtype=torch.float32, device=x.device)
            nb = _lib.load().wm_scale_add_bwd_det_workspace_bytes(B, C, L)
            _launch(x.device, "wm_scale_add_bwd_det", g, x, sc, gx, gs, _det_workspace(nb, x.device), nb, B, C, L)
            return gx, gs.view(ctx.scale_shape), g
        gx, gs = torch.empty_like(x), _zeros_small(C, x.device)
        _launch(x.device, "wm_scale_add_bwd", g, x, sc, gx, gs, B, C, L)
        return gx, gs.view(ctx.scale_shape), g


def scale_add_supported(x, scale, o):
    """Operands _ScaleAdd covers: (B, C, H, W) x and o of one shape, a C-element scale, B C <= 65535 (the planes are a grid
    dimension of wm_scale_add_fwd / _bwd)."""
    return (x.is_cuda and x.dim() == 4 and x.shape == o.shape and scale.numel() == x.shape[1]
            and x.shape[0] * x.shape[1] <= 65535)


def scale_add(x, scale, o):
    """x * scale.view(1, C, 1, 1) + o for (B, C, H, W) fp32 tensors and a C-element scale, differentiable."""
    _require_cuda("scale_add", x, scale, o)
    if not scale_add_supported(x, scale, o):
        raise NotImplementedError("scale_add: (B, C, H, W) operands with B C <= 65535 and a C-element scale")
    return _ScaleAdd.apply(x, scale, o)


# ------------------------------------------------------------------------------------------------
# depth-wise 3x3 convolution (+ bias, + SiLU) - inference path of SS2D.conv2d / ffn.conv2
# ------------------------------------------------------------------------------------------------
def dwconv3x3_supported(x):
    """Maps the module path (a depth-wise nn.Conv2d of the network: dwconv3x3, or dwconv3x3_train under autograd) takes: fp32
    on the GPU.  dwconv3x3 itself also serves the bf16-storage planes that lfss_block_forward hands it; a module never sees those."""
    return x.is_cuda and x.dtype == torch.float32


def dwconv3x3(x, weight, bias=None, act="none", flip=False):
    """F.conv2d(x, weight, bias, stride=1, padding=1, groups=C) [+ SiLU / exact GELU when act == 'silu' / 'gelu'] for a
    (C, 1, 3, 3) weight, NCHW fp32 (or bf16 planes: fp32 arithmetic, bf16 storage), forward only (no autograd graph is
    recorded).  flip: with weight.flip(2, 3) - the convolution's input gradient - read from `weight` itself."""
    _require_cuda("dwconv3x3", x, weight, bias)
    B, C, H, W = x.shape
    if weight.shape != (C, 1, 3, 3):
        raise RuntimeError(f"dwconv3x3: weight must be ({C}, 1, 3, 3), got {tuple(weight.shape)}")
    code = _dtype_code(x, "dwconv3x3")
    x = x.contiguous()
    y = torch.empty_like(x)
    _launch(x.device, "wm_dwconv3x3_fwd", x, _w(weight), None if bias is None else _w(bias), y,
            B, C, H, W, {"none": 0, "silu": 1, "gelu": 2}[act] + (4 if flip else 0), code)
    return y


def image_pre_u8(img, window_size=128, swap_rb=True):
    """(h, w, 3) uint8 device image -> (1, 3, Hp, Wp) fp32 in [0, 1], channel-major, reflect-padded to multiples of
    `window_size` (inference_wavemamba.py:99-105 + :28-36); swap_rb: BGR (cv2) -> RGB."""
    _require_cuda("image_pre_u8", img)
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        raise RuntimeError(f"image_pre_u8: expected (h, w, 3) uint8, got {tuple(img.shape)} {img.dtype}")
    h, w = img.shape[:2]
    Hp, Wp = h + (window_size - h % window_size) % window_size, w + (window_size - w % window_size) % window_size
    out = torch.empty((1, 3, Hp, Wp), dtype=torch.float32, device=img.device)
    _launch(img.device, "wm_image_pre_u8", img.contiguous(), out, h, w, Hp, Wp, int(bool(swap_rb)))
    return out


def image_post_u8(t, h, w, swap_rb=True):
    """(1, 3, Hp, Wp) fp32 -> (h, w, 3) uint8: crop, clamp [0, 1], * 255, round half to even, channel-last
    (inference_wavemamba.py:112-113 + tensor2img, img_util.py:67-94); swap_rb: RGB -> BGR."""
    _require_cuda("image_post_u8", t)
    if t.dtype != torch.float32 or t.dim() != 4 or t.shape[0] != 1 or t.shape[1] != 3:
        raise RuntimeError(f"image_post_u8: expected (1, 3, Hp, Wp) float32, got {tuple(t.shape)} {t.dtype}")
    Hp, Wp = t.shape[2:]
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=t.device)
    _launch(t.device, "wm_image_post_u8", t.contiguous(), out, h, w, Hp, Wp, int(bool(swap_rb)))
    return out


IMAGES_IO_TILE = 32                        # csrc/images_io.hip.h: IO_TILE - one workgroup per 32 x 32 tile (the tests' edge shapes)
IMAGES_PRE_WORDS, IMAGES_POST_WORDS = 4, 12      # IO_PRE_WORDS, IO_POST_WORDS: int64 per row
_IMAGES_TURN = (False, False, True, True, False, False, True, True)    # modes 2, 3, 6, 7 turn (h, w) into (w, h)


class ImagesTable:
    """One device table of images_io_table: `rows` (n, words) int64 on the device; pre: the padded shape (H, W) every row gives;
    post: the largest destination (H, W) and, per source tensor, (images, rows, columns) it must at least hold (`need`).
    `keep` holds the tensors whose addresses the table names, so they live as long as the table does."""

    def __init__(self, kind, rows, n, H, W, need, keep):
        self.kind, self.rows, self.n, self.H, self.W, self.need, self.keep = kind, rows, n, H, W, need, keep


def _images_u8(name, t, dev):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3 and t.is_contiguous()):
        what = f"{tuple(t.shape)} {t.dtype} on {t.device}, contiguous: {t.is_contiguous()}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"images_io_table: {name} must be a contiguous (h, w, 3) uint8 CUDA tensor, got {what}")
    if t.shape[0] < 1 or t.shape[1] < 1:
        raise RuntimeError(f"images_io_table: {name} is empty: {tuple(t.shape)}")
    if dev is not None and t.device != dev:
        raise RuntimeError(f"images_io_table: the images live on more than one device ({dev}, {t.device})")
    return t.device


def images_io_table(pre=None, post=None, window_size=128):
    """The device tables wm_images_pre_u8 and wm_images_post_u8 read (include/wavemamba_hip.h) -> (pre table, post table), each
    an ImagesTable, or None for a list not given.
    pre: [(image, mode), ...] - contiguous (h, w, 3) uint8 CUDA images and modes 0..7 of data_augmentation; image n of the launch's
    output is reflect_pad(chw(mode(image)) / 255), padded bottom / right to multiples of window_size AFTER the transform.  Every row
    must pad to the same (Hp, Wp), and a padding that reaches the transformed image's size raises RuntimeError, as F.pad(...,
    'reflect') does.
    post: [(image, [(tensor, index, mode), ...]), ...] - contiguous (h, w, 3) uint8 CUDA destinations, each the mean of k = 1 or 8
    sources in the order given: image `index` of source tensor 0 or 1 of the launch, which holds the network's result on the
    destination-shaped image transformed by `mode`.
    Like grad_guard_table the tables are built OUTSIDE a graph capture (RuntimeError inside one) and hold raw addresses: the images
    are kept alive by the table (ImagesTable.keep) and must stay in place, and a graph that captured a launch on a table needs the
    table for as long as it is replayed."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("images_io_table: a host-to-device copy must not be captured - build the tables before the capture")
    window = int(window_size)
    if window < 1:
        raise RuntimeError(f"images_io_table: window_size must be positive, got {window_size}")
    dev = None
    pre_rows, post_rows, shapes = [], [], set()
    for n, (img, mode) in enumerate(pre or ()):
        dev = _images_u8(f"pre image {n}", img, dev)
        if not (isinstance(mode, int) and 0 <= mode <= 7):
            raise RuntimeError(f"images_io_table: pre row {n}: mode must be 0..7, got {mode!r}")
        h, w = img.shape[:2]
        ht, wt = (w, h) if _IMAGES_TURN[mode] else (h, w)
        Hp, Wp = ht + (window - ht % window) % window, wt + (window - wt % window) % window
        if Hp - ht >= ht or Wp - wt >= wt:
            raise RuntimeError(f"images_io_table: pre row {n}: the reflect padding of a {ht} x {wt} image (mode {mode}) to {Hp} x {Wp} "
                               "reaches the image's size")
        shapes.add((Hp, Wp))
        pre_rows.append((img.data_ptr(), h, w, mode))
    if len(shapes) > 1:
        raise RuntimeError(f"images_io_table: the pre rows pad to different shapes {sorted(shapes)}: one launch writes one (N, 3, Hp, Wp)")
    need = [[0, 0, 0], [0, 0, 0]]
    hmax = wmax = 0
    for n, (img, srcs) in enumerate(post or ()):
        dev = _images_u8(f"post image {n}", img, dev)
        srcs = list(srcs)
        if len(srcs) not in (1, 8):
            raise RuntimeError(f"images_io_table: post row {n}: 1 or 8 sources, got {len(srcs)}")
        h, w = img.shape[:2]
        hmax, wmax = max(hmax, h), max(wmax, w)
        words = []
        for which, index, mode in srcs:
            if which not in (0, 1) or not (isinstance(mode, int) and 0 <= mode <= 7) or not 0 <= index < (1 << 31):
                raise RuntimeError(f"images_io_table: post row {n}: a source is (tensor 0 or 1, index >= 0, mode 0..7), got {(which, index, mode)}")
            ht, wt = (w, h) if _IMAGES_TURN[mode] else (h, w)
            need[which] = [max(need[which][0], index + 1), max(need[which][1], ht), max(need[which][2], wt)]
            words.append(mode | which << 8 | index << 16)
        post_rows.append((img.data_ptr(), h, w, len(srcs)) + tuple(words) + (0,) * (8 - len(words)))
    up = _GUARD_UPLOADS.setdefault(dev.index, _GuardTableUpload()) if dev is not None else None
    pre_t = post_t = None
    if pre is not None:
        rows = up.upload(pre_rows, dev) if pre_rows else torch.empty((0, IMAGES_PRE_WORDS), dtype=torch.int64, device=dev or "cuda")
        Hp, Wp = next(iter(shapes)) if shapes else (0, 0)
        pre_t = ImagesTable("pre", rows, len(pre_rows), Hp, Wp, None, [img for img, _ in pre])
    if post is not None:
        rows = up.upload(post_rows, dev) if post_rows else torch.empty((0, IMAGES_POST_WORDS), dtype=torch.int64, device=dev or "cuda")
        post_t = ImagesTable("post", rows, len(post_rows), hmax, wmax, need, [img for img, _ in post])
    return pre_t, post_t


def images_pre_u8(table, N, Hp, Wp, swap_rb=True, out=None):
    """N uint8 device images -> (N, 3, Hp, Wp) fp32 in [0, 1] in one launch (wm_images_pre_u8): image n is the table's row n
    transformed by its mode, channel-major, / 255, reflect-padded after the transform; swap_rb: BGR -> RGB.  `table`: the pre table of
    images_io_table, whose rows give this N and (Hp, Wp).  `out`: a contiguous (N, 3, Hp, Wp) float32 tensor on the table's device
    to write into (a captured graph's static input), else a new one.  cpu_twin.images_pre_u8 states the same in plain PyTorch."""
    if not isinstance(table, ImagesTable) or table.kind != "pre":
        raise RuntimeError("images_pre_u8: expected the pre table of images_io_table")
    if (table.n, table.H, table.W) != (int(N), int(Hp), int(Wp)):
        raise RuntimeError(f"images_pre_u8: the table holds {table.n} images padded to {table.H} x {table.W}, not {N} of {Hp} x {Wp}")
    dev = table.rows.device
    if out is None:
        out = torch.empty((table.n, 3, table.H, table.W), dtype=torch.float32, device=dev)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != dev
          or tuple(out.shape) != (table.n, 3, table.H, table.W) or not out.is_contiguous()):
        raise RuntimeError(f"images_pre_u8: out must be a contiguous ({table.n}, 3, {table.H}, {table.W}) float32 tensor on {dev}, got "
                           + (f"{tuple(out.shape)} {out.dtype} on {out.device}" if isinstance(out, torch.Tensor) else type(out).__name__))
    _launch(dev, "wm_images_pre_u8", table.rows, out, table.n, table.H, table.W, int(bool(swap_rb)))
    return out


def images_post_u8(table, sources, swap_rb=True):
    """fp32 network outputs -> the table's uint8 destinations in one launch (wm_images_post_u8): per destination the fp32 mean of
    its k sources, each cropped to its transformed shape and turned back, summed in the row's order and times 1 / k; then clamp
    [0, 1], * 255, round half to even, channel-last; swap_rb: RGB -> BGR.  `table`: the post table of images_io_table; `sources`: one
    contiguous (N, 3, Hp, Wp) float32 CUDA tensor or a pair of them (tensor 0 and tensor 1 of the table's source triples).
    -> the destination images (the tensors the table was built on).  cpu_twin.images_post_u8 states the same in plain PyTorch."""
    if not isinstance(table, ImagesTable) or table.kind != "post":
        raise RuntimeError("images_post_u8: expected the post table of images_io_table")
    sources = (sources,) if isinstance(sources, torch.Tensor) else tuple(sources)
    if not 1 <= len(sources) <= 2:
        raise RuntimeError(f"images_post_u8: one or two source tensors, got {len(sources)}")
    _require_cuda("images_post_u8", *sources)
    dev = table.rows.device
    for i, t in enumerate(sources):
        if t.dtype != torch.float32 or t.dim() != 4 or t.shape[1] != 3 or not t.is_contiguous() or t.device != dev:
            raise RuntimeError(f"images_post_u8: source {i} must be a contiguous (N, 3, Hp, Wp) float32 tensor on {dev}, got "
                               f"{tuple(t.shape)} {t.dtype} on {t.device}")
    for i, (n, hn, wn) in enumerate(table.need):
        have = (sources[i].shape[0], sources[i].shape[2], sources[i].shape[3]) if i < len(sources) else (0, 0, 0)
        if n > have[0] or hn > have[1] or wn > have[2]:
            raise RuntimeError(f"images_post_u8: the table reads {n} images of at least {hn} x {wn} from source {i}, which "
                               + (f"is {tuple(sources[i].shape)}" if i < len(sources) else "was not given"))
    s0 = sources[0]
    s1 = sources[1] if len(sources) == 2 else None
    _launch(dev, "wm_images_post_u8", table.rows, s0, s0.shape[0], s0.shape[2], s0.shape[3],
            s1, 0 if s1 is None else s1.shape[0], 0 if s1 is None else s1.shape[2], 0 if s1 is None else s1.shape[3],
            table.n, table.H, table.W, int(bool(swap_rb)))
    return list(table.keep)


def paired_patches_u8(table, P, swap_rb=True, out=None):
    """A training batch from uint8 images resident on the device (wm_paired_patches_u8, include/wavemamba_hip.h): what the
    reference's PairedImageDataset train phase and default collate produce at scale 1, bit for bit, in one launch.
    table: (B, 8) int64 CUDA tensor, per sample (lq_ptr, gt_ptr, h, w, top, left, mode, reserved) - data.PairedPatchBatcher
    writes it, and whoever writes it keeps the images alive.  The KERNEL reads it: a captured launch sees the table's contents
    at replay time.  -> (lq, gt), each (B, 3, P, P) float32; `out=(lq, gt)` writes into the caller's tensors instead (contiguous
    float32 of that shape on the table's device - GraphedTrainStep.lq / .gt, say)."""
    _require_cuda("paired_patches_u8", table)
    if table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != 8 or not table.is_contiguous():
        raise RuntimeError(f"paired_patches_u8: expected a contiguous (B, 8) int64 table, got {tuple(table.shape)} {table.dtype}")
    B, P = table.shape[0], int(P)
    if out is None:
        lq = torch.empty((B, 3, P, P), dtype=torch.float32, device=table.device)
        gt = torch.empty_like(lq)
    else:
        lq, gt = out
        for name, t in (("lq", lq), ("gt", gt)):
            if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != table.device
                    or tuple(t.shape) != (B, 3, P, P) or not t.is_contiguous()):
                raise RuntimeError(f"paired_patches_u8: out {name} must be a contiguous ({B}, 3, {P}, {P}) float32 tensor on "
                                   f"{table.device}, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}"
                                   + (f" {t.dtype} on {t.device}, strides {t.stride()}" if isinstance(t, torch.Tensor) else ""))
    _launch(table.device, "wm_paired_patches_u8", table, lq, gt, B, P, int(bool(swap_rb)))
    return lq, gt


def _metric_images(name, layout, *imgs):
    """uint8 CUDA images (H, W, 3) / (N, H, W, 3) for layout 'HWC', (3, H, W) / (N, 3, H, W) for 'CHW', all of one shape and
    device -> (4-D views, N, H, W, element strides (n, h, w, channel) shared by all of them)."""
    if layout not in ("HWC", "CHW"):
        raise ValueError(f"{name}: layout must be 'HWC' or 'CHW', got {layout!r}")
    _require_cuda(name, *imgs)
    for t in imgs:
        if t.dtype != torch.uint8:
            raise RuntimeError(f"{name}: expected uint8 images, got {t.dtype}")
        if t.shape != imgs[0].shape:
            raise RuntimeError(f"{name}: image shapes differ: {tuple(imgs[0].shape)} vs {tuple(t.shape)}")
        if t.device != imgs[0].device:
            raise RuntimeError(f"{name}: images on different devices: {imgs[0].device} vs {t.device}")
    ch = 3 if layout == "HWC" else 1
    if imgs[0].dim() not in (3, 4) or imgs[0].shape[ch - 4] != 3:
        raise RuntimeError(f"{name}: expected {'(N, H, W, 3)' if layout == 'HWC' else '(N, 3, H, W)'} images, got {tuple(imgs[0].shape)}")
    v = [t if t.dim() == 4 else t.unsqueeze(0) for t in imgs]
    if any(t.stride() != v[0].stride() for t in v):
        v = [t.contiguous() for t in v]
    s = v[0].stride()
    if layout == "HWC":
        N, H, W, _ = v[0].shape
        strides = (s[0], s[1], s[2], s[3])
    else:
        N, _, H, W = v[0].shape
        strides = (s[0], s[2], s[3], s[1])
    return v, N, H, W, strides


def psnr_ssim_y(a, b, crop_border=1, layout="HWC", bgr=True):
    """Y-channel PSNR and SSIM of uint8 CUDA image pairs on the device (comput_psnr_ssim.calculate_psnr / calculate_ssim with
    test_y_channel=True, as inference_wavemamba.py:116-117 calls them; definition in include/wavemamba_hip.h).
    a, b: (N, H, W, 3) for layout 'HWC' or (N, 3, H, W) for 'CHW' (or one image without N); bgr: channel 0 is blue.
    -> (N, 2) float64 CUDA tensor of (PSNR in dB, SSIM) per image; PSNR is inf for identical Y planes.  No host synchronisation."""
    lib = _lib.load()
    (va, vb), N, H, W, st = _metric_images("psnr_ssim_y", layout, a, b)
    crop = int(crop_border)
    ws_bytes = lib.wm_psnr_ssim_y_workspace_bytes(N, H, W, crop)
    if ws_bytes == 0:
        raise RuntimeError(f"psnr_ssim_y: crop_border {crop} leaves nothing of a {H} x {W} image (needs 0 <= crop < min(H, W) / 2)")
    out = torch.empty((N, 2), dtype=torch.float64, device=va.device)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=va.device)
    _launch(va.device, "wm_psnr_ssim_y_u8", va, vb, *st, N, H, W, crop, int(bool(bgr)), out, ws, ws_bytes)
    return out


def y_channel_u8(img, layout="HWC", bgr=True):
    """The reference's to_y_channel (comput_psnr_ssim.py:374-385, BT.601 Y in [16, 235], bit for bit) of uint8 CUDA images:
    (N, H, W, 3) / (N, 3, H, W) -> (N, H, W) float32, or (H, W) for one image without N."""
    (v,), N, H, W, st = _metric_images("y_channel_u8", layout, img)
    y = torch.empty((N, H, W), dtype=torch.float32, device=v.device)
    _launch(v.device, "wm_y_channel_u8", v, *st, N, H, W, int(bool(bgr)), y)
    return y if img.dim() == 4 else y[0]


def match_index_supported(C, num_matches):
    """match_index keeps every one of the C channels: `num_matches` must not ask for a selection among them."""
    return num_matches is None or num_matches == -1 or num_matches >= C


def match_index(G, nx, ny):
    """Channel matching with every channel kept: (B, C) int32 index of the L2-nearest candidate channel from the
    Gram outputs of `gram(maps, candidates)` (argmin_j |x_c|^2 + |y_j|^2 - 2 x_c . y_j)."""
    _require_cuda("match_index", G, nx, ny)
    B, C = nx.shape
    idx = torch.empty((B, C), dtype=torch.int32, device=G.device)
    _launch(G.device, "wm_match_index", G.contiguous(), nx.contiguous(), ny.contiguous(), idx, B, C)
    return idx


def _attn_fold_channels_ok(C, heads):
    return C <= 64 and C % heads == 0


def attn_fold_supported(x, w_po, heads):
    """The folded attention serves the (B, C, H, W) map `x` (the values) with the 1x1 projection weight `w_po`: wm_attn_fold's
    C <= 64 channels in `heads` equal groups, and the 1x1 convolution kernel (conv2d) that applies the folded weight."""
    return _attn_fold_channels_ok(x.shape[1], heads) and conv2d_supported(x, w_po)


def attn_fold(G, nq, nk, temperature, w_po, batch, heads):
    """(batch, C, C) = w_po @ blockdiag_h softmax(G / (|q||k|) * temperature): the transposed attention folded into its
    1x1 output projection.  G (batch * heads, ch, ch), nq / nk (batch * heads, ch) squared norms."""
    _require_cuda("attn_fold", G, nq, nk, temperature, w_po)
    C = w_po.shape[0]
    if not _attn_fold_channels_ok(C, heads):
        raise NotImplementedError("attn_fold: C <= 64 channels in `heads` equal groups")
    out = torch.empty((batch, C, C), dtype=torch.float32, device=G.device)
    _launch(G.device, "wm_attn_fold", G.contiguous(), nq.contiguous(), nk.contiguous(), temperature.detach().contiguous(),
            w_po.detach().reshape(C, C).contiguous(), out, batch, C, heads)
    return out


def skff_supported(feats, w_du, prelu):
    """Inputs wm_skff_fwd covers: three fp32 (B, C <= 64, H, W) maps, a (d <= 16, C) squeeze weight, a one-element PReLU."""
    return (len(feats) == 3 and all(t.is_cuda and t.dtype == torch.float32 for t in feats) and feats[0].shape[1] <= 64
            and w_du.shape[0] <= 16 and prelu.numel() == 1)


def skff(x0, x1, x2, w_du, prelu, w_fc):
    """SKFF of three (B, C, H, W) sub-bands: w_du (d, C[, 1, 1]), prelu (1,), w_fc (3, C, d) -> (B, C, H, W)."""
    lib = _lib.load()
    _require_cuda("skff", x0, x1, x2, w_du, prelu, w_fc)
    B, C, H, W = x0.shape
    d = w_du.shape[0]
    if x1.shape != x0.shape or x2.shape != x0.shape or x0.dtype != torch.float32:
        raise RuntimeError("skff: three fp32 tensors of equal shape")
    if not skff_supported((x0, x1, x2), w_du, prelu):
        raise NotImplementedError("skff: C <= 64, d <= 16 and a one-element PReLU")
    x0, x1, x2 = x0.contiguous(), x1.contiguous(), x2.contiguous()
    out = torch.empty_like(x0)
    ws = torch.empty(lib.wm_skff_workspace_bytes(B, C), dtype=torch.uint8, device=x0.device)
    _launch(x0.device, "wm_skff_fwd", x0, x1, x2, w_du.detach().reshape(d, C).contiguous(), prelu.detach().contiguous(),
            w_fc.detach().reshape(3, C, d).contiguous(), out, ws, ws.numel(), B, C, d, H, W)
    return out


CONV3X3_AUTO, CONV3X3_FIRST_GEN, CONV3X3_WAVE_SPECIALISED = 0, 1, 2


def conv2d_select(mode=CONV3X3_AUTO):
    """Which 3x3 kernel serves `conv2d` / `conv2d_gated` (wm_conv2d_select): by problem size (default), always the
    first-generation kernel, or the persistent wave-specialised one wherever its limits allow.  Process-wide; the two
    kernels accumulate in the same order, so this never changes a result (tests assert bit-equality)."""
    check(_lib.load().wm_conv2d_select(int(mode)), "wm_conv2d_select")


_PREPARED_GENERATION = [0]


def prepared_generation():
    """How often conv2d_cache_clear has run: a graph captured at another count replays prepared weight copies that are gone."""
    return _PREPARED_GENERATION[0]


def conv2d_cache_clear():
    """Drop every prepared (bf16-split) weight copy.  The cache validates an entry by (object, data_ptr, _version); a
    write through `.data` (p.data.copy_(), basicsr-style EMA `.data.mul_().add_()`, weight surgery) does NOT bump the
    version counter, so code that updates weights that way must call this (WaveMamba.train() / .eval() / ._apply() and
    trainer.load_network do).  A captured forward holds the addresses of the copies it was captured with: every call here advances
    prepared_generation(), by which inference.GraphedForward and the graphed UInt8Pipeline drop their graphs."""
    _PREPARED_GENERATION[0] += 1
    _WFRAG_CACHE.clear()
    _CORE_PREP_CACHE.clear()                 # (the SS2D core's prepared parameters: same validation, same caveat)


def _conv2d_wfrag(weight, cache=True):
    """The prepared (bf16-split, fragment-ordered) copy of a (Cout, Cin, ks, ks) weight; rebuilt when the
    parameter is updated in place (`_version`) or re-allocated.  cache=False: a weight computed on the fly
    (the folded attention), prepared every time.  A cached copy built on another stream is waited for (event) and
    recorded on the using stream, so multi-stream serving never reads it before the preparation kernel has finished
    nor sees it freed under a pending launch."""
    frag = _WFRAG_CACHE.get((weight,)) if cache else None
    if frag is not None:
        return frag
    cout, cin, ks = weight.shape[0], weight.shape[1], weight.shape[2]
    frag = torch.empty(_lib.load().wm_conv2d_wfrag_bytes(cout, cin, ks), dtype=torch.uint8, device=weight.device)
    _launch(weight.device, "wm_conv2d_prep", weight.detach().contiguous(), frag, cout, cin, ks)
    if cache and not torch.cuda.is_current_stream_capturing():   # prepared inside a capture: part of the graph, not of the cache
        _WFRAG_CACHE.put((weight,), frag)
    return frag


def _conv_operands(name, expects, x, x2, x2_index, weights):
    """The input X of `conv2d` / `conv2d_gated` = x, cat([x, x2], 1) or cat([x, gather(x2, 1, x2_index)], 1), checked against
    the (Cout, Cin, ...) `weights` (all float32) -> (x, x2, int32 index, cb, cb_src), contiguous, for the kernels' argument lists:
    cb channels of X come from x2, which has cb_src."""
    B, Ca, H, W = x.shape
    cin = weights[0].shape[1]
    cb = cb_src = 0
    if x2 is not None:
        if (x2.shape[0], x2.shape[2], x2.shape[3]) != (B, H, W):
            raise RuntimeError(f"{name}: x2 {tuple(x2.shape)} does not match x {tuple(x.shape)}")
        cb_src = x2.shape[1]
        cb = cb_src if x2_index is None else x2_index.shape[1]
        if x2_index is not None and (x2_index.shape[0] != B or x2_index.dim() != 2):
            raise RuntimeError(f"{name}: x2_index must be (B, Cb), got {tuple(x2_index.shape)}")
    if cin != Ca + cb:
        raise RuntimeError(f"{name}: {expects} {cin} input channels, got {Ca} + {cb}")
    for t in (x, *weights, x2):
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError(f"{name}: float32 only")
    return (x.contiguous(), None if x2 is None else x2.contiguous(),
            None if x2_index is None else x2_index.to(torch.int32).contiguous(), cb, cb_src)


def conv2d(x, weight, bias=None, x2=None, x2_index=None, gate=None, residual=None, dynamic_weight=False):
    """y = F.conv2d(X, weight, bias, stride=1, padding=ks // 2) for a dense (Cout, Cin, ks, ks) weight, ks in
    {1, 3}, NCHW fp32, where X = x, or cat([x, x2], 1), or cat([x, gather(x2, 1, x2_index)], 1) with x2_index
    (B, Cb) channel indices into x2; then y *= sigmoid(gate) and y += residual when given.  Forward only (no
    autograd graph is recorded).  bf16 matrix cores with a two-term split of both operands: 3-4e-6 relative to
    the fp64 result.  dynamic_weight: `weight` is a freshly computed tensor (no prepared-copy cache)."""
    _require_cuda("conv2d", x, weight, bias, x2, x2_index, gate, residual)
    B, Ca, H, W = x.shape
    cout, ks = weight.shape[0], weight.shape[2]
    if weight.dim() != 4 or weight.shape[3] != ks or ks not in (1, 3):
        raise RuntimeError(f"conv2d: weight must be (Cout, Cin, ks, ks) with ks in (1, 3), got {tuple(weight.shape)}")
    x, x2, idx, cb, cb_src = _conv_operands("conv2d", "weight expects", x, x2, x2_index, (weight,))
    for t in (gate, residual):
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError("conv2d: float32 only")
    for t, name in ((gate, "gate"), (residual, "residual")):
        if t is not None and tuple(t.shape) != (B, cout, H, W):
            raise RuntimeError(f"conv2d: {name} must be {(B, cout, H, W)}, got {tuple(t.shape)}")
    gate = None if gate is None else gate.contiguous()
    residual = None if residual is None else residual.contiguous()
    frag = _conv2d_wfrag(weight, cache=not dynamic_weight)
    y = torch.empty((B, cout, H, W), dtype=torch.float32, device=x.device)
    _launch(x.device, "wm_conv2d_fwd", x, x2, idx, frag, None if bias is None else bias.detach().contiguous(), gate, residual, y,
            B, Ca, cb, cb_src, cout, H, W, ks)
    return y


_F16_WS = {}


def _f16_ws_bytes(lib, cout, cin, ks):
    key = (cout, cin, ks)
    n = _F16_WS.get(key)
    if n is None:
        f = int(lib.wm_conv2d_wfrag_bytes(cout, cin, ks))
        n = _F16_WS[key] = f + 256 if f else 0
    return n


def conv2d_f16(x, weight, bias=None, dgrad=False):
    """y = F.conv2d(x, weight, bias, stride=1, padding=ks // 2), ks in {1, 3}, NCHW fp32, on the fp16 matrix cores with a
    two-term split of both operands and per-tensor power-of-two scales (csrc/conv2d.hip.h): ~1e-7 relative to the fp64
    result - the training step's form (forward, and the input gradient on the transposed, flipped weight).  Four launches:
    memset + the two largest magnitudes, weight fragments, convolution; nothing synchronises the host.  Forward only.
    dgrad: `weight` is the (Cin, Cout, ks, ks) weight of the FORWARD convolution whose input gradient this call computes from
    x = gy: the convolution with weight.transpose(0, 1).flip(2, 3), whose fragments the library reads from `weight`
    itself (autograd's formula: a flip and a copy kernel per convolution and step)."""
    lib = _lib.load()
    _require_cuda("conv2d_f16", x, weight, bias)
    B, Cin, H, W = x.shape
    cout, cin, ks = weight.shape[0], weight.shape[1], weight.shape[2]
    if dgrad:
        cout, cin = cin, cout
    if weight.dim() != 4 or weight.shape[3] != ks or ks not in (1, 3) or cin != Cin:
        raise RuntimeError(f"conv2d_f16: weight {tuple(weight.shape)} does not fit x {tuple(x.shape)} (ks in (1, 3))")
    if x.dtype != torch.float32 or weight.dtype != torch.float32:
        raise RuntimeError("conv2d_f16: float32 only")
    x = x.contiguous()
    w = weight.detach().contiguous()
    nws = _f16_ws_bytes(lib, cout, cin, ks)
    if nws == 0:
        check(_lib.WM_EUNSUPPORTED, "wm_conv2d_f16_steps")
    # wm_conv2d_f16_steps: the two maxima in a slot of the zeroed arena (no memset node), magnitudes + fragments in one launch
    amax = _zeros_small(2, x.device)
    wfrag = torch.empty(nws - 256, dtype=torch.uint8, device=x.device)
    y = torch.empty((B, cout, H, W), dtype=torch.float32, device=x.device)
    b = None if bias is None else bias.detach().contiguous()
    _launch(x.device, "wm_conv2d_f16_steps", x, w, b, y, amax, wfrag, B, cin, cout, H, W, ks, 1 if dgrad else 0)
    return y


def conv2d_ln(x, ln_weight, ln_bias, ln_eps, weight, bias=None, residual=None):
    """conv1x1(LayerNorm2d(x)) + bias (+ residual) in one kernel (wm_conv2d_ln_fwd): x (B, 32, H, W) fp32, weight (Cout, 32, 1, 1).
    Bit-identical to layernorm2d() + conv2d().  Forward only."""
    _require_cuda("conv2d_ln", x, ln_weight, ln_bias, weight, bias, residual)
    B, C, H, W = x.shape
    cout = weight.shape[0]
    if C != 32 or tuple(weight.shape[1:]) != (32, 1, 1) or x.dtype != torch.float32:
        raise NotImplementedError("conv2d_ln: fp32, 32 input channels, 1x1 weight")
    if residual is not None and tuple(residual.shape) != (B, cout, H, W):
        raise RuntimeError(f"conv2d_ln: residual must be {(B, cout, H, W)}, got {tuple(residual.shape)}")
    x = x.contiguous()
    frag = _conv2d_wfrag(weight)
    y = torch.empty((B, cout, H, W), dtype=torch.float32, device=x.device)
    _launch(x.device, "wm_conv2d_ln_fwd", x, _w(ln_weight), _w(ln_bias), float(ln_eps), frag,
            None if bias is None else bias.detach().contiguous(), None if residual is None else residual.contiguous(), y,
            B, C, cout, H, W)
    return y


_FUSE_LN_CONV = True      # False (tests / tools): LayerNorm2d and the 1x1 convolution as two launches


# A depth-wise 3x3 whose only reader is a 1x1 convolution, as ONE kernel (wm_dwconv_conv1x1_fwd: the plane between them never
# reaches HBM, 256 of the pair's 640 B per position; bit-identical).  False (tests / tools): the two launches.
_FUSE_DW_PW = True
# The maps the HFE branch sends to it: at least as many positions PER IMAGE as the smallest UHD level at which the fused call
# measured faster than the pair - level 3, the smallest level there is: nothing below it is measured, so nothing smaller takes it -
# and inside the entry's offset range (H W < 2^26).  Per call, pair -> fused, median of 7 x 20 calls with [slowest fused, fastest
# pair] (tools/bench_dw_pw.py, profiles/dw_pw/per_call.txt).  ffn tail: dwconv3x3(GELU) + conv1x1(+ residual) -> the fused call;
# value path: dwconv3x3 over 96 channels + conv1x1(v, + residual) -> dwconv3x3 over the 64 q | k channels + the fused call:
#   UHD level 1 (1088 x 1920)  ffn 0.287 -> 0.179 ms [0.191, 0.286]   value 0.498 -> 0.397 ms [0.398, 0.498]
#   UHD level 2 ( 544 x  960)  ffn 0.075 -> 0.043 ms [0.043, 0.074]   value 0.137 -> 0.111 ms [0.112, 0.136]
#   UHD level 3 ( 272 x  480)  ffn 0.029 -> 0.019 ms [0.019, 0.029]   value 0.037 -> 0.029 ms [0.030, 0.037]
_FUSE_DW_PW_MIN_POSITIONS = 272 * 480


def _fuse_dw_pw_map(B, H, W):
    """Maps on which the HFE branch takes dwconv_conv1x1: inside the entry's offset range and, per image, at least as large as the
    smallest map at which it measured faster than the pair."""
    return _FUSE_DW_PW and B > 0 and _FUSE_DW_PW_MIN_POSITIONS <= H * W < (1 << 26)


def dwconv_conv1x1_supported(x, dw_weight, weight):
    """Operands wm_dwconv_conv1x1_fwd covers: fp32 on the GPU, 32 -> 32 channels, a (32, 1, 3, 3) depth-wise weight."""
    return (x.is_cuda and x.dim() == 4 and x.shape[1] == 32 and tuple(dw_weight.shape) == (32, 1, 3, 3)
            and tuple(weight.shape) == (32, 32, 1, 1) and all(t.dtype == torch.float32 for t in (x, dw_weight, weight)))


def dwconv_conv1x1(x, dw_weight, dw_bias, act, weight, bias=None, residual=None, dynamic_weight=False):
    """F.conv2d(act(F.conv2d(x, dw_weight, dw_bias, padding=1, groups=32)), weight, bias) (+ residual) in one kernel
    (wm_dwconv_conv1x1_fwd), act in ('none', 'gelu'): x (B, 32, H, W) fp32 - a channel slice of a wider contiguous tensor is read in
    place -, dw_weight (32, 1, 3, 3), weight (32, 32, 1, 1).  Bit-identical to conv2d(dwconv3x3(x, ...), ...).  Forward only.
    dynamic_weight: `weight` is a freshly computed tensor (no prepared-copy cache)."""
    _require_cuda("dwconv_conv1x1", x, dw_weight, dw_bias, weight, bias, residual)
    if not dwconv_conv1x1_supported(x, dw_weight, weight):
        raise NotImplementedError("dwconv_conv1x1: fp32, 32 -> 32 channels, (32, 1, 3, 3) depth-wise and (32, 32, 1, 1) dense weights")
    if act not in ("none", "gelu"):
        raise ValueError(f"dwconv_conv1x1: act must be 'none' or 'gelu', got {act!r}")
    B, C, H, W = x.shape
    if residual is not None and (tuple(residual.shape) != (B, 32, H, W) or residual.dtype != torch.float32):
        raise RuntimeError(f"dwconv_conv1x1: residual must be float32 {(B, 32, H, W)}, got {tuple(residual.shape)}")
    if tuple(x.stride()[1:]) != (H * W, W, 1) or (B > 1 and x.stride(0) < C * H * W):
        x = x.contiguous()                                         # planes (H, W) back to back; any batch stride beyond them
    frag = _conv2d_wfrag(weight, cache=not dynamic_weight)
    y = torch.empty((B, 32, H, W), dtype=torch.float32, device=x.device)
    _launch(x.device, "wm_dwconv_conv1x1_fwd", x, x.stride(0) if B > 1 else C * H * W, _w(dw_weight),
            None if dw_bias is None else _w(dw_bias), {"none": 0, "gelu": 2}[act], frag,
            None if bias is None else bias.detach().contiguous(), None if residual is None else residual.contiguous(), y,
            B, C, 32, H, W)
    return y


# LayerNorm2d -> 1x1 -> the depth-wise 3x3 that alone reads the 1x1's first channels, as ONE kernel (wm_ln_conv1x1_dwconv_fwd: the plane
# between the 1x1 and the depth-wise conv never reaches HBM; bit-identical): the two heads of an HFE block - "qkv" (32 -> 96, the
# depth-wise conv on the 64 q | k channels, 512 of the pair's 1024 B per position) and "project_in" (32 -> 32, 256 of 512 B).
# False (tests / tools): wm_conv2d_ln_fwd + wm_dwconv3x3_fwd.
_FUSE_PW_DW = True
# One floor per head: the positions PER IMAGE of the smallest UHD level at which that head's fused call measured faster than the pair
# (its slowest repetition below the pair's fastest) - never below level 3, the smallest level there is: nothing below it is measured,
# so nothing smaller takes the fused call.  Per call, pair -> fused, median of 7 x 20 alternating calls with [slowest fused, fastest
# pair] (tools/bench_hfe_heads.py, profiles/hfe_heads/per_call.txt):
#   UHD level 1 (1088 x 1920)  qkv 0.518 -> 0.295 ms [0.300, 0.517]   project_in 0.242 -> 0.169 ms [0.176, 0.240]
#   UHD level 2 ( 544 x  960)  qkv 0.135 -> 0.090 ms [0.091, 0.134]   project_in 0.059 -> 0.043 ms [0.044, 0.059]
#   UHD level 3 ( 272 x  480)  qkv 0.034 -> 0.034 ms [0.036, 0.034]: no gain - the qkv head keeps the pair there
#                              project_in 0.025 -> 0.020 ms [0.021, 0.025]
_FUSE_PW_DW_MIN_POSITIONS = {"qkv": 544 * 960, "project_in": 272 * 480}
_PW_DW_HEADS = {"qkv": (96, 64), "project_in": (32, 32)}               # head -> (Cout, Cdw)


def _fuse_pw_dw_map(B, H, W, head):
    """Maps on which the HFE head `head` takes ln_conv1x1_dwconv: inside the entry's offset range (H W < 2^25) and, per image, at least
    as large as the smallest map at which it measured faster than the pair."""
    floor = _FUSE_PW_DW_MIN_POSITIONS[head]
    return bool(_FUSE_PW_DW and B > 0 and floor <= H * W < (1 << 25))


def ln_conv1x1_dwconv_supported(x, weight, dw_weight, n_dw):
    """Operands wm_ln_conv1x1_dwconv_fwd covers: fp32 on the GPU, 32 input channels, (Cout, channels under the depth-wise conv) one of
    the two HFE heads'.  Returns the head's name, or None."""
    if not (x.is_cuda and x.dim() == 4 and x.shape[1] == 32 and weight.dim() == 4 and tuple(weight.shape[1:]) == (32, 1, 1)
            and tuple(dw_weight.shape) == (n_dw, 1, 3, 3) and all(t.dtype == torch.float32 for t in (x, weight, dw_weight))):
        return None
    return next((h for h, form in _PW_DW_HEADS.items() if form == (weight.shape[0], n_dw)), None)


def ln_conv1x1_dwconv(x, ln_w, ln_b, eps, weight, bias, dw_weight, dw_bias, n_dw, band_rows=0):
    """y[:, :n_dw] = F.conv2d(pre, dw_weight, dw_bias, padding=1, groups=n_dw) of the first n_dw channels of pre = F.conv2d(LayerNorm2d(x),
    weight, bias), y[:, n_dw:] = pre[:, n_dw:], in one kernel (wm_ln_conv1x1_dwconv_fwd): x (B, 32, H, W) fp32, weight (Cout, 32, 1, 1),
    dw_weight (n_dw, 1, 3, 3), (Cout, n_dw) = (96, 64) or (32, 32).  Bit-identical to conv2d_ln() + dwconv3x3().  Forward only.
    band_rows: output rows per band of the kernel's row walk (0: the entry's choice)."""
    _require_cuda("ln_conv1x1_dwconv", x, ln_w, ln_b, weight, bias, dw_weight, dw_bias)
    if ln_conv1x1_dwconv_supported(x, weight, dw_weight, n_dw) is None:
        raise NotImplementedError("ln_conv1x1_dwconv: fp32, 32 input channels, (Cout, n_dw) = (96, 64) or (32, 32)")
    B, C, H, W = x.shape
    cout = weight.shape[0]
    x = x.contiguous()
    frag = _conv2d_wfrag(weight)
    y = torch.empty((B, cout, H, W), dtype=torch.float32, device=x.device)
    _launch(x.device, "wm_ln_conv1x1_dwconv_fwd", x, _w(ln_w), _w(ln_b), float(eps), frag,
            None if bias is None else bias.detach().contiguous(), _w(dw_weight), None if dw_bias is None else _w(dw_bias), y,
            B, C, cout, n_dw, H, W, int(band_rows))
    return y


# A 3x3 convolution whose only reader is the Haar analysis, as ONE kernel (wm_conv2d_dwt_fwd: the wave-specialised kernel forms the
# four sub-bands of each 2x2 quad in its epilogue, the full-resolution plane between the two - 128 B per position written and read
# back - never reaches HBM; bit-identical).  False (tests / tools): the two launches.
_FUSE_CONV_DWT = True
# UNet.conv_01 + down_group1's DWT take it per image (batch 1: the batch measured) from the smallest full-resolution map at which the
# fused call measured faster than the pair - the smaller of the two measured; nothing below it is measured, so nothing smaller takes
# it.  Per call, pair -> fused, median of 7 x 20 calls with [slowest fused, fastest pair] (tools/bench_fullres_ends.py,
# profiles/fullres_ends/per_call.txt):
#   2176 x 3840   0.663 -> 0.398 ms [0.399, 0.662]
#   1088 x 1920   0.188 -> 0.099 ms [0.101, 0.187]
_FUSE_CONV_DWT_MIN_POSITIONS = 1088 * 1920


def _fuse_conv_dwt_map(B, H, W):
    """Images whose conv_01 -> DWT pair runs as conv2d_dwt: batch 1 and at least as many positions as the smallest map at which it
    measured faster than the pair (the entry's own limits are in conv2d_dwt_supported)."""
    return _FUSE_CONV_DWT and B == 1 and H * W >= _FUSE_CONV_DWT_MIN_POSITIONS


def conv2d_dwt_supported(x, weight):
    """Operands wm_conv2d_dwt_fwd covers: fp32 on the GPU, a (32, Cin, 3, 3) weight, even H and W, a batch element of the input and
    of the 32-channel plane inside the wave-specialised kernel's 32-bit offsets."""
    return (x.is_cuda and x.dim() == 4 and weight.dim() == 4 and tuple(weight.shape) == (32, x.shape[1], 3, 3)
            and x.dtype == torch.float32 and weight.dtype == torch.float32 and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0
            and x.shape[0] <= 65535 and max(32, x.shape[1]) * x.shape[2] * x.shape[3] * 4 < 2 ** 32)


def conv2d_dwt(x, weight, bias=None):
    """dwt_init(F.conv2d(x, weight, bias, padding=1)) -> (ll, hl, lh, hh), each (B, 32, H / 2, W / 2), in one kernel
    (wm_conv2d_dwt_fwd): x (B, Cin, H, W) fp32, weight (32, Cin, 3, 3).  Bit-identical to dwt_init(conv2d(x, weight, bias)) - which
    is what runs while the first-generation 3x3 kernel is pinned (wm_conv2d_select(1), through conv2d_select or by the host itself:
    the entry then answers WM_EUNSUPPORTED, the form exists in the wave-specialised kernel only).  Forward only."""
    _require_cuda("conv2d_dwt", x, weight, bias)
    if not conv2d_dwt_supported(x, weight):
        raise NotImplementedError("conv2d_dwt: fp32, a (32, Cin, 3, 3) weight, even H and W, the wave-specialised 3x3 kernel's limits")
    B, Cin, H, W = x.shape
    x = x.contiguous()
    frag = _conv2d_wfrag(weight)
    outs = [torch.empty((B, 32, H // 2, W // 2), dtype=torch.float32, device=x.device) for _ in range(4)]
    rc = _launch(x.device, "wm_conv2d_dwt_fwd", x, frag, None if bias is None else bias.detach().contiguous(), *outs, B, Cin, 32, H, W,
                 WM_F32, status=True)
    if rc == _lib.WM_EUNSUPPORTED:                                 # (the operands are covered: the first-generation kernel is pinned)
        return dwt_init(conv2d(x, weight, bias))
    check(rc, "wm_conv2d_dwt_fwd")
    return tuple(outs)


# A Haar synthesis whose only reader is a 3x3 convolution, as ONE kernel (wm_idwt_conv2d_fwd: the producer waves of the
# wave-specialised kernel form the input tile from the four bands of each 2x2 quad; the full-resolution plane - 128 B per position
# written and read back - never reaches HBM; bit-identical).  False (tests / tools): the two launches.
_FUSE_IWT_CONV = True
# The last upFRG's IWT + UNet.last take it per image (batch 1: the batch measured) from the smallest full-resolution map at which the
# fused call measured faster than the pair - the smaller of the two measured.  Per call, pair -> fused, median of 7 x 20 calls with
# [slowest fused, fastest pair] (tools/bench_fullres_ends.py, profiles/fullres_ends/per_call.txt):
#   2176 x 3840   0.971 -> 0.704 ms [0.706, 0.970]
#   1088 x 1920   0.248 -> 0.179 ms [0.179, 0.248]
_FUSE_IWT_CONV_MIN_POSITIONS = 1088 * 1920


def _fuse_iwt_conv_map(B, H, W):
    """Images (B, H, W: the full-resolution output) whose IWT -> last pair runs as iwt_conv2d: batch 1 and at least as many positions as
    the smallest map at which it measured faster than the pair (the entry's own limits are in iwt_conv2d_supported)."""
    return _FUSE_IWT_CONV and B == 1 and H * W >= _FUSE_IWT_CONV_MIN_POSITIONS


def iwt_conv2d_supported(low, weight):
    """Operands wm_idwt_conv2d_fwd covers: a (B, 32, h, w) fp32 low band on the GPU (its high bands: (B, 96, h, w)), a (Cout, 32, 3, 3)
    weight, a batch element of the synthesised plane and of the output inside the wave-specialised kernel's 32-bit offsets."""
    return (low.is_cuda and low.dim() == 4 and low.shape[1] == 32 and weight.dim() == 4 and tuple(weight.shape[1:]) == (32, 3, 3)
            and low.dtype == torch.float32 and weight.dtype == torch.float32 and low.shape[0] <= 65535
            and max(32, weight.shape[0]) * low.shape[2] * low.shape[3] * 16 < 2 ** 32)


def iwt_conv2d(low, high, weight, bias=None, residual=None):
    """F.conv2d(iwt_init_pair(low, high), weight, bias, padding=1) (+ residual) in one kernel (wm_idwt_conv2d_fwd): low (B, 32, h, w),
    high (B, 96, h, w) fp32, weight (Cout, 32, 3, 3), residual (B, Cout, 2h, 2w) -> (B, Cout, 2h, 2w).  Bit-identical to
    conv2d(iwt_init_pair(low, high), weight, bias, residual=residual) - which is what runs while the first-generation 3x3 kernel is
    pinned (wm_conv2d_select(1): the entry then answers WM_EUNSUPPORTED).  Forward only."""
    _require_cuda("iwt_conv2d", low, high, weight, bias, residual)
    if not iwt_conv2d_supported(low, weight):
        raise NotImplementedError("iwt_conv2d: fp32, 32-channel bands, a (Cout, 32, 3, 3) weight, the wave-specialised 3x3 kernel's limits")
    B, C, h, w = low.shape
    cout = weight.shape[0]
    if tuple(high.shape) != (B, 3 * C, h, w) or high.dtype != torch.float32:
        raise RuntimeError(f"iwt_conv2d: high must be float32 {(B, 3 * C, h, w)}, got {tuple(high.shape)}")
    if residual is not None and (tuple(residual.shape) != (B, cout, 2 * h, 2 * w) or residual.dtype != torch.float32):
        raise RuntimeError(f"iwt_conv2d: residual must be float32 {(B, cout, 2 * h, 2 * w)}, got {tuple(residual.shape)}")
    frag = _conv2d_wfrag(weight)
    y = torch.empty((B, cout, 2 * h, 2 * w), dtype=torch.float32, device=low.device)
    rc = _launch(low.device, "wm_idwt_conv2d_fwd", low.contiguous(), high.contiguous(), frag,
                 None if bias is None else bias.detach().contiguous(), None if residual is None else residual.contiguous(), y,
                 B, C, cout, 2 * h, 2 * w, WM_F32, status=True)
    if rc == _lib.WM_EUNSUPPORTED:                                 # (the operands are covered: the first-generation kernel is pinned)
        return conv2d(iwt_init_pair(low, high), weight, bias, residual=residual)
    check(rc, "wm_idwt_conv2d_fwd")
    return y


def patchify_conv_supported(img, weight, r):
    """Shapes wm_patchify_conv_fwd covers: nn.PixelUnshuffle(r) + 1x1 nn.Conv2d on an fp32 NCHW image."""
    return (img.is_cuda and img.dtype == torch.float32 and img.dim() == 4 and weight.dim() == 4 and r in (2, 4, 8)
            and tuple(weight.shape[2:]) == (1, 1) and weight.shape[1] == img.shape[1] * r * r and weight.shape[0] in (16, 32, 48, 64)
            and img.shape[2] % r == 0 and img.shape[3] % r == 0 and weight.shape[0] * weight.shape[1] <= 16384)


def patchify_conv(img, weight, bias, r):
    """conv1x1(pixel_unshuffle(img, r)) (the UNet's ps_down1..3, reference wavemamba_arch.py:1014-1025 / :1043-1045) as one
    r x r / stride-r convolution read straight from the image: the unshuffled tensor is never materialised.  Forward only.
    img (B, Cin, H, W) fp32; weight (Cout, Cin r r, 1, 1); bias (Cout) or None -> (B, Cout, H / r, W / r) fp32."""
    _require_cuda("patchify_conv", img, weight)
    if not patchify_conv_supported(img, weight, r):
        raise ValueError("patchify_conv: unsupported shapes (see patchify_conv_supported)")
    img = img.contiguous()
    B, Cin, H, W = img.shape
    Cout = weight.shape[0]
    y = torch.empty((B, Cout, H // r, W // r), dtype=torch.float32, device=img.device)
    _launch(img.device, "wm_patchify_conv_fwd", img, _w(weight), None if bias is None else _w(bias), y, B, Cin, Cout, H, W, r)
    return y


def conv2d_ln_supported(x, weight):
    return (_FUSE_LN_CONV and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 32 and weight.dim() == 4
            and tuple(weight.shape[1:]) == (32, 1, 1) and x.shape[2] * x.shape[3] < 2 ** 31)


def conv2d_gated(x, weight3, weight1, bias1=None, x2=None, x2_index=None):
    """conv3x3(X; weight3) * sigmoid(conv1x1(X; weight1) + bias1) with X as in `conv2d` - PAConv's k3(x) * sigmoid(k2(x))
    (reference wavemamba_arch.py:694-697) in one kernel.  weight3 (Cout, Cin, 3, 3) without bias, weight1
    (Cout, Cin, 1, 1).  Forward only."""
    _require_cuda("conv2d_gated", x, weight3, weight1, bias1, x2, x2_index)
    B, Ca, H, W = x.shape
    cout, cin = weight3.shape[0], weight3.shape[1]
    if tuple(weight3.shape) != (cout, cin, 3, 3) or tuple(weight1.shape) != (cout, cin, 1, 1):
        raise RuntimeError(f"conv2d_gated: weights must be (Cout, Cin, 3, 3) and (Cout, Cin, 1, 1), got "
                           f"{tuple(weight3.shape)} and {tuple(weight1.shape)}")
    x, x2, idx, cb, cb_src = _conv_operands("conv2d_gated", "weights expect", x, x2, x2_index, (weight3, weight1))
    f3, f1 = _conv2d_wfrag(weight3), _conv2d_wfrag(weight1)
    y = torch.empty((B, cout, H, W), dtype=torch.float32, device=x.device)
    _launch(x.device, "wm_conv2d_gated_fwd", x, x2, idx, f3, f1, None if bias1 is None else bias1.detach().contiguous(), y,
            B, Ca, cb, cb_src, cout, H, W)
    return y


_LINEAR_WGRAD_SHAPES = {(128, 32), (32, 64), (64, 16), (16, 32), (32, 16), (16, 16), (64, 32), (32, 32), (16, 64)}


class _LinearNoBias(torch.autograd.Function):
    """F.linear(x, weight) for token tensors (..., I): ATen GEMMs for the output and the input gradient, the HIP MFMA
    reduction for the weight gradient (a (O, I) result with K = number of tokens)."""

    @staticmethod
    def forward(ctx, x, weight):
        ctx.save_for_backward(x, weight)
        return F.linear(x, weight)

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = gy.matmul(weight)
        if ctx.needs_input_grad[1]:
            O, I = weight.shape
            g2, x2 = gy.reshape(-1, O).contiguous().float(), x.reshape(-1, I).contiguous().float()
            if _DETERMINISTIC:
                gw = torch.empty(O, I, dtype=torch.float32, device=x.device)
                nb = _lib.load().wm_linear_wgrad_det_workspace_bytes(g2.shape[0], O, I)
                _launch(x.device, "wm_linear_wgrad_det", g2, x2, gw, _det_workspace(nb, x.device), nb, g2.shape[0], O, I)
                return gx, gw
            gw = _zeros_small(O * I, x.device).view(O, I)
            _launch(x.device, "wm_linear_wgrad", g2, x2, gw, g2.shape[0], O, I)
        return gx, gw


def linear_nobias_supported(x, weight):
    return (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32
            and tuple(weight.shape) in _LINEAR_WGRAD_SHAPES)


def linear_nobias(x, weight):
    """F.linear(x, weight) with the weight gradient on the HIP reduction kernel (training)."""
    _require_cuda("linear_nobias", x, weight)
    return _LinearNoBias.apply(x, weight)


class _ChannelGather(torch.autograd.Function):
    """y[b, j] = x[b, index[b, j]] over the channel axis of (B, C, ...) fp32 maps, index (B, M): wm_channel_gather_fwd, and for the
    gradient wm_channel_gather_bwd - every channel's sources added in ascending j, no atomics (ATen's scatter-add has no order)."""

    @staticmethod
    def forward(ctx, x, index):
        B, C = x.shape[:2]
        M = index.shape[1]
        HW = x[0, 0].numel() if B and C else 0
        idx = index.to(torch.int32).contiguous()
        y = torch.empty((B, M) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
        _launch(x.device, "wm_channel_gather_fwd", x, idx, y, B, C, M, HW)
        ctx.save_for_backward(idx)
        ctx.x_shape = tuple(x.shape)
        return y

    @staticmethod
    def backward(ctx, gy):
        idx, = ctx.saved_tensors
        B, C = ctx.x_shape[:2]
        M = idx.shape[1]
        gy = gy.contiguous().float()
        gx = torch.empty(ctx.x_shape, dtype=torch.float32, device=gy.device)
        _launch(gy.device, "wm_channel_gather_bwd", gy, idx, gx, B, C, M, gx[0, 0].numel() if B and C else 0)
        return gx, None


CHANNEL_GATHER_MAX_M = 1024                # csrc/det.hip.h: kGatherMaxM


def channel_gather_supported(x, index):
    """Operands _ChannelGather covers: a CUDA fp32 (B, C, ...) map with C >= 1, an integer (B, M) index, B, C, M within the grid."""
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() >= 3 and index.dim() == 2 and index.shape[0] == x.shape[0]
            and not index.dtype.is_floating_point and 1 <= x.shape[1] <= 65535 and x.shape[0] <= 65535
            and index.shape[1] <= CHANNEL_GATHER_MAX_M)


def channel_gather(x, index):
    """torch.gather(x, 1, index[:, :, None, ...].expand(...)) for x (B, C, *plane) and index (B, M) -> (B, M, *plane): the gathers of
    the HFE branch (Matching's matched maps, PAConv's second input).  CPU tensors take torch.gather (ordered there already); CUDA
    tensors the HIP kernels, whose gradient is bit-reproducible."""
    if not x.is_cuda:
        full = index.long().reshape(index.shape + (1,) * (x.dim() - 2)).expand(-1, -1, *x.shape[2:])
        return torch.gather(x, 1, full)
    _require_cuda("channel_gather", x, index)
    if not channel_gather_supported(x, index):
        raise NotImplementedError("channel_gather: a float32 (B, C, ...) map and an integer (B, M) index, M <= 1024")
    return _ChannelGather.apply(x.contiguous(), index)


def plane_sums(x):
    """x (B, C, H, W) fp32 -> (C,) sums over batch and plane (bias gradient of a convolution)."""
    _require_cuda("plane_sums", x)
    B, C, H, W = x.shape
    x = x.contiguous().float()
    if _DETERMINISTIC:
        out = torch.empty(C, dtype=torch.float32, device=x.device)
        nb = _lib.load().wm_plane_sums_det_workspace_bytes(B, C, H, W)
        _launch(x.device, "wm_plane_sums_det", x, out, _det_workspace(nb, x.device), nb, B, C, H, W)
        return out
    out = _zeros_small(C, x.device)
    _launch(x.device, "wm_plane_sums", x, out, B, C, H, W)
    return out


class _L1Mean(torch.autograd.Function):
    """mean |a - b| of two dense fp32 tensors of one shape (nn.L1Loss() and the reduction of FFTLoss, femasr_model.py:171-179;
    losses.py:306-313): forward and backward on the HIP kernels of loss.hip.h.  (ATen's reduction zeroes its semaphores with
    hipMemsetAsync - a memset node in a captured training step, which this runtime must not be given: the reported loss of a
    replay went wrong, profiles/r06/graph_memset_node.md.)"""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        if _DETERMINISTIC:
            out = torch.empty(1, dtype=torch.float32, device=a.device)
            nb = _lib.load().wm_l1_mean_fwd_det_workspace_bytes(a.numel())
            _launch(a.device, "wm_l1_mean_fwd_det", a, b, out, _det_workspace(nb, a.device), nb, a.numel())
            return out.reshape(())
        out = _zeros_small(1, a.device)
        _launch(a.device, "wm_l1_mean_fwd", a, b, out, a.numel())
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous().float()
        ga = torch.empty_like(a)
        _launch(a.device, "wm_l1_mean_bwd", a, b, g, ga, a.numel())
        return (ga if ctx.needs_input_grad[0] else None), (-ga if ctx.needs_input_grad[1] else None)


def l1_mean(a, b):
    """F.l1_loss(a, b) (mean reduction) for CUDA fp32 tensors of one shape, differentiable in both arguments."""
    _require_cuda("l1_mean", a, b)
    if a.shape != b.shape:
        raise RuntimeError(f"l1_mean: shapes differ: {tuple(a.shape)} vs {tuple(b.shape)}")
    if a.numel() == 0:
        raise RuntimeError("l1_mean: empty input")
    return _L1Mean.apply(a.contiguous().float(), b.contiguous().float())


GRAD_GUARD_CHUNK = 4096                    # csrc/grad_guard.hip.h: kGuardChunk - floats per table row (one workgroup each)


class _GuardTableUpload:
    """The two pinned slots (an event each) behind grad_guard_table, adamw_table and images_io_table, per device: PairedPatchBatcher's discipline - the host rewrites
    a slot only after the copy out of it has finished, so building the next step's table does not wait for this step's copy."""

    def __init__(self):
        self.pin, self.copied, self.slot = [None, None], [None, None], 0

    def upload(self, rows, dev):
        slot = self.slot
        self.slot ^= 1
        if self.copied[slot] is not None:
            self.copied[slot].synchronize()                        # the last copy out of this pinned slot
        width = len(rows[0])                                       # int64 words per row: 2 (grad_guard_table), 6 (adamw_table), 4 and 12 (images_io_table)
        words = len(rows) * width
        pin = self.pin[slot]
        if pin is None or pin.numel() < words:
            pin = self.pin[slot] = torch.empty(max(words, 2048), dtype=torch.int64, pin_memory=True)
        pin.numpy()[:words].reshape(len(rows), width)[:] = rows
        table = torch.empty((len(rows), width), dtype=torch.int64, device=dev)
        table.copy_(pin[:words].view(len(rows), width), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        self.copied[slot] = ev
        return table


_GUARD_UPLOADS = {}          # device index -> _GuardTableUpload


def grad_guard_table(tensors):
    """The device table wm_grad_guard reads, for a list of contiguous float32 CUDA tensors (one device): rows {address, count} of at
    most GRAD_GUARD_CHUNK floats, a tensor of more being split, an empty tensor giving no row; no row spans two tensors.
    -> (table (n_rows, 2) int64 on the device, n_rows).  The upload is a pinned-to-device copy on the current stream, so the table is
    always built OUTSIDE a graph capture (RuntimeError inside one); it holds raw addresses - the caller keeps the tensors alive and
    in place for as long as the table is used (a captured step: one flat gradient buffer, allocated before the capture), and a
    launch captured into a graph holds the address of the TABLE as well: keep the table for as long as the graph is replayed."""
    tensors = list(tensors)
    for t in tensors:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            what = f"{t.dtype} on {t.device}, contiguous: {t.is_contiguous()}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"grad_guard_table: contiguous float32 CUDA tensors only, got {what}")
    if len({t.device for t in tensors}) > 1:
        raise ValueError("grad_guard_table: the tensors live on more than one device")
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("grad_guard_table: a host-to-device copy must not be captured - build the table before the capture")
    dev = tensors[0].device if tensors else torch.device("cuda", torch.cuda.current_device())
    rows = []
    for t in tensors:
        base, n = t.data_ptr(), t.numel()
        rows.extend((base + 4 * at, min(GRAD_GUARD_CHUNK, n - at)) for at in range(0, n, GRAD_GUARD_CHUNK))
    if not rows:
        return torch.empty((0, 2), dtype=torch.int64, device=dev), 0
    up = _GUARD_UPLOADS.setdefault(dev.index, _GuardTableUpload())
    return up.upload(rows, dev), len(rows)


def grad_guard(tensors_or_table, max_norm=None, record=None, skipped=None, workspace=None):
    """The gradient norm, the non-finite flag and the clipping divisor of a set of gradients, on the device (wm_grad_guard: two
    launches, no atomics, no memset, no host read - bit-identical run to run and capturable).
    tensors_or_table: a list of contiguous float32 CUDA tensors (grad_guard_table is built here: not inside a capture), or the
    (table, n_rows) pair grad_guard_table returned.  max_norm: None for no clipping.  record (4 float32, overwritten with
    {norm, found_inf, grad_scale, 0}) and skipped (1 int64, += found_inf; False: no counter) are allocated when not given; `workspace` (uint8, at least
    wm_grad_guard_workspace_bytes(n_rows), contents irrelevant) likewise.  -> (record, skipped).
    cpu_twin.grad_guard states the same record in plain PyTorch."""
    if isinstance(tensors_or_table, tuple) and len(tensors_or_table) == 2 and isinstance(tensors_or_table[1], int):
        table, n_rows = tensors_or_table
    else:
        table, n_rows = grad_guard_table(tensors_or_table)
    if skipped is False:
        counter = None                                             # no counter: the entry point takes NULL
    else:
        counter = skipped
    _require_cuda("grad_guard", table, record, counter, workspace)
    if table.dtype != torch.int64 or not table.is_contiguous() or table.numel() < 2 * n_rows:
        raise ValueError("grad_guard: the table is (n_rows, 2) int64, contiguous")
    dev = table.device
    if record is None:
        record = torch.empty(4, dtype=torch.float32, device=dev)
    if skipped is None:
        counter = torch.zeros(1, dtype=torch.int64, device=dev)
    if record.dtype != torch.float32 or record.numel() < 4 or not record.is_contiguous():
        raise ValueError("grad_guard: record is 4 contiguous float32")
    if counter is not None and (counter.dtype != torch.int64 or counter.numel() < 1):
        raise ValueError("grad_guard: skipped is one int64")
    nb = _lib.load().wm_grad_guard_workspace_bytes(n_rows)
    if workspace is None:
        workspace = _det_workspace(nb, dev)
    ws_bytes = 0 if workspace is None else workspace.numel() * workspace.element_size()
    _launch(dev, "wm_grad_guard", table if n_rows else None, n_rows, 0.0 if max_norm is None else float(max_norm), record, counter,
            workspace, ws_bytes)
    return record, counter


ADAMW_ROW_WORDS = 6                        # csrc/adamw.hip.h: kAdamwRowWords - {param, grad, exp_avg, exp_avg_sq, ema or 0, count}


def adamw_table(params, grads, exp_avgs, exp_avg_sqs, emas=None):
    """The device table wm_adamw_step reads: for every parameter rows {param, grad, exp_avg, exp_avg_sq, ema or 0, count} of at most
    GRAD_GUARD_CHUNK floats (a tensor of more is split, an empty one gives no row; no row spans two tensors).  All five lists run
    in parallel over contiguous float32 CUDA tensors of one device, each quintuple of one size; `emas` is None (no averages) or
    holds None for a parameter that keeps none.  -> (table (n_rows, 6) int64 on the device, n_rows).  Like grad_guard_table the
    table is built OUTSIDE a graph capture, holds raw addresses - the caller keeps every tensor alive and in place - and must
    itself outlive a graph that captured a launch on it."""
    params, grads, exp_avgs, exp_avg_sqs = list(params), list(grads), list(exp_avgs), list(exp_avg_sqs)
    emas = [None] * len(params) if emas is None else list(emas)
    if not len(params) == len(grads) == len(exp_avgs) == len(exp_avg_sqs) == len(emas):
        raise ValueError("adamw_table: the lists differ in length")
    tensors = [t for group in (params, grads, exp_avgs, exp_avg_sqs, emas) for t in group if t is not None]
    for t in tensors:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            what = f"{t.dtype} on {t.device}, contiguous: {t.is_contiguous()}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"adamw_table: contiguous float32 CUDA tensors only, got {what}")
    if len({t.device for t in tensors}) > 1:
        raise ValueError("adamw_table: the tensors live on more than one device")
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("adamw_table: a host-to-device copy must not be captured - build the table before the capture")
    dev = tensors[0].device if tensors else torch.device("cuda", torch.cuda.current_device())
    rows = []
    for p, g, m, v, e in zip(params, grads, exp_avgs, exp_avg_sqs, emas):
        n = p.numel()
        if any(t.numel() != n for t in (g, m, v) + (() if e is None else (e,))):
            raise ValueError(f"adamw_table: a parameter of {n} floats with a gradient, moment or average of another size")
        bases = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr())
        eb = 0 if e is None else e.data_ptr()
        for at in range(0, n, GRAD_GUARD_CHUNK):
            rows.append(tuple(b + 4 * at for b in bases) + (eb + 4 * at if eb else 0, min(GRAD_GUARD_CHUNK, n - at)))
    if not rows:
        return torch.empty((0, ADAMW_ROW_WORDS), dtype=torch.int64, device=dev), 0
    up = _GUARD_UPLOADS.setdefault(dev.index, _GuardTableUpload())
    return up.upload(rows, dev), len(rows)


def adamw_step(table, lr, step, betas, eps, weight_decay, ema_decay=None, found_inf=None, grad_scale=None):
    """One AdamW step (torch.optim.AdamW, amsgrad=False, maximize=False) over the (table, n_rows) pair of adamw_table, with the
    moving average ema = d ema + (1 - d) p of the new weights for the rows that carry an ema address (wm_adamw_step: two launches,
    no atomics, no memset, no host read - bit-identical run to run and capturable).
    lr: one float32 on the device (a scheduler fills it in place); step: one float32 on the device, the steps taken so far, advanced
    by one here; betas, eps, weight_decay, ema_decay: Python floats - launch scalars, constants of a captured graph (a table built
    with `emas` needs an ema_decay: the table is not read back here to check).  found_inf /
    grad_scale: one float32 each on the device (GradGuard's record) or None: with found_inf != 0 nothing is written, the counter
    included; with grad_scale the update uses grad / grad_scale - the division is NOT written back: p.grad keeps the unclipped
    values (torch's fused AdamW stores them).  cpu_twin.adamw_step states the same update in plain PyTorch."""
    table, n_rows = table
    _require_cuda("adamw_step", table, lr, step, found_inf, grad_scale)
    if table.dtype != torch.int64 or not table.is_contiguous() or table.numel() < ADAMW_ROW_WORDS * n_rows:
        raise ValueError("adamw_step: the table is (n_rows, 6) int64, contiguous")
    for name, t in (("lr", lr), ("step", step), ("found_inf", found_inf), ("grad_scale", grad_scale)):
        if t is not None and (t.dtype != torch.float32 or t.numel() != 1):
            raise ValueError(f"adamw_step: {name} is one float32 on the device")
    hyper = (ctypes.c_double * 5)(float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                                  0.0 if ema_decay is None else float(ema_decay))
    _launch(table.device, "wm_adamw_step", table if n_rows else None, n_rows, lr, step, hyper, found_inf, grad_scale)


SSIM_TILE_H, SSIM_TILE_W = 24, 32         # csrc/ssim_loss.hip.h: SL_TH x SL_TW, one workgroup per tile (the tests' edge shapes)


def _ssim_forward(a, b, want_a, want_b):
    """wm_ssim_mean_fwd on dense fp32 (B, C, H, W): (ssim 0-dim, p1, p2, q, r) - the derivative maps only where wanted."""
    B, C, H, W = a.shape
    lib = _lib.load()
    ws_bytes = lib.wm_ssim_workspace_bytes(B * C, H, W)
    if ws_bytes == 0:
        raise RuntimeError(f"ssim_mean: {B * C} planes of {H} x {W} are more tiles than one launch holds (2^24 - 1)")
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=a.device)
    out = torch.empty(1, dtype=torch.float32, device=a.device)
    p1 = torch.empty_like(a) if want_a else None
    p2 = torch.empty_like(a) if want_b else None
    q, r = (torch.empty_like(a), torch.empty_like(a)) if want_a or want_b else (None, None)
    _launch(a.device, "wm_ssim_mean_fwd", a, b, out, p1, p2, q, r, ws, ws_bytes, B * C, H, W)
    return out.reshape(()), p1, p2, q, r


def _ssim_backward(x, other, p, q, r, g):
    B, C, H, W = x.shape
    gx = torch.empty_like(x)
    _launch(x.device, "wm_ssim_mean_bwd", x, other, p, q, r, g, gx, B * C, H, W)
    return gx


class _SSIMMean(torch.autograd.Function):
    """The mean SSIM of cal_ssim.py's SSIM() (femasr_model.py:29, :172) of two dense fp32 (B, C, H, W) tensors on the HIP kernels
    of ssim_loss.hip.h.  Forward: the tile kernel and the fixed-order sum (no ATen reduction: its semaphore memset must not be
    captured, see _L1Mean); where a gradient is wanted (want_a / want_b, decided by ssim_mean() - grad mode is off in here) the
    same pass stores dS/dmu, dS/de11, dS/de12, and backward is one filter kernel per gradient."""

    @staticmethod
    def forward(ctx, a, b, want_a, want_b):
        out, p1, p2, q, r = _ssim_forward(a, b, want_a, want_b)
        ctx.want = (want_a, want_b)
        ctx.save_for_backward(a, b, p1, p2, q, r)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b, p1, p2, q, r = ctx.saved_tensors
        g = g.contiguous().float()
        ga = _ssim_backward(a, b, p1, q, r, g) if ctx.want[0] and ctx.needs_input_grad[0] else None
        gb = _ssim_backward(b, a, p2, q, r, g) if ctx.want[1] and ctx.needs_input_grad[1] else None
        return ga, gb, None, None


def ssim_mean(img1, img2):
    """cal_ssim.SSIM()(img1, img2) (window 11, size_average) for CUDA tensors (B, C, H, W) of one shape: a 0-dim fp32 tensor,
    differentiable in both arguments.  The training loss is 1 - this (trainer.ssim_loss)."""
    _require_cuda("ssim_mean", img1, img2)
    if img1.dim() != 4 or img2.dim() != 4:
        raise RuntimeError(f"ssim_mean: expected (B, C, H, W) tensors, got {tuple(img1.shape)} and {tuple(img2.shape)}")
    if img1.shape != img2.shape:
        raise RuntimeError(f"ssim_mean: shapes differ: {tuple(img1.shape)} vs {tuple(img2.shape)}")
    if img1.numel() == 0:
        raise RuntimeError("ssim_mean: empty input")
    grad = torch.is_grad_enabled()
    return _SSIMMean.apply(img1.contiguous().float(), img2.contiguous().float(), grad and img1.requires_grad,
                           grad and img2.requires_grad)


FFT_L1_SIZE_RULE = "H and W powers of two in [16, 1024]"      # csrc/fft_loss.hip.h (wm_fft_l1_supported states it in the library)


def fft_l1_supported(H, W):
    """Whether the fused FFT loss has kernels for planes of H x W (the library's own answer: wm_fft_l1_supported)."""
    return bool(getattr(_lib.load(), "wm_fft_l1_supported")(int(H), int(W)))


def _fft_l1_sizes(planes, H, W):
    """(record bytes, workspace bytes) of the fused FFT loss; raises with the size rule where the library has no kernel."""
    lib = _lib.load()                      # (by name: tests/test_cabi.py lists the entry points this file may call as attributes)
    rec, ws = getattr(lib, "wm_fft_l1_record_bytes")(planes, H, W), lib.wm_fft_l1_workspace_bytes(planes, H, W)
    if rec == 0 or ws == 0:
        raise RuntimeError(f"fft_l1_mean: no kernel for {planes} planes of {H} x {W}: {FFT_L1_SIZE_RULE}, and at most 2^24 - 1 "
                           "workgroups in a launch")
    return rec, ws


def _fft_l1_forward(a, b, want):
    """wm_fft_l1_mean_fwd on dense fp32 (B, C, H, W): (loss 0-dim, record) - the record (a byte per spectrum bin: the signs) only
    where a gradient is wanted."""
    B, C, H, W = a.shape
    rec_bytes, ws_bytes = _fft_l1_sizes(B * C, H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=a.device)
    out = torch.empty(1, dtype=torch.float32, device=a.device)
    rec = torch.empty(rec_bytes, dtype=torch.uint8, device=a.device) if want else None
    _launch(a.device, "wm_fft_l1_mean_fwd", a, b, out, rec, ws, ws_bytes, B * C, H, W)
    return out.reshape(()), rec


def _fft_l1_backward(rec, g, shape, want_a, want_b):
    """wm_fft_l1_mean_bwd: (ga, gb), each only where wanted; gb = -ga comes out of the same launch."""
    B, C, H, W = shape
    _, ws_bytes = _fft_l1_sizes(B * C, H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=rec.device)
    ga = torch.empty(shape, dtype=torch.float32, device=rec.device) if want_a else None
    gb = torch.empty(shape, dtype=torch.float32, device=rec.device) if want_b else None
    _launch(rec.device, "wm_fft_l1_mean_bwd", rec, g, ga, gb, ws, ws_bytes, B * C, H, W)
    return ga, gb


class _FFTL1Mean(torch.autograd.Function):
    """FFTLoss (losses.py:300-313) of two dense fp32 (B, C, H, W) tensors on the HIP kernels of fft_loss.hip.h: one transform of
    a - b, the L1 mean of its half spectrum summed in a fixed order (bit-equal run to run in every mode, capturable).  Where a
    gradient is wanted (decided by fft_l1_mean() - grad mode is off in here) the forward keeps the signs of the spectrum, a byte
    per bin, and backward transforms them back: two launches for both gradients."""

    @staticmethod
    def forward(ctx, a, b, want_a, want_b):
        out, rec = _fft_l1_forward(a, b, want_a or want_b)
        ctx.want = (want_a, want_b)
        ctx.shape = tuple(a.shape)
        ctx.save_for_backward(rec)
        return out

    @staticmethod
    def backward(ctx, g):
        rec, = ctx.saved_tensors
        want_a, want_b = (ctx.want[i] and ctx.needs_input_grad[i] for i in (0, 1))
        if not (want_a or want_b):
            return None, None, None, None
        ga, gb = _fft_l1_backward(rec, g.contiguous().float(), ctx.shape, want_a, want_b)
        return ga, gb, None, None


def fft_l1_mean(pred, target):
    """FFTLoss()(pred, target) at loss_weight 1 (losses.py:300-313: the L1 mean between the stacked real / imaginary parts of the
    two rfft2) for CUDA tensors (B, C, H, W) of one shape, H and W powers of two in [16, 1024]: a 0-dim fp32 tensor, differentiable
    in both arguments.  The difference is taken first and transformed once (fft_loss.hip.h); cpu_twin.fft_l1_mean states the same."""
    _require_cuda("fft_l1_mean", pred, target)
    if pred.dim() != 4 or target.dim() != 4:
        raise RuntimeError(f"fft_l1_mean: expected (B, C, H, W) tensors, got {tuple(pred.shape)} and {tuple(target.shape)}")
    if pred.shape != target.shape:
        raise RuntimeError(f"fft_l1_mean: shapes differ: {tuple(pred.shape)} vs {tuple(target.shape)}")
    if pred.numel() == 0:
        raise RuntimeError("fft_l1_mean: empty input")
    if not fft_l1_supported(pred.shape[2], pred.shape[3]):
        raise RuntimeError(f"fft_l1_mean: no kernel for planes of {pred.shape[2]} x {pred.shape[3]}: {FFT_L1_SIZE_RULE}")
    grad = torch.is_grad_enabled()
    return _FFTL1Mean.apply(pred.contiguous().float(), target.contiguous().float(), grad and pred.requires_grad,
                            grad and target.requires_grad)


# Which code computes the FFT term of the training loss (trainer.fft_l1): "torch" - torch.fft.rfft2 of both images and ops.l1_mean
# over the spectra, as always - or "hip" - fft_l1_mean above, for the shapes it has kernels for.  Off ("torch") by default; WM_FFT_LOSS
# in the environment sets the initial value (read at import, like WM_TRAIN_CONV).  Read when the loss is CALLED: a graph captured
# under one backend replays that backend.
_FFT_LOSS_BACKENDS = ("torch", "hip")
_FFT_LOSS = os.environ.get("WM_FFT_LOSS", "torch")
if _FFT_LOSS not in _FFT_LOSS_BACKENDS:
    raise RuntimeError(f"WM_FFT_LOSS={_FFT_LOSS!r}: one of {_FFT_LOSS_BACKENDS}")


def set_fft_loss(backend):
    """Choose the FFT loss's backend, "torch" or "hip" (see above).  Returns the previous one."""
    global _FFT_LOSS
    if backend not in _FFT_LOSS_BACKENDS:
        raise ValueError(f"set_fft_loss: {backend!r} is not one of {_FFT_LOSS_BACKENDS}")
    prev, _FFT_LOSS = _FFT_LOSS, backend
    return prev


def fft_loss_backend():
    return _FFT_LOSS


class _Conv2dTrain(torch.autograd.Function):
    """Dense 3x3 / 1x1 convolution (stride 1, 'same' padding) for training: forward and input gradient on the
    matrix-core kernels (the input gradient is the same convolution with the weight transposed and flipped) - the fp16 form
    (f16, conv2d_f16) or the inference kernels' split-bf16 form; weight and bias gradients from _conv_weight_grad / plane_sums."""

    @staticmethod
    def forward(ctx, x, weight, bias, f16):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        ctx.f16 = f16
        if f16:
            return conv2d_f16(x.detach(), weight.detach(), None if bias is None else bias.detach())
        return conv2d(x.detach(), weight.detach(), None if bias is None else bias.detach())

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gy = gy.contiguous().float()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            if ctx.f16:
                gx = conv2d_f16(gy, weight, dgrad=True)                           # the transposed, flipped weight is never built
            else:
                wt = weight.detach().transpose(0, 1).flip(2, 3).contiguous()      # (Cin, Cout, ks, ks)
                gx = conv2d(gy, wt, None, dynamic_weight=True)
        gw, gb = _conv_param_grads(gy, x, weight, ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2])
        return gx, gw, gb, None


# Weight gradients of the dense convolutions in training: the HIP kernel (conv_wgrad.hip.h: K = positions on the bf16 matrix
# cores, split operands) instead of MIOpen's NHWC implicit-GEMM kernels and their layout transposes / hipBLASLt for 1x1.
# A leaf gradient - its ~4e-6 per product propagates nowhere.  set_train_conv_wgrad_hip(False) keeps ATen's.
_TRAIN_CONV_WGRAD_HIP = True


def set_train_conv_wgrad_hip(on):
    global _TRAIN_CONV_WGRAD_HIP
    prev, _TRAIN_CONV_WGRAD_HIP = _TRAIN_CONV_WGRAD_HIP, bool(on)
    return prev


def conv2d_wgrad_supported(x, weight):
    Cout, Cin, ks, ks2 = weight.shape
    return (x.is_cuda and x.dtype == torch.float32 and ks == ks2 and ks in (1, 3) and x.shape[3] % 32 == 0
            and (Cout + 15) // 16 in (1, 2, 4, 6) and not (ks == 3 and 64 < Cout <= 80))


def conv2d_wgrad(gy, x, ks, _refusal=RuntimeError, with_bias=False):
    """dW (Cout, Cin, ks, ks) of a stride-1 'same' convolution from gy (B, Cout, H, W) and x (B, Cin, H, W); with_bias: -> (dW, db),
    db (Cout) = gy summed over batch and plane, from the same pass over gy."""
    lib = _lib.load()
    _require_cuda("conv2d_wgrad", gy, x)
    if x.dim() != 4 or gy.dim() != 4 or gy.shape[0] != x.shape[0] or gy.shape[2:] != x.shape[2:]:
        raise _refusal(f"wm_conv2d_wgrad: gy {tuple(gy.shape)} does not match x {tuple(x.shape)}")
    B, Cout, H, W = gy.shape
    Cin = x.shape[1]
    gy = gy.contiguous().float(); x = x.contiguous().float()
    need = lib.wm_conv2d_wgrad_workspace_bytes(B, Cin, Cout, H, W, ks)
    if need == 0:
        raise _refusal("wm_conv2d_wgrad: unsupported shape (see conv2d_wgrad_supported)")
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    dW = torch.empty(Cout, Cin, ks, ks, dtype=torch.float32, device=x.device)
    db = torch.empty(Cout, dtype=torch.float32, device=x.device) if with_bias else None
    rc = _launch(x.device, "wm_conv2d_wgrad", gy, x, dW, db, ws, need, B, Cin, Cout, H, W, ks, status=True)
    if rc in (_lib.WM_EUNSUPPORTED, _lib.WM_EALIGN) and _refusal is not RuntimeError:
        raise _refusal(f"wm_conv2d_wgrad refused the call (code {rc})")
    check(rc, "wm_conv2d_wgrad")
    return (dW, db) if with_bias else dW


class _WgradRefused(RuntimeError):
    pass


def _conv_weight_grad(gy, x, weight, with_bias=False):
    """HIP matrix-core weight gradient, or ATen's for anything the kernel refuses - by the Python predicate, by
    wm_conv2d_wgrad_workspace_bytes (its shape limits) or by the call itself (WM_EUNSUPPORTED / WM_EALIGN): a training step
    never dies on a shape, as conv_wgrad.hip.h promises.  with_bias: -> (dW, db), the bias gradient from the same kernel (or
    plane_sums next to ATen's weight gradient)."""
    ks = weight.shape[2]
    if _DETERMINISTIC and _TRAIN_CONV_WGRAD_HIP and x.is_cuda and x.shape[3] % 32 != 0:
        # Deterministic mode: MIOpen's weight-gradient kernels are not ordered (measured: the 16-wide maps of a 64 x 64 crop, 39
        # weight tensors of the shipped network differing run to run), so maps the HIP kernel refuses for their width go to it
        # with gy and x zero-padded on the right to a multiple of 32 columns - the padded columns of gy contribute nothing and
        # those of x are the convolution's own zero padding: the same sums, added in the kernel's fixed order.
        pad = -x.shape[3] % 32
        xp, gp = F.pad(x.float(), (0, pad)), F.pad(gy.float(), (0, pad))
        if conv2d_wgrad_supported(xp, weight):
            try:
                return conv2d_wgrad(gp, xp, ks, _refusal=_WgradRefused, with_bias=with_bias)
            except _WgradRefused:
                pass
    if _TRAIN_CONV_WGRAD_HIP and conv2d_wgrad_supported(x, weight):
        try:
            return conv2d_wgrad(gy, x, ks, _refusal=_WgradRefused, with_bias=with_bias)
        except _WgradRefused:
            pass
    _, gw, _ = torch.ops.aten.convolution_backward(
        gy, x, weight, None, [1, 1], [ks // 2, ks // 2], [1, 1], False, [0, 0], 1, [False, True, False])
    return (gw, plane_sums(gy)) if with_bias else gw


def _conv_param_grads(gy, x, weight, want_w, want_b):
    """(dW, db) of a convolution's parameters, each None when not wanted: one kernel for both when both are."""
    if want_w and want_b:
        return _conv_weight_grad(gy, x, weight, with_bias=True)
    return (_conv_weight_grad(gy, x, weight) if want_w else None), (plane_sums(gy) if want_b else None)


class _Conv2dAten(torch.autograd.Function):
    """ATen's fp32 convolution (stride 1, 'same' padding) and input gradient, with the BIAS gradient on the HIP plane-sum
    kernel (autograd's own `grad_output.sum((0, 2, 3))` is ATen's generic strided reduction - 141 launches, 5.4 ms of a
    95-ms BASELINE config-3 training step, tools/train_breakdown.py) and the WEIGHT gradient on the HIP matrix-core
    kernel (`_conv_weight_grad`)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        return F.conv2d(x, weight, bias, stride=1, padding=weight.shape[2] // 2)

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gy = gy.contiguous()
        ks = weight.shape[2]
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx, _, _ = torch.ops.aten.convolution_backward(
                gy, x, weight, None, [1, 1], [ks // 2, ks // 2], [1, 1], False, [0, 0], 1, [True, False, False])
        gw, gb = _conv_param_grads(gy, x, weight, ctx.needs_input_grad[1], ctx.needs_input_grad[2])
        return gx, gw, gb


# Training convolutions (forward + input gradient; weight / bias gradients: _conv_weight_grad, plane_sums).  Modes:
#   "auto"    (default) per call, whichever of the next two is faster at that shape (tools/bench_conv_train.py on MI355X,
#             profiles/r04/bench_conv_train.txt): the fp16 form for 3x3 convolutions over >= 2^17 positions and 1x1 over >= 2^19
#             (BASELINE config 3's level-1 / level-2 and full-resolution maps: 3x3 64 -> 64 at 8 x 256 x 256 0.137 against
#             0.371 ms, 32 -> 96 0.130 / 0.306, 64 -> 64 at 128 x 128 0.066 / 0.099, 1x1 32 -> 64 0.066 / 0.119), ATen below that
#             (8 x 64 x 64 maps: three launches cost more than MIOpen's one: 0.055 against 0.032 ms);
#   "f16"     always the fp16 form of the matrix-core kernels: two-term split, per-tensor power-of-two scales - 22 significant
#             bits per operand, fp32-class (conv2d_f16): a training step without MIOpen / hipBLASLt in it;
#   "aten"    always ATen's fp32 convolutions (MIOpen Winograd / hipBLASLt): the mode of rounds 3-4a, kept as the cross-check;
#   "bf16x3"  the inference kernels' split-bf16 form: 16 significant bits per operand (3-4e-6 on an output) - right for
#             inference (the contract's bar is 1e-4 on outputs), but in the training step those 3e-6 on the activations become
#             ~1e-4 on the parameter gradients of the deepest block, whose 8 x 8 maps make every gradient a short cancelling sum
#             (tools/grad_localize.py: prediction 2.8e-6 / worst gradient tensor 1.1e-4 with it, 7.7e-8 / 1.4e-5 with fp32
#             convolutions; the reference's own fp32: 9.7e-8 / 6e-6).  Never the default.
# WM_TRAIN_CONV=<mode> in the environment, or set_train_conv_mode().
_TRAIN_CONV_MODES = ("auto", "f16", "aten", "bf16x3")
_TRAIN_CONV_MODE = os.environ.get("WM_TRAIN_CONV", "auto")
if _TRAIN_CONV_MODE not in _TRAIN_CONV_MODES:
    raise RuntimeError(f"WM_TRAIN_CONV={_TRAIN_CONV_MODE!r}: one of {_TRAIN_CONV_MODES}")


def set_train_conv_mode(mode):
    """Select how autograd's dense convolutions run (see above).  Returns the previous mode."""
    global _TRAIN_CONV_MODE
    if mode not in _TRAIN_CONV_MODES:
        raise ValueError(f"set_train_conv_mode: {mode!r} is not one of {_TRAIN_CONV_MODES}")
    prev, _TRAIN_CONV_MODE = _TRAIN_CONV_MODE, mode
    return prev


def train_conv_mode():
    return _TRAIN_CONV_MODE


def conv2d_train(x, weight, bias=None):
    """F.conv2d(x, weight, bias, stride=1, padding=ks // 2) with autograd, in the mode set_train_conv_mode() selects."""
    _require_cuda("conv2d_train", x, weight, bias)
    mode = _TRAIN_CONV_MODE
    if mode == "auto":
        mode = "f16" if x.shape[0] * x.shape[2] * x.shape[3] >= ((1 << 17) if weight.shape[2] == 3 else (1 << 19)) else "aten"
        if mode == "f16" and _f16_ws_bytes(_lib.load(), weight.shape[0], weight.shape[1], weight.shape[2]) == 0:
            mode = "aten"                        # a shape the fp16 kernels refuse: the step never dies on it
    if mode == "aten":
        if not ((bias is not None and bias.requires_grad) or weight.requires_grad):
            return F.conv2d(x.float(), weight, bias, stride=1, padding=weight.shape[2] // 2)
        return _Conv2dAten.apply(x.float(), weight, bias)
    return _Conv2dTrain.apply(x.contiguous().float(), weight, bias, mode == "f16")


def conv2d_supported(x, weight, x2=None):
    return (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and x.dim() == 4
            and weight.dim() == 4 and tuple(weight.shape[2:]) in ((3, 3), (1, 1)) and x.shape[2] * x.shape[3] < 2 ** 31
            and (x2 is None or (x.shape[1] % 8 == 0 and x2.dtype == torch.float32)))


# ------------------------------------------------------------------------------------------------
# profiling hooks (bench.py)
# ------------------------------------------------------------------------------------------------
PROF_KERNELS = ("haar_analysis", "haar_synthesis", "selscan_chunk_reduce", "selscan_carry",
                "selscan_chunk_scan", "lfss_in", "ss2d_proj", "dwconv3x3",
                "ss2d_core_scan", "lfss_mid", "ss2d_core_reduce", "lfss_out", "selscan_bwd",
                "conv3x3", "conv1x1", "skff", "layernorm2d", "dwconv3x3_other", "patchify_conv", "det_finish")


def prof_enable(on=True):
    """on: False/True (every kernel class) or an iterable of PROF_KERNELS names (only those classes)."""
    if on is True:
        mask = 0xFFFFFFFF
    elif not on:
        mask = 0
    else:
        mask = 0
        for name in on:
            mask |= 1 << PROF_KERNELS.index(name)
    _lib.load().wm_prof_enable(mask)


def prof_collect():
    """-> {kernel name: (launches, total_ms)} since prof_enable(True); blocks on the recorded events."""
    import ctypes
    lib = _lib.load()
    n = (ctypes.c_int * _lib.WM_PROF_NKERNELS)()
    ms = (ctypes.c_double * _lib.WM_PROF_NKERNELS)()
    check(lib.wm_prof_collect(n, ms), "wm_prof_collect")
    return {PROF_KERNELS[k]: (n[k], ms[k]) for k in range(_lib.WM_PROF_NKERNELS)}
