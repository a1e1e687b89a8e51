"""CPU twins of the hot-path operators of the drop-in boundary ("each with CPU + HIP implementations"; BASELINE config 1: the
LOLv1 / 1x3x256x256 "CPU-only PyTorch forward (plumbing, no GPU)").

    dwt_init            Haar analysis               /root/reference/basicsr/archs/wavemamba_arch.py:97-110
    iwt_init(_pair)     Haar synthesis              :113-130
    selective_scan_fn   the selective-scan operator :465-471 (mamba_ssm's published selective_scan_ref semantics)
    ss2d_core           SS2D.forward_core           :446-478 (for the torch.library op wavemamba_hip::ss2d_core on CPU tensors)
    paired_patches      the train phase of PairedImageDataset.__getitem__ after the decode + default collate
                        (/root/reference/basicsr/data/paired_image_dataset.py:80-131; host form of ops.paired_patches_u8)
    dihedral(_inverse)  the eight flips / rotations of data_augmentation (basicsr/data/transforms.py:223-268) and
                        what undoes them, as views
    images_pre_u8       N uint8 images, a mode each -> reflect_pad(chw(mode(img)) / 255), padded after the transform
                        (host form of ops.images_pre_u8; inference_wavemamba.py:28-36, :99-105 on the transformed image)
    images_post_u8      the fp32 mean of k network outputs turned back, quantised to uint8 (host form of ops.images_post_u8)
    grad_guard          gradient norm, non-finite flag and clipping divisor of the guarded optimizer step (no reference counterpart;
                        host form of ops.grad_guard)
    adamw_step          torch.optim.AdamW's single-tensor update plus the reference's model_ema (base_model.py:85-92; host form of
                        ops.adamw_step)

Plain PyTorch, differentiable by autograd, written from the operators' definitions.  They are
the implementation for CPU TENSORS and nothing else: `ops.py` selects them by the device of the input, never by the absence of
the HIP library - a CUDA (ROCm) tensor always runs the HIP kernels and raises when the library is missing
(tests/test_cabi.py::test_missing_library_fails_loudly, tests/test_cpu_twin.py::test_other_devices_never_reach_the_cpu_twins,
tests/test_gpu_parity.py::test_cuda_tensors_fail_loudly_without_the_library).
Nothing here imports `oracle/` (the C restatement the tests check BOTH implementations against), and bench.py /
__graft_entry__.smoke() never run it.  Speed is not a goal: the scan walks the sequence step by step.
"""
import torch
import torch.nn.functional as F


def _quads(x):
    """The four polyphase components of an even-sized NCHW map, each pre-divided by 2 (:98-103):
    a = x[2i, 2j], b = x[2i+1, 2j], c = x[2i, 2j+1], d = x[2i+1, 2j+1]."""
    if x.dim() != 4 or x.shape[2] % 2 or x.shape[3] % 2:
        raise RuntimeError(f"dwt_init: expected (B, C, H, W) with even H and W, got {tuple(x.shape)}")
    even_rows, odd_rows = x[:, :, 0::2, :] / 2, x[:, :, 1::2, :] / 2
    return even_rows[..., 0::2], odd_rows[..., 0::2], even_rows[..., 1::2], odd_rows[..., 1::2]


def dwt_init(x):
    """(LL, HL, LH, HH), each (B, C, H/2, W/2), dtype of x (:104-110)."""
    a, b, c, d = _quads(x)
    return a + b + c + d, -a - b + c + d, -a + b - c + d, a - b - c + d


def iwt_init(x):
    """(B, 4C, h, w) = [x1 | x2 | x3 | x4] channel blocks -> (B, C, 2h, 2w), always float32 (:113-130)."""
    if x.dim() != 4 or x.shape[1] % 4:
        raise RuntimeError(f"iwt_init: expected (B, 4C, h, w), got {tuple(x.shape)}")
    B, C4, h, w = x.shape
    C = C4 // 4
    x1, x2, x3, x4 = (x[:, i * C:(i + 1) * C].float() / 2 for i in range(4))
    out = torch.empty(B, C, 2 * h, 2 * w, dtype=torch.float32, device=x.device)
    out[:, :, 0::2, 0::2] = x1 - x2 - x3 + x4
    out[:, :, 1::2, 0::2] = x1 - x2 + x3 - x4
    out[:, :, 0::2, 1::2] = x1 + x2 - x3 - x4
    out[:, :, 1::2, 1::2] = x1 + x2 + x3 + x4
    return out


def iwt_init_pair(x_l, x_h):
    return iwt_init(torch.cat([x_l, x_h], dim=1))


def selective_scan_fn(u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, return_last_state=False):
    """h_t = exp(dt_t A) h_{t-1} + dt_t B_t u_t,  y_t = C_t . h_t + D u_t  (then y * silu(z)), dt = softplus(delta + bias) when
    delta_softplus.  u, delta (batch, dim, L); A (dim, N); B, C (batch, [G,] N, L) - the G groups split `dim` evenly; D, delta_bias
    (dim).  fp32 arithmetic, `out` in u's dtype; the fp32 last state (batch, dim, N) when return_last_state."""
    if u.dim() != 3 or delta.shape != u.shape or A.dim() != 2 or A.shape[0] != u.shape[1]:
        raise RuntimeError(f"selective_scan_fn: inconsistent shapes u {tuple(u.shape)}, delta {tuple(delta.shape)}, A {tuple(A.shape)}")
    batch, dim, L = u.shape
    N = A.shape[1]
    in_dtype = u.dtype
    u, dt, A = u.float(), delta.float(), A.float()
    if delta_bias is not None:
        dt = dt + delta_bias.float()[None, :, None]
    if delta_softplus:
        dt = F.softplus(dt)
    B4 = B.float() if B.dim() == 4 else B.float()[:, None]
    C4 = C.float() if C.dim() == 4 else C.float()[:, None]
    G = B4.shape[1]
    if B4.shape != (batch, G, N, L) or C4.shape != B4.shape or dim % G:
        raise RuntimeError(f"selective_scan_fn: B {tuple(B.shape)} / C {tuple(C.shape)} do not fit u {tuple(u.shape)}, A {tuple(A.shape)}")
    Bd = B4.repeat_interleave(dim // G, dim=1)               # (batch, dim, N, L): the group's B for each of its channels
    Cd = C4.repeat_interleave(dim // G, dim=1)
    h = u.new_zeros(batch, dim, N)
    ys = []
    for t in range(L):
        dt_t = dt[:, :, t, None]                             # (batch, dim, 1)
        h = torch.exp(dt_t * A) * h + (dt_t * u[:, :, t, None]) * Bd[:, :, :, t]
        ys.append((h * Cd[:, :, :, t]).sum(-1))
    y = torch.stack(ys, dim=-1) if ys else u.new_zeros(batch, dim, 0)
    if D is not None:
        y = y + u * D.float()[None, :, None]
    if z is not None:
        y = y * F.silu(z.float())
    y = y.to(in_dtype)
    return (y, h) if return_last_state else y


def ss2d_core(x, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds):
    """SS2D.forward_core (:446-478) on an NCHW map x (B, D, H, W): the four scan orders - row-major, column-major and their
    reversals (:451-452) - the per-direction projections x_dbl = x_proj_weight[k] . xs[k] -> (dt_r | B | C) and
    dts = dt_projs_weight[k] . dt_r (:453-455), one grouped selective scan (:465-471), and the four outputs brought back to
    row-major positions (:474-478).  Returns (y_row, y_row_reversed, y_col, y_col_reversed), each (B, D, H W) float32."""
    B, D, H, W = x.shape
    L = H * W
    K, N, R = 4, A_logs.shape[1], dt_projs_weight.shape[2]
    x = x.float()
    two = torch.stack([x.reshape(B, D, L), x.transpose(2, 3).reshape(B, D, L)], dim=1)
    xs = torch.cat([two, two.flip(-1)], dim=1)                                           # (B, 4, D, L)
    x_dbl = torch.einsum("bkdl,kcd->bkcl", xs, x_proj_weight.float())
    dt_r, Bs, Cs = torch.split(x_dbl, [R, N, N], dim=2)
    dts = torch.einsum("bkrl,kdr->bkdl", dt_r, dt_projs_weight.float())
    out = selective_scan_fn(xs.reshape(B, K * D, L), dts.reshape(B, K * D, L), -torch.exp(A_logs.float()), Bs, Cs, Ds.float(), None,
                            dt_projs_bias.float().reshape(-1), True).reshape(B, K, D, L)
    back = out[:, 2:4].flip(-1)
    to_rows = lambda t: t.reshape(B, D, W, H).transpose(2, 3).reshape(B, D, L)
    return out[:, 0], back[:, 0], to_rows(out[:, 1]), to_rows(back[:, 1])


def ssim_window_1d():
    """The 11-tap window of the SSIM training loss as cal_ssim.py builds it (gaussian(11, 1.5), :7-9): exp(-(i - 5)^2 / 4.5)
    evaluated and normalised in FLOAT32.  The float32 taps sum to 1 - 3.1e-8, and flat bright regions feel that (sigma^2 + C2
    is 9e-4 there, against a 2-D window sum that moves mu^2 by 7e-8), so the taps are kept exactly as the reference has them."""
    g = torch.tensor([-(i - 5) ** 2 / 4.5 for i in range(11)], dtype=torch.float64).exp().float()
    return g / g.sum()


def ssim_mean(img1, img2):
    """SSIM(window_size=11, size_average=True) of cal_ssim.py (:17-35, :39-64) for (B, C, H, W) tensors of any float dtype and
    device: the mean over every plane and pixel of
        S = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)),   C1 = 0.01^2, C2 = 0.03^2,
    the five moments taken with the zero-padded 11 x 11 Gaussian, here as a row pass and a column pass.  Evaluated in float64
    (as the HIP kernels accumulate: the reference's float32 loses e11 - mu1^2 on flat bright regions) and returned in the
    inputs' dtype; differentiable by autograd."""
    if img1.dim() != 4 or img1.shape != img2.shape:
        raise RuntimeError(f"ssim_mean: expected two (B, C, H, W) tensors of one shape, got {tuple(img1.shape)} and {tuple(img2.shape)}")
    if img1.numel() == 0:
        raise RuntimeError("ssim_mean: empty input")
    C = img1.shape[1]
    g = ssim_window_1d().to(device=img1.device, dtype=torch.float64)
    rows, cols = g.view(1, 1, 1, 11).repeat(C, 1, 1, 1), g.view(1, 1, 11, 1).repeat(C, 1, 1, 1)

    def blur(t):
        return F.conv2d(F.conv2d(t, rows, padding=(0, 5), groups=C), cols, padding=(5, 0), groups=C)
    a, b = img1.double(), img2.double()
    mu1, mu2 = blur(a), blur(b)
    s1, s2, s12 = blur(a * a) - mu1 * mu1, blur(b * b) - mu2 * mu2, blur(a * b) - mu1 * mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    s_map = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))
    return s_map.mean().to(img1.dtype)


def fft_l1_mean(pred, target):
    """FFTLoss at loss_weight 1 (losses.py:300-313: l1_loss between stack([rfft2(x).real, rfft2(x).imag]) of pred and of target)
    for (B, C, H, W) tensors of any float dtype, any H and W, stated as the HIP kernels compute it: rfft2 is linear, so the
    DIFFERENCE is transformed, once, and the mean of |Re| + |Im| over its half spectrum is the loss.  Evaluated in the inputs'
    dtype (float32 for the 16-bit ones) and returned in it; differentiable by autograd.  In float32 this form keeps the sign of
    each bin where the reference's takes it from a small difference of two large spectra."""
    if pred.dim() != 4 or pred.shape != target.shape:
        raise RuntimeError(f"fft_l1_mean: expected two (B, C, H, W) tensors of one shape, got {tuple(pred.shape)} and {tuple(target.shape)}")
    if pred.numel() == 0:
        raise RuntimeError("fft_l1_mean: empty input")
    work = pred.dtype if pred.dtype in (torch.float32, torch.float64) else torch.float32
    y = torch.fft.rfft2(pred.to(work) - target.to(work))
    return ((y.real.abs().sum() + y.imag.abs().sum()) / (2 * y.numel())).to(pred.dtype)


# out[i, j] = A[r, c] for the eight modes of data_augmentation (transforms.py:223-268): (r from j?, r mirrored?, c mirrored?)
_AUG_MODES = ((False, False, False), (False, True, False), (True, False, True), (True, False, False),
              (False, True, True), (False, False, True), (True, True, False), (True, True, True))


def border_reflect_index(n_padded, n):
    """Source indices of the first n_padded positions of an axis of n elements continued by cv2.BORDER_REFLECT
    (...cba|abcdefgh|hgf..., the edge-including reflection, numpy's 'symmetric'): m = y mod 2n, m < n ? m : 2n - 1 - m."""
    m = torch.arange(n_padded) % (2 * n)
    return torch.where(m < n, m, 2 * n - 1 - m)


def paired_patches(pairs, rows, gt_size, swap_rb=True):
    """The reference's training batch from uint8 images (paired_image_dataset.py:80-131 at scale 1, then the default collate).
    pairs: a sequence of (lq, gt) images, each (h, w, 3) uint8 (numpy arrays or CPU tensors; BGR as cv2 reads them, or RGB with
    swap_rb=False); rows: (index into pairs, top, left, mode) per sample.  Per sample, for both images: pad bottom / right to at
    least gt_size with cv2.BORDER_REFLECT (img_util.py:150-166), take the gt_size window at (top, left) (transforms.py:24-83),
    apply mode 0..7 of data_augmentation (transforms.py:223-268; the index table of include/wavemamba_hip.h), reverse the channels
    (swap_rb), HWC -> CHW, float32, / 255.  -> (lq, gt), each (B, 3, gt_size, gt_size) float32.  Rows out of range raise."""
    P = int(gt_size)
    ii, jj = torch.meshgrid(torch.arange(P), torch.arange(P), indexing="ij")
    out = ([], [])
    for index, top, left, mode in rows:
        imgs = [torch.as_tensor(im) for im in pairs[index]]
        if imgs[0].shape != imgs[1].shape:
            raise ValueError(f"paired_patches: lq {tuple(imgs[0].shape)} and gt {tuple(imgs[1].shape)} differ in shape")
        h, w = imgs[0].shape[:2]
        H, W = max(h, P), max(w, P)
        if not (0 <= top <= H - P and 0 <= left <= W - P and 0 <= mode <= 7):
            raise ValueError(f"paired_patches: row {(index, top, left, mode)} outside a {h} x {w} image padded to {H} x {W}")
        sy, sx = border_reflect_index(H, h)[top:top + P], border_reflect_index(W, w)[left:left + P]
        turn, flip_r, flip_c = _AUG_MODES[mode]
        r, c = (jj, ii) if turn else (ii, jj)
        r, c = (P - 1 - r if flip_r else r), (P - 1 - c if flip_c else c)
        for k, im in enumerate(imgs):
            if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3:
                raise ValueError(f"paired_patches: expected (h, w, 3) uint8 images, got {tuple(im.shape)} {im.dtype}")
            a = im[sy[r], sx[c]]                                  # (P, P, 3): out[i, j] = A[r, c], A = padded[top + ., left + .]
            if swap_rb:
                a = a.flip(-1)
            out[k].append(a.permute(2, 0, 1).to(torch.float32) / 255.0)
    empty = torch.empty(0, 3, P, P, dtype=torch.float32)
    return tuple(torch.stack(o) if o else empty.clone() for o in out)


DIHEDRAL_INVERSE = (0, 1, 6, 3, 4, 5, 2, 7)      # mode -> the mode that undoes it: the two rotations by a quarter swap


def dihedral(img, mode, dims=(0, 1)):
    """data_augmentation(img, mode) (transforms.py:223-268) on a tensor whose image axes are `dims` = (rows, columns) - (0, 1) for
    (h, w, 3), (-2, -1) for (..., h, w): out[i, j] = A[r, c] by _AUG_MODES, (h, w) -> (w, h) for modes 2, 3, 6, 7.  A view."""
    turn, flip_r, flip_c = _AUG_MODES[mode]
    flips = [d for d, f in zip(dims, (flip_r, flip_c)) if f]
    a = img.flip(flips) if flips else img
    return a.transpose(*dims) if turn else a


def dihedral_inverse(img, mode, dims=(0, 1)):
    """The transform that undoes dihedral(., mode): dihedral(., DIHEDRAL_INVERSE[mode])."""
    return dihedral(img, DIHEDRAL_INVERSE[mode], dims)


def _pad_to(n, window_size):
    return n + (window_size - n % window_size) % window_size


def images_pre_u8(images, modes, window_size=128, swap_rb=True):
    """ops.images_pre_u8 in plain PyTorch: per (h, w, 3) uint8 image (numpy array or CPU tensor) and mode,
    reflect_pad(chw(dihedral(img, mode)) / 255) bottom / right to multiples of window_size - the padding follows the transform, as
    check_image_size(aug(img)) pads - stacked to (N, 3, Hp, Wp) float32.  A padding that reaches the transformed image's size and
    images that pad to different shapes raise RuntimeError."""
    out = []
    for im, mode in zip(images, modes, strict=True):
        a = dihedral(torch.as_tensor(im), mode)
        if a.dtype != torch.uint8 or a.dim() != 3 or a.shape[2] != 3:
            raise RuntimeError(f"images_pre_u8: expected (h, w, 3) uint8 images, got {tuple(a.shape)} {a.dtype}")
        h, w = a.shape[:2]
        Hp, Wp = _pad_to(h, window_size), _pad_to(w, window_size)
        if h < 1 or w < 1 or Hp - h >= h or Wp - w >= w:
            raise RuntimeError(f"images_pre_u8: the reflect padding of a {h} x {w} image to {Hp} x {Wp} reaches the image's size")
        if swap_rb:
            a = a.flip(-1)
        x = a.permute(2, 0, 1).to(torch.float32) / 255.0
        out.append(F.pad(x[None], (0, Wp - w, 0, Hp - h), "reflect")[0])
    if len({tuple(o.shape) for o in out}) > 1:
        raise RuntimeError(f"images_pre_u8: the images pad to different shapes: {sorted({tuple(o.shape[1:]) for o in out})}")
    return torch.stack(out)


def images_post_u8(sources, rows, swap_rb=True):
    """ops.images_post_u8 in plain PyTorch.  sources: one (N, 3, Hp, Wp) float32 tensor or a pair of them; rows: per destination
    (h, w, [(tensor, index, mode), ...]) - the k network outputs of the (h, w) image transformed by `mode`.  Per destination:
    y_s = dihedral_inverse(source cropped to the transformed shape, mode); mean = (((y_0 + y_1) + y_2) + ...) * (1 / k) in float32,
    in the row's order; -> hwc(round_half_even(clamp(mean, 0, 1) * 255)) uint8, channels reversed with swap_rb.  A list of (h, w, 3)."""
    sources = (sources,) if isinstance(sources, torch.Tensor) else tuple(sources)
    out = []
    for h, w, srcs in rows:
        total = None
        for which, index, mode in srcs:
            ht, wt = (w, h) if _AUG_MODES[mode][0] else (h, w)
            y = dihedral_inverse(sources[which][index, :, :ht, :wt].to(torch.float32), mode, (-2, -1))
            total = y.clone() if total is None else total + y
        mean = total * torch.tensor(1.0 / len(srcs), dtype=torch.float32)
        q = (mean.clamp(0, 1) * 255.0).round().to(torch.uint8).permute(1, 2, 0)
        out.append((q.flip(-1) if swap_rb else q).contiguous())
    return out


def grad_guard(tensors, max_norm=None):
    """The record of ops.grad_guard / wm_grad_guard in plain PyTorch: 4 float32 on the CPU, {norm, found_inf, grad_scale, 0}.
    norm = float32(sqrt(sum of squares)) with every square and add in float64; found_inf = 1 when an element is not finite or the
    norm is not finite in float32; grad_scale = max(1, (norm + 1e-6) / max_norm) in float32 arithmetic when max_norm is a finite
    positive number and found_inf is 0, else 1 (torch.nn.utils.clip_grad_norm_'s coefficient, inverted).  The decision of the guarded
    step for CPU tensors (trainer.GradGuard), and the yardstick of the kernel's tests."""
    total = torch.zeros((), dtype=torch.float64)
    finite = True
    for t in tensors:
        d = t.detach().to("cpu", torch.float64).reshape(-1)
        finite = finite and bool(torch.isfinite(d).all())
        total = total + (d * d).sum()
    norm = total.sqrt().to(torch.float32)
    found = not finite or not bool(torch.isfinite(norm))
    scale = torch.ones((), dtype=torch.float32)
    if max_norm is not None and 0.0 < float(max_norm) < float("inf") and not found:
        scale = torch.clamp((norm + torch.tensor(1e-6, dtype=torch.float32)) / torch.tensor(float(max_norm), dtype=torch.float32), min=1.0)
    return torch.stack([norm, torch.tensor(1.0 if found else 0.0), scale, torch.zeros(())])


def adamw_step(params, grads, exp_avgs, exp_avg_sqs, lr, step, betas, eps, weight_decay, emas=None, ema_decay=None, grad_scale=None):
    """One step of ops.adamw_step / wm_adamw_step in plain PyTorch, in place: torch.optim.AdamW (amsgrad=False, maximize=False)
    written with the tensor operations of torch's single-tensor form - with a float lr it equals torch.optim.AdamW bit for bit in
    parameters and both moments - then, for a parameter with an entry in `emas`, the reference's model_ema (base_model.py:85-92)
    on the new weights.  `step`: the number of steps taken so far (this one is t = step + 1; the caller advances its counter).
    grad_scale: the update uses grad / grad_scale, the gradients themselves stay as they are.  A skipped step is the caller not
    calling this.  The update of trainer.HipAdamW for CPU tensors, and the yardstick of the kernel's tests."""
    beta1, beta2 = float(betas[0]), float(betas[1])
    lr, t = float(lr), float(int(step) + 1)
    bias_correction1, bias_correction2 = 1 - beta1 ** t, 1 - beta2 ** t
    step_size = lr / bias_correction1
    bias_correction2_sqrt = bias_correction2 ** 0.5
    emas = [None] * len(params) if emas is None else emas
    with torch.no_grad():
        for p, g, m, v, e in zip(params, grads, exp_avgs, exp_avg_sqs, emas):
            if grad_scale is not None:
                g = g / float(grad_scale)
            p.mul_(1 - lr * weight_decay)
            m.lerp_(g, 1 - beta1)
            v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
            denom = (v.sqrt() / bias_correction2_sqrt).add_(eps)
            p.addcdiv_(m, denom, value=-step_size)
            if e is not None:
                e.mul_(ema_decay).add_(p, alpha=1 - ema_decay)
