/*
 * wavemamba_hip.h - C ABI of libwavemamba_hip.so, the MI355X (gfx950) implementation of the
 * Wave-Mamba hot path: Haar DWT/IWT over NCHW feature maps, the selective-scan recurrence, and the
 * SS2D four-direction scan core.
 *
 * The reference (AlexZou14/Wave-Mamba, citations into /root/reference/) is pure Python; its only
 * FFI on this path is the pybind module `selective_scan_cuda.{fwd,bwd}` of the third-party package
 * `mamba_ssm`, reached through `selective_scan_fn` (basicsr/archs/wavemamba_arch.py:6, :383,
 * :465-471).  Each entry point below names the reference interface it replaces.  The Python host
 * side (wave_mamba_amd/ops.py) binds these symbols with ctypes and mirrors the reference's
 * operator surface (same names, argument meaning, error behaviour).
 *
 * Conventions
 *   - Plain pointers and sizes only; every pointer is a DEVICE pointer unless stated otherwise.
 *   - Ownership: the caller allocates every input, output and workspace buffer.  The library never
 *     allocates or frees device memory and keeps no state between calls (profiling hooks aside).
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls only enqueue work;
 *     they never synchronise the host.
 *   - Return value: WM_OK (0) on success; a negative WM_E* code for argument errors; a positive
 *     value is a hipError_t from the launch.  wm_strerror() renders either.
 *   - Tensors are dense, row-major ("contiguous") in the stated shape unless a stride is given.
 *   - dtype codes: WM_F32 = 0 (float), WM_BF16 = 1 (bfloat16 storage, fp32 arithmetic unless noted).
 */
#ifndef WAVEMAMBA_HIP_H
#define WAVEMAMBA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WM_OK 0
#define WM_EINVAL (-1)      /* bad shape / size argument */
#define WM_ENULL (-2)       /* required pointer is NULL */
#define WM_EALIGN (-3)      /* pointer not aligned to the element size */
#define WM_EWORKSPACE (-4)  /* workspace too small */
#define WM_EUNSUPPORTED (-5)/* argument combination not implemented */
#define WM_EHIP (-6)        /* a HIP runtime call made on behalf of the launch failed (device query, function attribute) */

#define WM_F32 0
#define WM_BF16 1

/* ABI version of this header (bumped on any signature change; entry points that are only ADDED - the _det forms, the channel
 * gather, wm_grad_guard and wm_adamw_step - change no signature a caller compiled against 34 uses, so they do not bump it). */
int wm_abi_version(void);
/* Identity of the sources this binary was compiled from: the first 16 hex digits of a sha256 over csrc/ and this header
 * (wave_mamba_amd/build.py passes it as -DWM_BUILD_ID; "unknown" for a bare hipcc build).  Measurements that describe
 * one binary (profiles/pmc_traffic.json) carry it, and bench.py quotes them only for the binary that is loaded. */
const char* wm_build_id(void);
const char* wm_strerror(int code);

/* --------------------------------------------------------------------------------------------
 * Haar DWT.  Replaces dwt_init(x) -> (x_LL, x_HL, x_LH, x_HH), wavemamba_arch.py:97-110
 * (DWT.forward :138-139, called from DownFRG.forward :973).
 *   x  (B, C, H, W)  H, W even   ->  ll, hl, lh, hh  each (B, C, H/2, W/2), same dtype as x.
 * bf16: every add rounds to bf16 like the reference's eager bf16 tensor arithmetic.
 * wm_dwt2d_bwd: gradient of the above; (dll, dhl, dlh, dhh) -> dx (B, C, H, W).
 * -------------------------------------------------------------------------------------------- */
int wm_dwt2d_fwd(const void* x, void* ll, void* hl, void* lh, void* hh,
                 int B, int C, int H, int W, int dtype, void* stream);
int wm_dwt2d_bwd(const void* dll, const void* dhl, const void* dlh, const void* dhh, void* dx,
                 int B, int C, int H, int W, int dtype, void* stream);

/* --------------------------------------------------------------------------------------------
 * Haar IWT.  Replaces iwt_init(x) -> h, wavemamba_arch.py:113-130 (IWT.forward :147-148, called
 * from upFRG.forward :1006 on cat([x_l, h_out_conv(x_h)], dim=1)).
 * The reference takes one (B, 4C, h, w) tensor whose channel blocks are [x1 | x2 | x3 | x4].  Here
 * each block is its own base pointer with its own batch stride (in elements), so the caller can
 * pass the concatenated tensor (x_k = x + k*C*h*w, stride 4*C*h*w) or the un-concatenated pair
 * (x1 = x_l, stride C*h*w;  x2..x4 = x_h + {0,1,2}*C*h*w, stride 3*C*h*w) without a copy.
 *   out (B, C, 2h, 2w) is ALWAYS fp32 (reference :122-123), whatever `dtype` the inputs have.
 * wm_idwt2d_bwd: dout (B, C, 2h, 2w) fp32 -> d1..d4 (same addressing, element type `dtype`).
 * -------------------------------------------------------------------------------------------- */
int wm_idwt2d_fwd(const void* x1, const void* x2, const void* x3, const void* x4,
                  int64_t bs1, int64_t bs2, int64_t bs3, int64_t bs4,
                  float* out, int B, int C, int h, int w, int dtype, void* stream);
int wm_idwt2d_bwd(const float* dout, void* d1, void* d2, void* d3, void* d4,
                  int64_t bs1, int64_t bs2, int64_t bs3, int64_t bs4,
                  int B, int C, int h, int w, int dtype, void* stream);

/* --------------------------------------------------------------------------------------------
 * Selective scan.  Replaces mamba_ssm's
 *   selective_scan_fn(u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False,
 *                     return_last_state=False)
 * as called at wavemamba_arch.py:465-471 (fp32 in / out / state, asserted at :472).
 *   u, delta, z, out : (batch, dim, L) fp32          A : (dim, N) fp32
 *   Bm, Cm           : (batch, G, N, L) fp32, dim % G == 0, channel d reads group d / (dim / G)
 *   D, delta_bias    : (dim) fp32 or NULL            z : NULL = no gate (out = y), else y*silu(z)
 *   last_state       : (batch, dim, N) fp32 or NULL
 *   1 <= N <= 32.
 *   delta' = softplus(delta + delta_bias) if delta_softplus else delta + delta_bias
 *   h_t = exp(delta'_t A) h_{t-1} + delta'_t B_t u_t ;  y_t = <C_t, h_t> + D u_t
 * The sequence is split into chunks scanned in parallel (local reduce -> carry scan -> local scan);
 * `workspace` holds the per-chunk (decay product, end state) pairs; query its size first.
 * -------------------------------------------------------------------------------------------- */
size_t wm_selscan_fwd_workspace_bytes(int batch, int dim, int L, int N, int G);
int wm_selscan_fwd(const float* u, const float* delta, const float* A, const float* Bm,
                   const float* Cm, const float* D, const float* z, const float* delta_bias,
                   float* out, float* last_state, void* workspace, size_t workspace_bytes,
                   int batch, int dim, int L, int N, int G, int delta_softplus, void* stream);

/* Backward of the above (mamba_ssm's selective_scan_cuda.bwd, reached by autograd in training,
 * basicsr/models/femasr_model.py:181).  z is not supported (the reference passes z=None, :467).
 *   dy (batch, dim, L) -> du, ddelta (batch, dim, L); dB, dC (batch, G, N, L);
 *   dA (dim, N), dD (dim) or NULL, dbias (dim) or NULL.  All outputs are OVERWRITTEN.
 */
size_t wm_selscan_bwd_workspace_bytes(int batch, int dim, int L, int N, int G);
int wm_selscan_bwd(const float* u, const float* delta, const float* A, const float* Bm,
                   const float* Cm, const float* D, const float* delta_bias, const float* dy,
                   float* du, float* ddelta, float* dA, float* dB, float* dC, float* dD,
                   float* dbias, void* workspace, size_t workspace_bytes,
                   int batch, int dim, int L, int N, int G, int delta_softplus, void* stream);

/* --------------------------------------------------------------------------------------------
 * Fused SS2D four-direction scan core.  Replaces SS2D.forward_core(x), wavemamba_arch.py:446-478:
 * direction flatten (:451-452), x_proj / dt_proj einsums (:453-455), the selective scan (:465-471)
 * and the flips / transposes back (:474-478), without materialising any of the intermediates.
 *   x (B, D, H, W) fp32;  x_proj_weight (4, R + 2N, D);  dt_projs_weight (4, D, R);
 *   dt_projs_bias (4, D);  A_logs (4 D, N)  [A = -exp(A_logs)];  Ds (4 D)
 *   outputs, each (B, D, H*W) in row-major l, in the reference's return order (:478):
 *     y_row_fwd = out_y[:,0], y_row_rev = flip(out_y[:,2]), y_col_fwd, y_col_rev (column scans,
 *     transposed back).  merged != 0: only y_row_fwd is written and holds the SUM of the four
 *     (what SS2D.forward computes next, :490, added in the reference's order); the other three
 *     pointers may be NULL.  wm_lfss_mid_fwd can add the four un-merged outputs while it reads them.
 *     merged must be 0 or 1 (2 was round 4's two-plane mode - measured slower, profiles/r04/core_ab_paired_planes.txt - deleted).
 *   Supported: N <= 32, R <= 4, D <= 64, D * H * W < 2^31 (else WM_EUNSUPPORTED: use wm_selscan_fwd); any H, W.
 *   W % 4 == 0 with 16-byte aligned x / y buffers: 16-byte tile accesses; otherwise (odd widths, fp32 planes only)
 *   the same kernels with element-wise tile accesses, slower per position.
 *   The workspace size depends on `merged` (three temporary y buffers) and on wm_ss2d_core_carry_select.
 */
size_t wm_ss2d_core_fwd_workspace_bytes(int B, int D, int H, int W, int N, int R, int merged);
/*   wm_ss2d_core_carry_select  what the chunk-reduce launch of wm_ss2d_core_fwd leaves for the carry over chunks (host state, as
 *   wm_conv2d_select): 0 (default) one sum of dt per (chunk, batch, channel), from which the carry launch forms
 *   P = exp2(sum_dt * A); 1 the NP values of P themselves (the form until this selector existed: 16-32 times the words for the
 *   same information).  The outputs have the same bits either way (parity tests and per-call A/B runs pin each in turn);
 *   wm_ss2d_core_fwd_workspace_bytes answers for the current choice, so size the workspace after selecting.  Other values: WM_EINVAL.
 */
int wm_ss2d_core_carry_select(int mode);
/*   Host-only: the work split wm_ss2d_core_fwd uses for this shape (no GPU needed; tests and tools).
 *   out[0..9] = waves per workgroup, rows per column segment, segments per column, column tiles, column workgroup slots
 *   per direction, steps per row chunk, row chunks, row workgroups per direction, workgroups per launch, estimated
 *   launch length in row-tile times x 100 under the dispatch model (wavemamba_hip.hip: core_makespan).
 */
int wm_ss2d_core_plan(int B, int D, int H, int W, int N, int R, int* out10);
/*   plane_dtype: storage type of x and of the y buffers, WM_F32 or WM_BF16 (bf16-storage mode: bf16 planes between
 *   the kernels, fp32 tiles / projection / state inside; needs W % 4 == 0 and 16-byte aligned planes: WM_EUNSUPPORTED /
 *   WM_EALIGN otherwise).
 */
/*   prepared: NULL, or the buffer wm_ss2d_core_prep filled from THESE parameters (wm_ss2d_core_prep_bytes(N) bytes,
 *   16-byte aligned): the bf16-split x_proj weight fragments, A * log2(e) and the per-channel constants the kernels
 *   read.  With NULL the call prepares them itself into the workspace (one more small launch); inference callers whose
 *   parameters do not change keep one prepared buffer per SS2D module.
 */
int wm_ss2d_core_fwd(const void* x, const float* x_proj_weight, const float* dt_projs_weight,
                     const float* dt_projs_bias, const float* A_logs, const float* Ds,
                     void* y_row_fwd, void* y_row_rev, void* y_col_fwd, void* y_col_rev,
                     int merged, void* workspace, size_t workspace_bytes, const void* prepared,
                     int B, int D, int H, int W, int N, int R, int plane_dtype, void* stream);
size_t wm_ss2d_core_prep_bytes(int N);
int wm_ss2d_core_prep(const float* x_proj_weight, const float* dt_projs_weight, const float* dt_projs_bias,
                      const float* A_logs, const float* Ds, void* prepared, int D, int N, int R, void* stream);

/* --------------------------------------------------------------------------------------------
 * Depth-wise 3x3 convolution, stride 1, zero padding 1, + bias, + optional SiLU.
 * Replaces nn.Conv2d(groups=channels) + nn.SiLU of SS2D (wavemamba_arch.py:346-355, :487) and the
 * ffn's conv2 (:220, :226) in LFSSBlock.  x, y (B, C, H, W) fp32; weight (C, 1, 3, 3); bias (C) or
 * NULL; act: 0 = none, 1 = SiLU, 2 = GELU (exact erf form), + 4: the nine taps of every channel rotated by 180 degrees
 * (weight.flip(2, 3) without the flipped copy: the input gradient of the same convolution is act = 4 on gy).
 * plane_dtype: storage type of x and y (WM_F32 / WM_BF16, fp32 arithmetic).  Forward only.
 * -------------------------------------------------------------------------------------------- */
int wm_dwconv3x3_fwd(const void* x, const float* weight, const float* bias, void* y,
                     int B, int C, int H, int W, int act, int plane_dtype, void* stream);

/* --------------------------------------------------------------------------------------------
 * LFSSBlock / SS2D per-position glue around the scan core, fused (forward only; C in {8,16,32},
 * inner width D = 2C, ffn hidden = 2C).  Token tensors are (B, L, C) rows unless the *_nchw flag
 * says (B, C, L); plane tensors are (B, D, L).  Reference lines: wavemamba_arch.py
 *   wm_lfss_in_fwd  : ln_1 (:524) + in_proj (:483) + chunk (:484) + NHWC->NCHW (:486)
 *                     tok -> x (conv input), z (gate)
 *   wm_lfss_mid_fwd : transpose (:491) + out_norm (:492) + *silu(z) (:493) + out_proj (:494)
 *                     + skip_scale residual (:525) + ln_2 + ffn.conv1 (:526, :226)
 *                     ysum, z, tok -> tok1, f (input of ffn.conv2).  ny = 1: `ysum` is the merged core output;
 *                     ny = 4: `ysum` points at four (B, D, L) buffers `ystride` ELEMENTS of the plane dtype apart in the order
 *                     [y_row_fwd, y_row_rev, y_col_fwd, y_col_rev] and the kernel adds them (:490) as it loads
 *   wm_lfss_out_fwd : gelu gate (:227-228) + ffn.conv3 (:230) + skip_scale2 residual (:526)
 *                     fc, tok1 -> out
 * -------------------------------------------------------------------------------------------- */
/* plane_dtype: storage type of the plane tensors x, z, ysum, f, fc (WM_F32; WM_BF16 at C = 32 - the bf16-storage
 * mode); token tensors are always fp32. */
int wm_lfss_in_fwd(const float* tok, int tok_nchw, const float* ln_w, const float* ln_b, float ln_eps,
                   const float* in_proj_weight, void* x, void* z, int B, int64_t L, int C, int plane_dtype, void* stream);
int wm_lfss_mid_fwd(const void* ysum, int ny, int64_t ystride, const void* z, const float* tok, int tok_nchw,
                    const float* out_norm_w, const float* out_norm_b, float out_norm_eps,
                    const float* out_proj_weight, const float* skip_scale,
                    const float* ln2_w, const float* ln2_b, float ln2_eps,
                    const float* conv1_weight, const float* conv1_bias,
                    float* tok1, void* f, int B, int64_t L, int C, int plane_dtype, void* stream);
/* wm_lfss_mid_fwd with the gate RECOMPUTED from `tok` instead of read: z = in_proj(ln_1(tok))[..., D:2D] (:485-486) on the
 * matrix cores, in the matrix-instruction order of wm_lfss_in_fwd (fp32 planes: bit-identical results).  With it
 * wm_lfss_in_fwd is called with z = NULL (the gate half is never written): 512 fewer bytes per position of the block's 3456.
 * C == 32 only (WM_EUNSUPPORTED otherwise). */
int wm_lfss_mid_rz_fwd(const void* ysum, int ny, int64_t ystride, const float* tok, int tok_nchw, const float* ln1_w,
                       const float* ln1_b, float ln1_eps, const float* in_proj_weight, const float* out_norm_w,
                       const float* out_norm_b, float out_norm_eps, const float* out_proj_weight,
                       const float* skip_scale, const float* ln2_w, const float* ln2_b, float ln2_eps,
                       const float* conv1_weight, const float* conv1_bias, float* tok1, void* f, int B, int64_t L,
                       int C, int plane_dtype, void* stream);
int wm_lfss_out_fwd(const void* fc, const float* tok1, const float* conv3_weight, const float* conv3_bias,
                    const float* skip_scale2, float* out, int out_nchw, int B, int64_t L, int C, int plane_dtype,
                    void* stream);
/* SS2D's prologue in one kernel (wavemamba_arch.py:483-487 behind ln_1, :524): wm_lfss_in_fwd(z = NULL) with the depth-wise 3x3
 * (conv2d, :486) and SiLU (:487) of wm_dwconv3x3_fwd(act = 1) folded in - tok -> xc = silu(conv2d(in_proj(ln_1(tok))[..., :D])) as
 * (B, 2C, H, W) fp32 planes; x itself never exists in HBM (-512 B per position, one launch less per LFSSBlock).  Bit-identical to the
 * two calls.  C == 32, plane_dtype == WM_F32, W % 32 == 0 and H W <= 2^23 only (WM_EUNSUPPORTED otherwise: use the two calls).
 * conv_weight (2C, 1, 3, 3); conv_bias (2C) or NULL.
 * wm_lfss_in_conv_band_rows: host only - the output rows a wave walks per band at this shape (every band recomputes two more rows
 * of x); negative status outside the domain. */
int wm_lfss_in_conv_fwd(const float* tok, int tok_nchw, const float* ln_w, const float* ln_b, float ln_eps,
                        const float* in_proj_weight, const float* conv_weight, const float* conv_bias, float* xc,
                        int B, int H, int W, int C, int plane_dtype, void* stream);
int wm_lfss_in_conv_band_rows(int B, int H, int W);
/* wm_lfss_out_fwd with the gated ffn's depth-wise 3x3 (conv2, wavemamba_arch.py:220, :226) folded in: takes conv1's
 * output planes f (B, 2C, H, W) instead of conv2's, so `fc` never exists in HBM (-512 B per position, one launch less
 * per LFSSBlock).  Bit-identical to wm_dwconv3x3_fwd(act = none) + wm_lfss_out_fwd on fp32 planes.
 * C == 32 and W % 32 == 0 only (WM_EUNSUPPORTED otherwise: use the two calls).  conv2_bias may be NULL. */
int wm_lfss_out_conv_fwd(const void* f, const float* conv2_weight, const float* conv2_bias, const float* tok1,
                         const float* conv3_weight, const float* conv3_bias, const float* skip_scale2, float* out,
                         int out_nchw, int B, int H, int W, int C, int plane_dtype, void* stream);
/* The gated ffn without f (conv1's output planes) in HBM: wm_lfss_mid_rz_fwd + wm_lfss_out_conv_fwd as
 *   wm_lfss_mid_rz_tok_fwd  wm_lfss_mid_rz_fwd that ends at tok1 (no ln_2, conv1 or f; bit-identical tok1).  C == 32, ny == 4 and
 *                           plane_dtype == WM_F32 only (WM_EUNSUPPORTED otherwise).
 *   wm_lfss_ffn_fwd         tok1 (B, L, C) -> out = tok1 * skip_scale2 + conv3(gelu(fc[:C]) * fc[C:]), fc = conv2(conv1(ln_2(tok1)))
 *                           (wavemamba_arch.py:226-230, :526) in one kernel: f on the depth-wise 3x3's one-pixel halo is recomputed
 *                           from tok1, never stored (-700 B per position).  Bit-identical to the pair on fp32 planes.  C == 32,
 *                           plane_dtype == WM_F32, W % 32 == 0 and H W <= 2^23 only (WM_EUNSUPPORTED otherwise: use the pair).
 *                           conv2_bias may be NULL; out (B, L, C) or (B, C, H, W) when out_nchw, aliases no input.  band_rows: output
 *                           rows per band of the row walk, 0 = the entry's plan.
 *   wm_lfss_ffn_band_rows   host only - that plan at this shape (every band recomputes two more rows of f); negative status outside
 *                           the domain. */
int wm_lfss_mid_rz_tok_fwd(const void* ysum, int ny, int64_t ystride, const float* tok, int tok_nchw, const float* ln1_w,
                           const float* ln1_b, float ln1_eps, const float* in_proj_weight, const float* out_norm_w,
                           const float* out_norm_b, float out_norm_eps, const float* out_proj_weight, const float* skip_scale,
                           float* tok1, int B, int64_t L, int C, int plane_dtype, void* stream);
int wm_lfss_ffn_fwd(const float* tok1, const float* ln2_w, const float* ln2_b, float ln2_eps, const float* conv1_weight,
                    const float* conv1_bias, const float* conv2_weight, const float* conv2_bias, const float* conv3_weight,
                    const float* conv3_bias, const float* skip_scale2, float* out, int out_nchw, int B, int H, int W, int C,
                    int plane_dtype, int band_rows, void* stream);
int wm_lfss_ffn_band_rows(int B, int H, int W);

/* --------------------------------------------------------------------------------------------
 * LayerNorm2d of the HFE branch (first "next" row): per-pixel LayerNorm over the C
 * channels of an NCHW map, eps inside the square root, biased variance (wavemamba_arch.py:532-569).
 * x, y (B, C, L) fp32; C in {8, 16, 32, 64}.  Forward only.
 * -------------------------------------------------------------------------------------------- */
int wm_layernorm2d_fwd(const float* x, const float* weight, const float* bias, float eps, float* y,
                       int B, int64_t L, int C, void* stream);

/* --------------------------------------------------------------------------------------------
 * Channel Gram matrix over the pixel axis (HFE branch): G[b][i][j] = sum_l X[b][i][l] Y[b][j][l],
 * nx[b][i] = sum_l X^2, ny likewise.  X, Y (B, C, L) fp32, C <= 32; G (B, C, C), nx, ny (B, C) are
 * overwritten.  Replaces torch.cdist(x, perception) (wavemamba_arch.py:664) and
 * normalize(q) @ normalize(k)^T (:787-790), both contractions over H*W.  `workspace`
 * (wm_gram_workspace_bytes, 16-byte aligned) holds the per-block partial sums, which are added in a
 * fixed order: the result is bit-reproducible run to run, as the reference's matmul is.
 * -------------------------------------------------------------------------------------------- */
size_t wm_gram_workspace_bytes(int B, int C, int64_t L);
int wm_gram_fwd(const float* X, const float* Y, float* G, float* nx, float* ny, void* workspace,
                size_t workspace_bytes, int B, int C, int64_t L, void* stream);

/* Training-side gradients of the two streaming helpers above.
 *   wm_dwconv3x3_wgrad: dW (C,1,3,3) and db (C, may be NULL) of the depth-wise conv from x and gy (B,C,H,W);
 *     the input gradient is wm_dwconv3x3_fwd(gy, weight, NULL, act = 4).
 *   wm_layernorm2d_bwd: reference LayerNormFunction.backward (wavemamba_arch.py:545-557): gx, dweight, dbias. */
int wm_dwconv3x3_wgrad(const float* x, const float* gy, float* dW, float* db, int B, int C, int H, int W,
                       void* stream);
int wm_layernorm2d_bwd(const float* x, const float* weight, const float* gy, float eps, float* gx,
                       float* dweight, float* dbias, int B, int64_t L, int C, void* stream);


/* Dense 3x3 (stride 1, zero padding 1) and 1x1 convolutions, NCHW fp32, with the element-wise neighbours they
 * have in the HFE branch fused (wavemamba_arch.py: PAConv k2/k3/k4 :690-697 on
 * cat([x, gather(candidates, idx)]) :666/:713, CMTAttention.qkv/.project_out :768-797, FeedForward 1x1s :733-742,
 * DownFRG.l_conv on cat([x_LL, x_d]) :966/:975, upFRG.h_out_conv :993/:1006, UNet.conv_01/.last/ps_down*
 * :1015-1037).  Forward only.  Runs on the bf16 matrix cores with a two-term split of both operands (three
 * products, fp32 accumulation): 3-4e-6 relative to an fp64 convolution, see csrc/conv2d.hip.h.
 *   wm_conv2d_prep    weight (Cout, Cin, ks, ks), ks in {1, 3} -> `wfrag` (wm_conv2d_wfrag_bytes(Cout, Cin, ks) bytes,
 *                     16-byte aligned, caller-owned): split, zero-padded to 16 | Cin and 32 | Cout, MFMA fragment
 *                     order.  Redo whenever the weight changes.
 *   wm_conv2d_fwd     x = cat([xa (B, Ca, H, W), xb' (B, Cb, H, W)], 1) where xb' = xb (Cb_src == Cb, xb_index NULL)
 *                     or xb'[b, c] = xb[b, xb_index[b, c]] for xb (B, Cb_src, H, W), xb_index (B, Cb) int32
 *                     (torch.gather over channels, never materialised); Cb may be 0 (xb, xb_index ignored);
 *                     Ca % 8 == 0 when Cb > 0.
 *                     y (B, Cout, H, W) = conv(x) + bias;  y *= sigmoid(gate) if gate;  y += residual if residual
 *                     (gate, residual: (B, Cout, H, W), may be NULL; bias may be NULL).  `wfrag` prepared for
 *                     Cin = Ca + Cb and the same ks.  H * W < 2^31.
 *   wm_conv2d_gated_fwd  y = conv3x3(x; wfrag3) * sigmoid(conv1x1(x; wfrag1) + bias1) over the same (concatenated /
 *                     gathered) input: PAConv's k3(x) * sigmoid(k2(x)) (:694-697) in one kernel - the 1x1 shares the
 *                     3x3's centre-tap operand fragments.  wfrag3 / wfrag1 prepared with ks = 3 / 1 for (Cout, Ca + Cb).
 *   wm_conv2d_select  which 3x3 kernel serves wm_conv2d_fwd / wm_conv2d_gated_fwd: 0 (default) by problem size - the
 *                     persistent wave-specialised kernel (one workgroup per compute unit, producer waves fetch / split
 *                     / stage, consumer waves multiply: conv2d_ws.hip.h) when every compute unit gets a few tiles, the
 *                     first-generation kernel otherwise; 1 always the first generation; 2 the wave-specialised one
 *                     wherever its limits allow (a batch element of each tensor < 4 GiB, <= 128 gathered channels, not
 *                     gate and residual together).  Both accumulate in the same order: results are bit-identical.
 *                     Process-wide; WM_CONV_WS=0 in the environment = select(1).  WM_EINVAL for another mode. */
int wm_conv2d_select(int mode);
size_t wm_conv2d_wfrag_bytes(int Cout, int Cin, int ks);
int wm_conv2d_prep(const float* weight, void* wfrag, int Cout, int Cin, int ks, void* stream);
/* y = conv1x1(LayerNorm2d(x; ln_weight, ln_bias, ln_eps)) + bias (+ residual): HFEBlock's norm1 -> attn.qkv and norm2 ->
 * ffn.project_in[0] (wavemamba_arch.py:843-851 over LayerNorm2d :532-569) as ONE kernel - the normalisation happens in the registers
 * the 1x1 kernel stages its pixels through (same arithmetic as wm_layernorm2d_fwd + wm_conv2d_fwd: bit-identical results), the
 * LayerNorm launch and its 256 B per position are gone.  Cin == 32 only (WM_EUNSUPPORTED otherwise); `wfrag` from
 * wm_conv2d_prep(weight (Cout, 32, 1, 1)); bias, residual may be NULL. */
int wm_conv2d_ln_fwd(const float* x, const float* ln_weight, const float* ln_bias, float ln_eps, const void* wfrag, const float* bias,
                     const float* residual, float* y, int B, int Cin, int Cout, int H, int W, void* stream);
/* y = conv1x1(act(dwconv3x3(x) + dw_bias)) + bias (+ residual): a depth-wise 3x3 whose only reader is a 1x1 convolution, as ONE
 * kernel - FeedForward.project_out (wavemamba_arch.py:739-741, act = GELU) and the value third of CMTAttention.qkv_dwconv under the
 * folded project_out (:771, :797).  Bit-identical to wm_dwconv3x3_fwd + wm_conv2d_fwd; the plane between them (256 B per position,
 * written and read back) never exists.  x: 32 consecutive channel planes (H, W) fp32 per batch element, batch elements
 * x_batch_stride ELEMENTS apart (a channel slice of a wider tensor; 4-byte alignment suffices); dw_weight (32, 1, 3, 3); dw_bias (32)
 * or NULL; act: 0 = none, 2 = GELU (exact erf form), anything else WM_EINVAL; `wfrag` from wm_conv2d_prep(weight (32, 32, 1, 1));
 * bias, residual (B, 32, H, W) may be NULL; y (B, 32, H, W) aliases no input.  C == Cout == 32 and H W < 2^26 only
 * (WM_EUNSUPPORTED otherwise: use the two calls). */
int wm_dwconv_conv1x1_fwd(const float* x, int64_t x_batch_stride, const float* dw_weight, const float* dw_bias, int act,
                          const void* wfrag, const float* bias, const float* residual, float* y, int B, int C, int Cout, int H,
                          int W, void* stream);
/* The two heads of an HFE block as ONE kernel each: norm1 -> attn.qkv -> qkv_dwconv on the q | k channels (wavemamba_arch.py:768-771,
 * Cout = 96, Cdw = 64) and norm2 -> ffn.project_in (:733-736, Cout = Cdw = 32).
 *   y[:, :Cdw] = dwconv3x3(conv1x1(LayerNorm2d(x)) + bias)[:, :Cdw] + dw_bias      y[:, Cdw:] = (conv1x1(LayerNorm2d(x)) + bias)[:, Cdw:]
 * Bit-identical to wm_conv2d_ln_fwd followed by wm_dwconv3x3_fwd on the first Cdw channels; the plane between them (2 x 4 Cdw bytes
 * per position) never exists.  x (B, 32, H, W); `wfrag` from wm_conv2d_prep(weight (Cout, 32, 1, 1)); dw_weight (Cdw, 1, 3, 3); bias
 * (Cout) and dw_bias (Cdw) may be NULL; y (B, Cout, H, W) aliases no input.  band_rows: output rows per band of the row walk, 0 = the
 * entry's choice (tests force several bands on small maps).  Cin == 32, (Cout, Cdw) in {(96, 64), (32, 32)} and H W < 2^25 only
 * (WM_EUNSUPPORTED otherwise: use the two calls). */
int wm_ln_conv1x1_dwconv_fwd(const float* x, const float* ln_weight, const float* ln_bias, float ln_eps, const void* wfrag,
                             const float* bias, const float* dw_weight, const float* dw_bias, float* y, int B, int Cin, int Cout,
                             int Cdw, int H, int W, int band_rows, void* stream);
/* The training form of the same convolutions (the F.conv2d calls of wavemamba_arch.py under autograd, femasr_model.py:170-181:
 * forward, and - on the transposed, flipped weight - the input gradient): fp16 matrix cores, two-term split of both operands
 * (22 significant bits, fp32-class: ~1e-7 relative to an fp64 convolution instead of the bf16 form's 3-4e-6, which the
 * parameter gradients of the deepest blocks do not tolerate), each tensor scaled by a power of two taken from its largest
 * finite magnitude so that fp16's exponent range is never the limit.  y = conv(x, weight) + bias (bias may be NULL), ks in {1, 3}.
 * `amax`: TWO device floats, written by the call ({max |x|, max |weight|}; in a registered zero arena - wm_zero_arena_register -
 * the call issues no memset node); `wfrag`: wm_conv2d_wfrag_bytes(Cout, Cin, ks) bytes, 16-byte aligned; both caller-owned
 * scratch.  dgrad != 0: `weight` (Cin, Cout, ks, ks) is the FORWARD convolution's weight and the call computes that convolution's
 * input gradient from x = gy: the convolution with w'[co][ci][ky][kx] = weight[ci][co][ks-1-ky][ks-1-kx] (what autograd evaluates
 * as conv(gy, weight.transpose(0, 1).flip(2, 3))), its fragments read straight from `weight` - no flipped copy exists; Cin / Cout
 * are those of the gradient convolution (= the forward's Cout / Cin).  Two launches: magnitudes + weight preparation, convolution.
 * Same kernels, tilings and limits as wm_conv2d_fwd; no concatenated / gathered second input, no gate; nothing synchronises the
 * host.  (Rounds 4-5 exported the steps one by one - wm_conv2d_amax / _prep_f16 / _fwd_f16 / wm_conv2d_f16: folded into this call.) */
int wm_conv2d_f16_steps(const float* x, const float* weight, const float* bias, float* y, float* amax, void* wfrag, int B, int Cin,
                        int Cout, int H, int W, int ks, int dgrad, void* stream);
int wm_conv2d_fwd(const float* xa, const float* xb, const int* xb_index, const void* wfrag, const float* bias,
                  const float* gate, const float* residual, float* y, int B, int Ca, int Cb, int Cb_src, int Cout,
                  int H, int W, int ks, void* stream);
int wm_conv2d_gated_fwd(const float* xa, const float* xb, const int* xb_index, const void* wfrag3, const void* wfrag1,
                        const float* bias1, float* y, int B, int Ca, int Cb, int Cb_src, int Cout, int H, int W,
                        void* stream);
/* (ll, hl, lh, hh) = dwt_init(conv3x3(img) + bias): a 3x3 convolution whose only reader is the Haar analysis, as ONE kernel -
 * UNet.conv_01 followed by down_group1's DWT (wavemamba_arch.py:1037, :973).  The wave-specialised kernel forms the four sub-bands
 * of each 2x2 quad in its epilogue; the full-resolution plane between the two (written once, read once) never exists.  Bit-identical
 * to wm_conv2d_fwd + wm_dwt2d_fwd.  img (B, Cin, H, W); `wfrag` from wm_conv2d_prep(weight (Cout, Cin, 3, 3)); bias (Cout) or NULL;
 * ll, hl, lh, hh each (B, Cout, H / 2, W / 2).  H, W odd: WM_EINVAL.  dtype == WM_F32 and Cout == 32 only, and only where the
 * wave-specialised kernel runs (a batch element of the input and of the plane < 4 GiB, wm_conv2d_select not 1): WM_EUNSUPPORTED
 * otherwise (use the two calls). */
int wm_conv2d_dwt_fwd(const void* img, const void* wfrag, const float* bias, void* ll, void* hl, void* lh, void* hh, int B, int Cin,
                      int Cout, int H, int W, int dtype, void* stream);
/* y = conv3x3(iwt_init(cat([low, high], 1))) + bias (+ residual): a Haar synthesis whose only reader is a 3x3 convolution, as ONE
 * kernel - the last upFRG's IWT followed by UNet.last (wavemamba_arch.py:1006, :1062).  The producer waves of the wave-specialised
 * kernel load the four band values of each 2x2 quad and form the input tile from them; the full-resolution plane between the two never
 * exists.  Bit-identical to wm_idwt2d_fwd + wm_conv2d_fwd.  low (B, Cin, H / 2, W / 2) = x1, high (B, 3 Cin, H / 2, W / 2) = x2 | x3 | x4
 * (the un-concatenated pair of wm_idwt2d_fwd); `wfrag` from wm_conv2d_prep(weight (Cout, Cin, 3, 3)); bias (Cout), residual
 * (B, Cout, H, W) may be NULL; y (B, Cout, H, W).  H, W (of y) odd: WM_EINVAL.  dtype == WM_F32 and Cin == 32 only, and only where the
 * wave-specialised kernel runs (a batch element of the synthesised plane and of y < 4 GiB, wm_conv2d_select not 1): WM_EUNSUPPORTED
 * otherwise (use the two calls). */
int wm_idwt_conv2d_fwd(const void* low, const void* high, const void* wfrag, const float* bias, const float* residual, float* y, int B,
                       int Cin, int Cout, int H, int W, int dtype, void* stream);

/* Backward of wm_ss2d_core_fwd: autograd of SS2D.forward_core (wavemamba_arch.py:446-478) - the four directional
 * flattenings, the x_proj / dt_proj einsums and the selective scan - without materialising xs / dts / Bs / Cs.
 *   dy_*            gradients of the four outputs in wm_ss2d_core_fwd's order, each (B, D, L) row-major positions; for
 *                   the merged forward pass the same pointer four times.
 *   dx (B, D, H, W), dx_proj_weight (4, R + 2N, D), ddt_projs_weight (4, D, R), ddt_projs_bias (4, D),
 *   dA_logs (4 D, N), dDs (4 D): overwritten.
 * Limits: N <= 32, R <= 4, D <= 64; workspace wm_ss2d_core_bwd_workspace_bytes(...), 16-byte aligned. */
size_t wm_ss2d_core_bwd_workspace_bytes(int B, int D, int H, int W, int N, int R);
int wm_ss2d_core_bwd(const float* x, const float* x_proj_weight, const float* dt_projs_weight,
                     const float* dt_projs_bias, const float* A_logs, const float* Ds, const float* dy_row_fwd,
                     const float* dy_row_rev, const float* dy_col_fwd, const float* dy_col_rev, float* dx,
                     float* dx_proj_weight, float* ddt_projs_weight, float* ddt_projs_bias, float* dA_logs, float* dDs,
                     void* workspace, size_t workspace_bytes, int B, int D, int H, int W, int N, int R, void* stream);

/* nn.LayerNorm(C) over the last axis of contiguous token tensors (T, C): LFSSBlock.ln_1 / ln_2, SS2D.out_norm
 * (wavemamba_arch.py:385, :493, :507-526), forward and backward (training).  C in {8, 16, 32, 64}; biased variance,
 * eps inside the square root; dweight / dbias (C) are overwritten.  16-byte aligned pointers. */
int wm_layernorm_tok_fwd(const float* x, const float* weight, const float* bias, float eps, float* y, int64_t T, int C,
                         void* stream);
int wm_layernorm_tok_bwd(const float* x, const float* weight, const float* gy, float eps, float* gx, float* dweight,
                         float* dbias, int64_t T, int C, void* stream);

/* The caller's I/O step (inference_wavemamba.py:99-113, basicsr/utils/img_util.py:9-98).
 *   wm_image_pre_u8   image (h, w, 3) uint8 on the device -> out (3, Hp, Wp) fp32 = channel-major, / 255, reflect-padded
 *                     bottom / right (Hp >= h, Wp >= w, pads smaller than the image); swap_rb: BGR -> RGB.
 *   wm_image_post_u8  in (3, Hp, Wp) fp32 -> image (h, w, 3) uint8 = round_half_even(clamp(in[:, :h, :w], 0, 1) * 255);
 *                     swap_rb: RGB -> BGR. */
int wm_image_pre_u8(const uint8_t* image, float* out, int h, int w, int Hp, int Wp, int swap_rb, void* stream);
int wm_image_post_u8(const float* in, uint8_t* image, int h, int w, int Hp, int Wp, int swap_rb, void* stream);

/* The same I/O step for N images per launch, a dihedral mode per image and a group average on the way out, csrc/images_io.hip.h:
 * batched, graph-replayed and self-ensembled inference.  Both are driven by DEVICE tables of int64 words (ops.images_io_table).
 *   wm_images_pre_u8   row n = {image, h, w, mode}: a contiguous (h, w, 3) uint8 image on the device and a mode 0..7 of
 *                      data_augmentation (the table of wm_paired_patches_u8 below; modes 2, 3, 6, 7 turn h x w into w x h).
 *                      out[n] (3, Hp, Wp) fp32 = reflect_pad(chw(mode(image)) / 255): the padding follows the transform, bottom / right
 *                      of the transformed image, as check_image_size(aug(img)) pads.  out is contiguous (N, 3, Hp, Wp); every row
 *                      must give the launch's (Hp, Wp) with pads smaller than the transformed image.  swap_rb: BGR -> RGB.
 *   wm_images_post_u8  row = {image, h, w, k, word_0 .. word_7}: a contiguous (h, w, 3) uint8 destination and k in 1..8 sources,
 *                      word = mode | tensor << 8 | index << 16 naming image `index` of src0 (tensor 0; (N0, 3, Hp0, Wp0) fp32,
 *                      contiguous) or of src1 (tensor 1; NULL with N1 = 0 when unused) - the result of the network on the image
 *                      transformed by `mode`.  image = hwc(round_half_even(clamp(mean, 0, 1) * 255)), mean = (((y_0 + y_1) + ...)
 *                      + y_{k-1}) * (1 / k) in fp32 in the row's order, y_s = source s cropped to the transformed shape and turned
 *                      back by the inverse mode.  k = 1, mode 0 is wm_image_post_u8 bit for bit.  h_max / w_max: the largest
 *                      destination (the grid).  swap_rb: RGB -> BGR.
 * One launch each, no atomics, nothing zeroed first: both capture into a HIP graph, and the tables are read by the KERNELS.  The host
 * cannot check a device table: a pre row that names no image, does not fit (Hp, Wp) or whose padding reaches the image's size
 * yields zeros; a post row with a NULL image, k outside 1..8, a source index outside its tensor or a source smaller than the
 * destination's transformed shape is left unwritten - neither indexes out of range.  The pointers are the caller's responsibility.
 * WM_EINVAL: a negative size; an empty launch is a no-op; WM_EALIGN: table not 8-byte, fp32 tensors not 4-byte aligned;
 * WM_EUNSUPPORTED: more than 65535 images / rows of the table, Hp or h_max above 65535, Wp or w_max above 65535 * 32. */
int wm_images_pre_u8(const int64_t* table, float* out, int N, int Hp, int Wp, int swap_rb, void* stream);
int wm_images_post_u8(const int64_t* table, const float* src0, int N0, int Hp0, int Wp0, const float* src1, int N1, int Hp1, int Wp1,
                      int rows, int h_max, int w_max, int swap_rb, void* stream);

/* A training batch from uint8 images on the device: the train phase of PairedImageDataset.__getitem__ after the decode
 * (basicsr/data/paired_image_dataset.py:80-131 at scale 1) and the default collate, csrc/patch_batch.hip.h.  Per sample b the
 * row table[b] = {lq_ptr, gt_ptr, h, w, top, left, mode, reserved} (int64 each; the two pointers are device addresses of
 * contiguous (h, w, 3) uint8 images of one shape) yields lq[b] and gt[b], each (3, P, P) fp32:
 *   padding   bottom / right to H = max(h, P), W = max(w, P) with cv2.BORDER_REFLECT (img_util.py:150-166): padded row y is source
 *             row m < h ? m : 2 h - 1 - m, m = y mod 2 h, columns alike - the edge-including reflection (numpy 'symmetric'), not the
 *             'reflect' of wm_image_pre_u8; no padded image is made;
 *   crop      the window [top, top + P) x [left, left + P) of both (paired_random_crop, transforms.py:24-83);
 *   augment   mode 0..7 of data_augmentation (transforms.py:223-268): identity, flipud, rot90, flipud(rot90), rot90 k=2,
 *             flipud(rot90 k=2), rot90 k=3, flipud(rot90 k=3);
 *   convert   channel-major, uint8 / 255 in fp32 (img2tensor, img_util.py:9-38); swap_rb: BGR -> RGB.
 * Bit for bit what the reference's dataset and collate hand to feed_data.  One launch, every output element written (nothing is
 * zeroed first), so it captures into a HIP graph; the table is read by the KERNEL, so rewriting it between replays changes the
 * crops.  The host cannot check a device table: the kernel clamps top / left into [0, H - P] / [0, W - P] and uses mode & 7, and a
 * row with h or w outside [1, 2^30] or a NULL image yields zeros - a wrong row selects a wrong window but never reads outside
 * the image it names.  The pointers themselves are the caller's responsibility.  Images may start at any byte.
 * WM_EINVAL: B < 0 or P <= 0; B == 0 is a no-op; WM_EALIGN: table not 8-byte, lq / gt not 4-byte aligned; WM_EUNSUPPORTED: more
 * than 2^24 - 1 tiles of 32 x 32 (2 B ceil(P / 32)^2). */
int wm_paired_patches_u8(const int64_t* table, float* lq, float* gt, int B, int P, int swap_rb, void* stream);

/* dW (O, I) = gy^T x for token-major gy (T, O), x (T, I): weight gradient of nn.Linear (SS2D.in_proj / out_proj,
 * wavemamba_arch.py:345 / :386) in training.  (O, I) in {(128,32), (32,64), (64,16), (16,32), (32,16), (16,16), (64,32),
 * (32,32), (16,64)}: the in_proj / out_proj shapes of hidden_dim 32, 16, 8. */
int wm_linear_wgrad(const float* gy, const float* x, float* dW, int64_t T, int O, int I, void* stream);
/* Weight gradient of a dense convolution (stride 1, 'same' zero padding, ks = 1 or 3):
 *   dW[co][ci][ky][kx] = sum_{b,h,w} gy[b][co][h][w] * x[b][ci][h + ky - ks/2][w + kx - ks/2]
 * - what autograd evaluates for the weight of every nn.Conv2d reached from WaveMamba.forward in training (ATen:
 * convolution_backward, output_mask[1]; on ROCm MIOpen's NHWC implicit-GEMM kernels between layout transposes).
 * gy (B, Cout, H, W), x (B, Cin, H, W) fp32 NCHW, 16-byte aligned; dW (Cout, Cin, ks, ks) is overwritten.
 * bf16 matrix cores with split operands (three products, ~4e-6 per product, fp32 accumulation).
 * Supported: W % 32 == 0, Cout <= 16, 32, 64 or 96 (tiles of 16: 1, 2, 4, 6); else WM_EUNSUPPORTED (workspace_bytes 0) and
 * the caller keeps ATen's gradient.
 * db (Cout) or NULL: the BIAS gradient db[co] = sum_{b,h,w} gy[b][co][h][w] (output_mask[2]) from the same pass over gy - fp32
 * sums in a fixed order (bit-reproducible), overwritten; wm_plane_sums is the stand-alone form.
 */
size_t wm_conv2d_wgrad_workspace_bytes(int B, int Cin, int Cout, int H, int W, int ks);
int wm_conv2d_wgrad(const float* gy, const float* x, float* dW, float* db, void* workspace, size_t workspace_bytes, int B, int Cin,
                    int Cout, int H, int W, int ks, void* stream);

/* The two loss terms of FeMaSRModel.optimize_parameters (basicsr/models/femasr_model.py:171-179): nn.L1Loss() on the prediction and
 * FFTLoss (basicsr/losses/losses.py:306-313: an L1 mean over the stacked real / imaginary parts of rfft2 = the same mean over the
 * interleaved floats of the complex tensor).  out[0] = mean_i |a_i - b_i| (zeroed here; one atomic per workgroup: ~1e-7 run to run);
 * ga_i = gout[0] * sign(a_i - b_i) / n (sign(0) = 0, like ATen).  a, b, ga: n fp32 elements, dense; gout: one device float.
 * (ATen's own reduction zeroes its semaphores with hipMemsetAsync, which must not be captured into a HIP graph on this runtime:
 * see the note on zero-initialised outputs below.) */
int wm_l1_mean_fwd(const float* a, const float* b, float* out, int64_t n, void* stream);
int wm_l1_mean_bwd(const float* a, const float* b, const float* gout, float* ga, int64_t n, void* stream);

/* The SSIM training loss: SSIM(window_size = 11, size_average = True) of basicsr/models/cal_ssim.py:17-35, :39-64 - what
 * FeMaSRModel builds as self.ssim (basicsr/models/femasr_model.py:29, :172) and options/train_wavemamba_uhdll.yml:99-100 weights
 * (pixel_ssim_opt) - csrc/ssim_loss.hip.h.  a, b: `planes` (= B C) dense fp32 planes of H x W, any H, W >= 1.  Per plane the five
 * moments mu1, mu2, e11, e22, e12 with the 11 x 11 Gaussian of sigma 1.5 (cal_ssim.py:7-15: float32 taps) and ZERO padding of 5,
 * S = (2 mu1 mu2 + C1)(2 (e12 - mu1 mu2) + C2) / ((mu1^2 + mu2^2 + C1)((e11 - mu1^2) + (e22 - mu2^2) + C2)), C1 = 0.01^2,
 * C2 = 0.03^2; out[0] = the mean of S over all planes and pixels (float64 accumulation; identical inputs give exactly 1).
 *   wm_ssim_mean_fwd: two launches, no atomics, no memset, deterministic.  workspace: wm_ssim_workspace_bytes(planes, H, W) bytes,
 *     8-byte aligned, written before it is read (0 = invalid shape, or more than 2^24 - 1 tiles: WM_EUNSUPPORTED).  For a gradient
 *     pass q and r (each planes H W floats: dS/de11 = dS/de22 and dS/de12) with p1 and / or p2 (dS/dmu1, dS/dmu2); all four NULL
 *     stores nothing.
 *   wm_ssim_mean_bwd: gx = gout[0] / n * [ w * p + 2 x (w * q) + other (w * r) ], n = planes H W, gout one device float: the
 *     gradient for a is (x = a, other = b, p = p1), for b (x = b, other = a, p = p2).  One launch. */
size_t wm_ssim_workspace_bytes(int64_t planes, int H, int W);
int wm_ssim_mean_fwd(const float* a, const float* b, float* out, float* p1, float* p2, float* q, float* r, void* workspace,
                     size_t workspace_bytes, int64_t planes, int H, int W, void* stream);
int wm_ssim_mean_bwd(const float* x, const float* other, const float* p, const float* q, const float* r, const float* gout,
                     float* gx, int64_t planes, int H, int W, void* stream);

/* The FFT training loss: FFTLoss of basicsr/losses/losses.py:300-313 (L1 mean between the stacked real / imaginary parts of
 * rfft2(pred) and rfft2(target); options/train_wavemamba_uhdll.yml:102-104 weights it by 0.1, `fft_opt`) - csrc/fft_loss.hip.h.
 * rfft2 is linear: d = a - b is taken in fp32 first and transformed ONCE, and no spectrum exists as a tensor.
 * a, b: `planes` (= B C) dense fp32 planes of H x W, 16-byte aligned; H and W powers of two in [16, 1024]; K = W / 2 + 1.
 *   Y[k1, k2] = sum d[n1, n2] exp(-2 pi i (k1 n1 / H + k2 n2 / W)), k2 < K;  out[0] = sum(|Re Y| + |Im Y|) / M, M = planes H K 2
 *   ga[n1, n2] = gout[0] / M * Re sum_{k1, k2 < K} s[k1, k2] exp(+2 pi i (k1 n1 / H + k2 n2 / W)), s = sign(Re Y) + i sign(Im Y),
 *   sign(0) = 0 (the half spectrum only, no Hermitian doubling, no 1 / HW: autograd's gradient of the reference composition); the
 *   imaginary sign of the four self-conjugate bins (k1 in {0, H / 2}, k2 in {0, W / 2}) counts as 0.  gb = -ga.
 *   wm_fft_l1_supported: 1 when H and W are powers of two in [16, 1024], else 0.
 *   wm_fft_l1_record_bytes: what forward leaves for backward (one byte per bin); wm_fft_l1_workspace_bytes: the workgroups' float64
 *     partial sums and one complex fp32 half spectrum of the difference, the same size for both directions.  Both 0 for an
 *     unsupported shape (WM_EUNSUPPORTED from the launching entries: a size that is no power of two in [16, 1024], or more planes
 *     than one launch holds - 2^24 - 1 workgroups).  The workspace is 16-byte aligned and written before it is read.
 *   wm_fft_l1_mean_fwd: three launches; per-workgroup sums in float64, added in a fixed order by a kernel that OVERWRITES out: no
 *     atomics, no memset, bit-identical run to run.  record: wm_fft_l1_record_bytes bytes, or NULL for the value alone.
 *   wm_fft_l1_mean_bwd: two launches; gout one device float (read on the device); ga and / or gb (NULL: not wanted; 16-byte
 *     aligned).  The record is only read: a second backward from it gives the same bits.
 * No host synchronisation, no allocation: everything runs on `stream` and can be captured into a graph. */
int wm_fft_l1_supported(int H, int W);
size_t wm_fft_l1_record_bytes(int64_t planes, int H, int W);
size_t wm_fft_l1_workspace_bytes(int64_t planes, int H, int W);
int wm_fft_l1_mean_fwd(const float* a, const float* b, float* out, void* record, void* workspace, size_t workspace_bytes,
                       int64_t planes, int H, int W, void* stream);
int wm_fft_l1_mean_bwd(const void* record, const float* gout, float* ga, float* gb, void* workspace, size_t workspace_bytes,
                       int64_t planes, int H, int W, void* stream);

/* Image-quality metrics of the reference's evaluation loop (inference_wavemamba.py:116-117, :133-134 -> comput_psnr_ssim.py with
 * crop_border, input_order 'HWC' / 'CHW', test_y_channel = True), csrc/metrics.hip.h.
 *   Images: N uint8 images of H x W x 3, element (n, h, w, ch) at n sn + h sh + w sw + ch sc (strides in elements, >= 0: HWC and
 *   CHW alike); bgr = 1: channel 0 is blue (cv2.imread / tensor2img), bgr = 0: channel 0 is red.  a and b share the strides.
 *   Y (to_y_channel :374-385 -> bgr2ycbcr :210-237, bit for bit): x = float32(u8) / 255 in float32,
 *     y64 = ((x_b 24.966 + x_g 128.553) + x_r 65.481) + 16 in float64, Y = float32(float32(y64 / 255) * 255).
 *   wm_psnr_ssim_y_u8: crop [crop, H - crop) x [crop, W - crop) (:426-428, :642-644; crop 0 = none), then per image
 *     out[2 n] = PSNR = 20 log10(255 / sqrt(mse)) (:430-438; +inf when mse = 0; mse in float64 - the reference's is float32),
 *     out[2 n + 1] = SSIM = mean of _ssim_cly's map (:558-593: 11 x 11 Gaussian of sigma 1.5, BORDER_REPLICATE, float64).
 *     out: N x 2 doubles, 8-byte aligned.  workspace: wm_psnr_ssim_y_workspace_bytes(N, H, W, crop) bytes, 8-byte aligned; every
 *     byte of it that is read is written first in the same call (nothing needs zeroing).  Deterministic (fixed summation order, no
 *     atomics).  WM_EINVAL when crop < 0 or crop >= min(H, W) / 2 (nothing left to measure); workspace_bytes is then 0.
 *   wm_y_channel_u8: y (N, H, W) float32 dense = Y of every pixel (no crop). */
size_t wm_psnr_ssim_y_workspace_bytes(int N, int H, int W, int crop);
int wm_psnr_ssim_y_u8(const uint8_t* a, const uint8_t* b, int64_t sn, int64_t sh, int64_t sw, int64_t sc, int N, int H, int W,
                      int crop, int bgr, double* out, void* workspace, size_t workspace_bytes, void* stream);
int wm_y_channel_u8(const uint8_t* img, int64_t sn, int64_t sh, int64_t sw, int64_t sc, int N, int H, int W, int bgr, float* y,
                    void* stream);

/* sums (C) = sum over batch and plane of x (B, C, H, W): the bias gradient of a convolution (training). */
int wm_plane_sums(const float* x, float* sums, int B, int C, int H, int W, void* stream);

/* --------------------------------------------------------------------------------------------
 * Element-wise gates and scaled skips of the LFSSBlock TRAINING path, forward and backward:
 *   wm_gate_fwd:      out = act(a) * b          act 1 = SiLU  (SS2D: y * F.silu(z),           wavemamba_arch.py:493)
 *                                               act 2 = GELU  (ffn:  F.gelu(x1) * x2, erf form, :228-229)
 *                                               act 3 = sigmoid (PAConv: k3(x) * sigmoid(k2(x)), :697-699)
 *   wm_gate_bwd:      ga = g * b * act'(a),  gb = g * act(a)
 *   wm_scale_add_fwd: out = x * scale[c] + o    (LFSSBlock: input * skip_scale + ..., x * skip_scale2 + ..., :525-526)
 *   wm_scale_add_bwd: gx = g * scale[c],  gscale[c] = sum_{b, p} g * x   (zeroed here, accumulated with one atomic per block)
 * Gate operands are (B, per_b) fp32 with batch strides in elements, so the two halves of a channel chunk are passed as
 * views; scale_add operands are dense (B, C, L).  16-byte accesses when sizes / strides / pointers allow, scalar otherwise.
 */
int wm_gate_fwd(const float* a, const float* b, float* out, int act, int B, int64_t per_b, int64_t stride_a, int64_t stride_b,
                int64_t stride_out, void* stream);
int wm_gate_bwd(const float* a, const float* b, const float* g, float* ga, float* gb, int act, int B, int64_t per_b,
                int64_t stride_a, int64_t stride_b, int64_t stride_g, int64_t stride_ga, int64_t stride_gb, void* stream);
int wm_scale_add_fwd(const float* x, const float* scale, const float* o, float* out, int B, int C, int64_t L, void* stream);
int wm_scale_add_bwd(const float* g, const float* x, const float* scale, float* gx, float* gscale, int B, int C, int64_t L,
                     void* stream);

/* Small-tensor steps of the HFE branch as single kernels (csrc/hfe.hip.h).  Forward only.
 *   wm_match_index   channel matching with every channel kept (wavemamba_arch.py:659-666, match_factor = 1):
 *                    index[b, c] = argmin_j (nx[b, c] + ny[b, j] - 2 G[b, c, j]) from wm_gram_fwd's outputs; (B, C) int32.
 *   wm_attn_fold     transposed attention folded into its output projection (:787-797): Wout[b] (C, C) =
 *                    Wpo (C, C) @ blockdiag_h softmax_j(G[b, h] / (max(|q_i|, 1e-12) max(|k_j|, 1e-12)) * temperature[h]);
 *                    G (B * heads, C / heads, C / heads), nq / nk (B * heads, C / heads) squared norms.  C <= 64.
 *                    project_out(attn @ v) is then the 1x1 convolution of v with Wout[b] (+ project_out's bias).
 *   wm_skff_fwd      SKFF of three sub-bands (:937-959): out = sum_i softmax_i(Wfc[i] prelu(Wdu mean(x0 + x1 + x2))) x_i.
 *                    x_i, out (B, C, H, W); Wdu (d, C); prelu (1); Wfc (3, C, d); C <= 64, d <= 16; workspace
 *                    wm_skff_workspace_bytes(B, C) bytes. */
int wm_match_index(const float* G, const float* nx, const float* ny, int* index, int B, int C, void* stream);
int wm_attn_fold(const float* G, const float* nq, const float* nk, const float* temperature, const float* Wpo,
                 float* Wout, int B, int C, int heads, void* stream);
size_t wm_skff_workspace_bytes(int B, int C);
int wm_skff_fwd(const float* x0, const float* x1, const float* x2, const float* Wdu, const float* prelu,
                const float* Wfc, float* out, void* workspace, size_t workspace_bytes, int B, int C, int d, int H, int W,
                void* stream);

/* The UNet's pixel-unshuffled image inputs, ps_down{1,2,3} = nn.Sequential(nn.PixelUnshuffle(r), nn.Conv2d(r*r*Cin, Cout, 1))
 * (wavemamba_arch.py:1014-1025, applied to the input image at :1043-1045), as one r x r / stride-r convolution read straight from
 * the image: y[b, o, yo, xo] = bias[o] + sum_{c,i,j} weight[o, (c r + i) r + j] * img[b, c, r yo + i, r xo + j].
 *   img (B, Cin, H, W) fp32, 16-byte aligned, H and W multiples of r; weight (Cout, Cin r r) = the Conv2d's (Cout, Cin r r, 1, 1);
 *   bias (Cout) or NULL; y (B, Cout, H / r, W / r) fp32.  r in {2, 4, 8}, Cout in {16, 32, 48, 64}, Cin r r Cout <= 16384
 *   (else WM_EUNSUPPORTED: callers keep the two modules).  fp32 FMAs in PixelUnshuffle's (c, i, j) channel order. */
int wm_patchify_conv_fwd(const float* img, const float* weight, const float* bias, float* y, int B, int Cin, int Cout, int H, int W,
                         int r, void* stream);

/* --------------------------------------------------------------------------------------------
 * Profiling hooks used by bench.py (HIP events recorded on the launch stream around each kernel
 * class).  Disabled by default; when disabled the library records nothing.
 *   kernel ids: 0 haar analysis (dwt fwd / iwt bwd), 1 haar synthesis (iwt fwd / dwt bwd),
 *               2 scan chunk-reduce, 3 scan carry, 4 scan chunk-scan (drop-in op), 5 wm_lfss_in_fwd,
 *               6 ss2d projection records (core backward), 7 depth-wise conv + SiLU (SS2D.conv2d), 8 ss2d core chunk-scan
 *               (+ the merged-output sum), 9 wm_lfss_mid_fwd, 10 ss2d core chunk-reduce (+ the parameter prep),
 *               11 wm_lfss_out_fwd / wm_lfss_out_conv_fwd, 12 selective-scan backward (all phases),
 *               13 dense 3x3 convolution, 14 1x1 convolution, 15 SKFF (all three kernels), 16 LayerNorm2d,
 *               17 depth-wise conv without SiLU (HFE branch, ffn), 18 wm_patchify_conv_fwd,
 *               19 the fixed-order finish of the wm_*_det entry points (one launch per deterministic call)
 * wm_prof_enable(mask): bit k of `mask` switches recording for kernel id k (0 = off, ~0u = every class);
 * a non-zero mask also clears what was recorded before.  Two hipEventRecord calls cost ~10 us of stream
 * time per launch, so a caller timing a whole step enables only the classes it needs.
 * wm_prof_collect synchronises the recorded events (host-blocking) and returns, per kernel id,
 * the number of launches and their summed duration in milliseconds since the last wm_prof_enable(mask != 0).
 * -------------------------------------------------------------------------------------------- */
#define WM_PROF_NKERNELS 20
void wm_prof_enable(unsigned mask);
int wm_prof_collect(int* launches /*[WM_PROF_NKERNELS]*/, double* total_ms /*[WM_PROF_NKERNELS]*/);

/* Zero-initialised accumulator outputs.  The entry points whose kernels ADD into an output with atomics - wm_dwconv3x3_wgrad
 * (dW, db), wm_layernorm2d_bwd and wm_layernorm_tok_bwd (dweight, dbias), wm_linear_wgrad (dW), wm_plane_sums (sums),
 * wm_scale_add_bwd (gscale), wm_conv2d_f16_steps (amax), wm_l1_mean_fwd (out) - zero that output first, on the stream, with a small
 * KERNEL (round 6; never hipMemsetAsync: captured into a HIP graph that is a memset node, and ROCm 7.0.2 fills with a pattern it
 * re-reads from recycled memory when the graph is launched again after eager work - profiles/r06/graph_memset_node.md).  A caller that
 * hands these buffers out of memory it has ALREADY zeroed (one memset for many buffers: the host side's bump arena,
 * ops._zeros_small) registers the range; a buffer lying entirely inside a registered range is then taken as zero and the launch is
 * skipped (a BASELINE config-3 training step had 323 of them, 1.4 ms of stream time).  The caller's contract: every buffer it
 * passes from a registered range is zero at that point of the stream (ONE-SHOT: a buffer that has been accumulated into is not zero
 * any more - passing it again, to this or another accumulate-into entry point, adds onto its old contents without any error; hand
 * every buffer out of the range once), and the range is unregistered before its memory is freed.
 * register: WM_EINVAL for an empty range or one that overlaps a registered range; unregister: WM_EINVAL for an unknown base.
 * Process-wide, thread-safe.  No reference counterpart (the reference's gradients come from ATen). */
int wm_zero_arena_register(void* base, size_t bytes);
int wm_zero_arena_unregister(void* base);

/* --------------------------------------------------------------------------------------------
 * Deterministic forms of the accumulate-into entry points above (the host side's deterministic training mode,
 * ops.set_deterministic / WM_DETERMINISTIC=1).  Each wm_<entry>_det computes what wm_<entry> computes - same arguments with
 * `workspace, workspace_bytes` inserted in front of the sizes, same kernels on the SAME grid - but no workgroup adds into the output:
 * every workgroup stores its partial sums as one record in the caller-owned workspace, and a finishing kernel (csrc/det.hip.h:
 * det_finish_kernel) adds the records of each output element in an order that depends on the shapes alone - S lanes per element
 * (S a power of two <= 64 chosen from the record width and count), lane s adding records s, s + S, ... in ascending order, then the
 * S lane sums in a butterfly.  The outputs are OVERWRITTEN: they need no zeroing, no zero arena, and a call captured into a HIP
 * graph holds no accumulator state.  Results are bit-identical run to run and differ from the atomic form's by summation order
 * only.  Reference counterpart: none (the reference's gradients come from ATen, whose own reductions are not ordered either).
 *   Workspace: wm_<entry>_det_workspace_bytes(sizes) bytes of uninitialised memory, every byte that is read written first in the
 *   same call; 0 for an empty or unsupported shape.  Records per output element (= the atomic form's adds per element):
 *     wm_dwconv3x3_wgrad_det     B x (workgroups per plane) records of 10 C floats [dW taps | db] (zero sums are stored too)
 *     wm_layernorm2d_bwd_det     min(512, ...) records of 2 C floats [dweight | dbias]; C >= 32 is the two-lanes-per-pixel kernel
 *     wm_layernorm_tok_bwd_det   min(1024, ...) records of 2 C floats
 *     wm_linear_wgrad_det        one record of O I floats per workgroup; inside a workgroup the eight waves add their tiles into the
 *                                LDS record one after the other instead of with LDS atomics
 *     wm_plane_sums_det          B x (blocks per plane) records of C floats
 *     wm_scale_add_bwd_det       B x (blocks per plane) records of C floats
 *     wm_l1_mean_fwd_det         one float per workgroup (at most 1024)
 *     wm_selscan_bwd_det         behind wm_selscan_bwd's own workspace: the finish kernel's (blocks per channel) x dim records of
 *                                N + 4 floats [dA | dD, dbias] and, when a group's channels are split over wpg > 1 workgroups
 *                                (dim / G > 64), wpg slabs each of dB and dC, stored plainly and added in ascending slice order
 *   Status: as the atomic entry, plus WM_ENULL for a NULL workspace, WM_EWORKSPACE for one that is too small and WM_EALIGN
 *   (wm_linear_wgrad_det, wm_selscan_bwd_det) for one that is not 16-byte aligned.  An empty problem zeroes the outputs (by a kernel).
 * -------------------------------------------------------------------------------------------- */
size_t wm_dwconv3x3_wgrad_det_workspace_bytes(int B, int C, int H, int W);
int wm_dwconv3x3_wgrad_det(const float* x, const float* gy, float* dW, float* db, void* workspace, size_t workspace_bytes, int B, int C,
                           int H, int W, void* stream);
size_t wm_layernorm2d_bwd_det_workspace_bytes(int B, int64_t L, int C);
int wm_layernorm2d_bwd_det(const float* x, const float* weight, const float* gy, float eps, float* gx, float* dweight, float* dbias,
                           void* workspace, size_t workspace_bytes, int B, int64_t L, int C, void* stream);
size_t wm_layernorm_tok_bwd_det_workspace_bytes(int64_t T, int C);
int wm_layernorm_tok_bwd_det(const float* x, const float* weight, const float* gy, float eps, float* gx, float* dweight, float* dbias,
                             void* workspace, size_t workspace_bytes, int64_t T, int C, void* stream);
size_t wm_linear_wgrad_det_workspace_bytes(int64_t T, int O, int I);
int wm_linear_wgrad_det(const float* gy, const float* x, float* dW, void* workspace, size_t workspace_bytes, int64_t T, int O, int I,
                        void* stream);
size_t wm_plane_sums_det_workspace_bytes(int B, int C, int H, int W);
int wm_plane_sums_det(const float* x, float* sums, void* workspace, size_t workspace_bytes, int B, int C, int H, int W, void* stream);
size_t wm_scale_add_bwd_det_workspace_bytes(int B, int C, int64_t L);
int wm_scale_add_bwd_det(const float* g, const float* x, const float* scale, float* gx, float* gscale, void* workspace,
                         size_t workspace_bytes, int B, int C, int64_t L, void* stream);
size_t wm_l1_mean_fwd_det_workspace_bytes(int64_t n);
int wm_l1_mean_fwd_det(const float* a, const float* b, float* out, void* workspace, size_t workspace_bytes, int64_t n, void* stream);
size_t wm_selscan_bwd_det_workspace_bytes(int batch, int dim, int L, int N, int G);
int wm_selscan_bwd_det(const float* u, const float* delta, const float* A, const float* Bm, const float* Cm, const float* D,
                       const float* delta_bias, const float* dy, float* du, float* ddelta, float* dA, float* dB, float* dC, float* dD,
                       float* dbias, void* workspace, size_t workspace_bytes, int batch, int dim, int L, int N, int G,
                       int delta_softplus, void* stream);

/* Channel gather with one index per (batch element, output channel) and its gradient (csrc/det.hip.h): the two gathers of the HFE
 * branch - Matching's matched candidate maps (wavemamba_arch.py:666) and PAConv's cat([x, matched]) (:713) - whose backward in the
 * reference is ATen's scatter-add (float atomics: the order of two sources of one channel is not fixed).
 *   wm_channel_gather_fwd   y[b, j, :] = x[b, index[b, j], :]          x (B, C, HW), index (B, M) int32, y (B, M, HW); bit for bit
 *                           torch.gather.  An index outside [0, C) yields a zero plane (the host cannot check a device index).
 *   wm_channel_gather_bwd   gx[b, c, :] = sum over j with index[b, j] == c of gy[b, j, :], added in ASCENDING j starting from 0;
 *                           a channel no index names is zero.  gx (B, C, HW) is overwritten (no zeroing, no atomics): one
 *                           workgroup per (plane segment, c, b) lists the sources of c and adds their planes, so gy is read once.
 * fp32, dense; HW = the plane size (H W for NCHW maps, the last axis of (B, C, HW) token maps).  HW % 4 == 0 with 16-byte aligned
 * planes: 16-byte accesses; otherwise element-wise.  No workspace.  WM_EINVAL: a negative size, or C == 0 with something to gather;
 * WM_ENULL; WM_EALIGN: a pointer not 4-byte aligned; WM_EUNSUPPORTED: B or the grid's channel axis > 65535, M > 1024 (backward). */
int wm_channel_gather_fwd(const float* x, const int* index, float* y, int B, int C, int M, int64_t HW, void* stream);
int wm_channel_gather_bwd(const float* gy, const int* index, float* gx, int B, int C, int M, int64_t HW, void* stream);

/* --------------------------------------------------------------------------------------------
 * Guarded optimizer step (csrc/grad_guard.hip.h): the global L2 norm of a set of fp32 gradients, a non-finite flag and the clipping
 * divisor, left on the device for the optimizer launch that follows on the same stream - torch's fused AdamW reads them as
 * `found_inf` and `grad_scale` - so a step captured into a HIP graph can skip itself and clip without the host.  Reference
 * counterpart: none (femasr_model.py:157-185 steps unconditionally); the divisor is torch.nn.utils.clip_grad_norm_'s coefficient,
 * inverted.  (Added to ABI 34 like the _det forms: no existing signature changes.)
 *   table    n_rows rows {int64 address, int64 count} in DEVICE memory: each a run of `count` >= 0 contiguous floats starting at
 *            any 4-byte boundary.  The host splits a tensor into runs of at most 4096 floats (one workgroup per row; a longer run
 *            is summed correctly, by one workgroup); a run never spans two tensors.
 *   record   4 floats, OVERWRITTEN: {norm, found_inf, grad_scale, 0}
 *              norm       = (float) sqrt(sum of squares), every square and every add in double (1e19 and 1e-30 both survive)
 *              found_inf  = 1 if any element has all exponent bits set (inf, NaN - tested on the bit pattern) or norm is not
 *                           finite in fp32 (finite elements can overflow it), else 0
 *              grad_scale = max(1, (norm + 1e-6f) / max_norm) in fp32 when max_norm is finite and > 0 and found_inf == 0, else 1
 *   skipped  one int64 (may be NULL): skipped[0] += found_inf, a plain read-modify-write by one thread
 *   ws       wm_grad_guard_workspace_bytes(n_rows) bytes (16 per row; 0 for no rows), uninitialised: one {double, flag} per row is
 *            written by its workgroup and read by the finishing workgroup, which adds the rows in an order fixed by n_rows.
 * No atomics, no memset: bit-identical run to run, and nothing is assumed about what ws or record held.
 * Status, by host arithmetic before any launch: WM_EINVAL n_rows < 0; WM_ENULL record; n_rows == 0 then writes {0, 0, 1, 0} (one
 * launch); WM_ENULL table or ws; WM_EWORKSPACE; WM_EUNSUPPORTED n_rows >= 2^31; WM_EALIGN table, ws or skipped not 8-byte, record
 * not 4-byte aligned.
 * -------------------------------------------------------------------------------------------- */
size_t wm_grad_guard_workspace_bytes(int64_t n_rows);
int wm_grad_guard(const void* table, int64_t n_rows, float max_norm, float* record, int64_t* skipped, void* ws, size_t ws_bytes,
                  void* stream);

/* --------------------------------------------------------------------------------------------
 * Table-driven AdamW step with the weights' exponential moving average (csrc/adamw.hip.h): torch.optim.AdamW (amsgrad = False,
 * maximize = False) on fp32 tensors named by a device table, and - for rows that carry an ema address - the reference's model_ema
 * (base_model.py:85-92) in the same pass.  Nothing of a step is decided on the host, so a launch captured into a HIP graph follows
 * a learning-rate schedule and the guard above.  (Added to ABI 34: no existing signature changes.)
 *   table      n_rows rows of six int64 in DEVICE memory: {param, grad, exp_avg, exp_avg_sq, ema or 0, count}, each address a run of
 *              `count` contiguous floats; the host gives a row at most 4096 floats (one workgroup of 256 per row; a longer row is
 *              still updated correctly) and no row spans two tensors.  A row whose addresses all lie on 16-byte boundaries runs on
 *              16-byte accesses with a scalar tail; any other row (gradient views packed back to back) element by element.
 *   lr         one float, DEVICE.    step   one float, DEVICE: the number of steps taken; this step is t = step + 1.
 *   hyper      five doubles in HOST memory, read before the launch: {beta1, beta2, eps, weight_decay, ema_decay}; they become
 *              launch scalars - constants of a run, and of a captured graph.  ema_decay is used by rows with an ema address.
 *   found_inf  one float, DEVICE, or NULL: != 0 -> nothing is written - parameters, moments, averages and `step` stay bit-equal.
 *   grad_scale one float, DEVICE, or NULL: g = grad / grad_scale.  The divided gradient is NOT written back.
 * Per element, every operation rounded to fp32 on its own, the scalars rounded to fp32 once from double (1 - beta^t in double):
 *   p *= 1 - lr wd;  m = fma(1 - beta1, g - m, m);  v = v beta2 + ((1 - beta2) g) g;
 *   p += (-(lr / (1 - beta1^t)) m) / (sqrt(v) / sqrt(1 - beta2^t) + eps);  ema = ema d + (1 - d) p
 * Two launches: the update, then one lane's step += 1 (unless found_inf).  No atomics, no memset: bit-identical run to run.
 * Status, by host arithmetic before any launch: WM_EINVAL n_rows < 0; n_rows == 0 is WM_OK (nothing runs); WM_ENULL table, hyper, lr
 * or step; WM_EUNSUPPORTED n_rows >= 2^31; WM_EALIGN table not 8-byte, a float pointer not 4-byte aligned; WM_EINVAL a beta or the
 * ema decay outside [0, 1), eps or weight_decay negative.
 * -------------------------------------------------------------------------------------------- */
int wm_adamw_step(const void* table, int64_t n_rows, const float* lr, float* step, const double* hyper, const float* found_inf,
                  const float* grad_scale, void* stream);

/* Host-blocking wait for `event` (a hipEvent_t recorded OUTSIDE any capture) that is legal while a stream of this
 * thread is being captured: hipEventSynchronize under a thread-local relaxed capture mode
 * (hipThreadExchangeStreamCaptureMode), restored before returning.  The host side uses it for a prepared-weight buffer
 * whose preparation kernel ran on another stream before the capture began: an uncaptured event cannot be waited for by a
 * capturing stream, and a plain hipEventSynchronize invalidates a capture in the global mode (torch.cuda.graph's
 * default).  No reference counterpart (the reference has no graph capture). */
int wm_event_synchronize_relaxed(void* event);

#ifdef __cplusplus
}
#endif
#endif /* WAVEMAMBA_HIP_H */
