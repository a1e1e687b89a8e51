// haar_image.hip - C ABI over the Haar transforms, uint8 image I/O, training-batch formation, the L1 and SSIM losses and the
// image-quality metrics.
#include <initializer_list>
#include "host_common.h"
#include "haar.hip.h"
#include "imageio.hip.h"
#include "images_io.hip.h"
#include "loss.hip.h"
#include "metrics.hip.h"
#include "patch_batch.hip.h"
#include "ssim_loss.hip.h"

namespace wm {

// ------------------------------------------------------------------------------------------------
// Haar launchers
// ------------------------------------------------------------------------------------------------
template <typename Tf, typename Ts, bool ROUND>
static int launch_analysis(const void* full, void* s0, void* s1, void* s2, void* s3, const HaarGeom& g,
                           bool vec, hipStream_t st) {
    const dim3 block(64, 4);
    const int cols = vec ? (g.w + 3) / 4 : g.w;
    const dim3 grid((unsigned)((g.rows + 3) / 4), (unsigned)((cols + 63) / 64));
    if (vec)
        hipLaunchKernelGGL((haar_analysis_kernel<Tf, Ts, ROUND, true>), grid, block, 0, st,
                           (const Tf*)full, (Ts*)s0, (Ts*)s1, (Ts*)s2, (Ts*)s3, g);
    else
        hipLaunchKernelGGL((haar_analysis_kernel<Tf, Ts, ROUND, false>), grid, block, 0, st,
                           (const Tf*)full, (Ts*)s0, (Ts*)s1, (Ts*)s2, (Ts*)s3, g);
    return launch_status();
}
template <typename Ts, typename Tf, bool ROUND>
static int launch_synthesis(const void* s0, const void* s1, const void* s2, const void* s3, void* full,
                            const HaarGeom& g, bool vec, hipStream_t st) {
    const dim3 block(64, 4);
    const int cols = vec ? (g.w + 3) / 4 : g.w;
    const dim3 grid((unsigned)((g.rows + 3) / 4), (unsigned)((cols + 63) / 64));
    if (vec)
        hipLaunchKernelGGL((haar_synthesis_kernel<Ts, Tf, ROUND, true>), grid, block, 0, st,
                           (const Ts*)s0, (const Ts*)s1, (const Ts*)s2, (const Ts*)s3, (Tf*)full, g);
    else
        hipLaunchKernelGGL((haar_synthesis_kernel<Ts, Tf, ROUND, false>), grid, block, 0, st,
                           (const Ts*)s0, (const Ts*)s1, (const Ts*)s2, (const Ts*)s3, (Tf*)full, g);
    return launch_status();
}

static int haar_geom(HaarGeom& g, int B, int C, int h, int w, int64_t b0, int64_t b1, int64_t b2,
                     int64_t b3) {
    if (B < 0 || C < 0 || h < 0 || w < 0) return WM_EINVAL;
    g.C = C; g.h = h; g.w = w; g.rows = (long long)B * C * h;
    g.bs[0] = b0; g.bs[1] = b1; g.bs[2] = b2; g.bs[3] = b3;
    if ((g.rows + 3) / 4 > 0x7fffffffLL) return WM_EINVAL;
    return WM_OK;
}
// vector path: 4 sub-band columns per thread, every row start / stride 16-byte aligned on the
// full-res side and 16 B (fp32) / 8 B (bf16) aligned on the sub-band side
static bool haar_vec_ok(const HaarGeom& g, const void* full, const void* const s[4]) {
    if (g.w % 4 != 0) return false;
    if (!aligned16(full)) return false;
    for (int k = 0; k < 4; ++k)
        if (!aligned16(s[k]) || (g.bs[k] % 4) != 0) return false;
    return true;
}

}  // namespace wm

using namespace wm;

// ================================================================================================
// Image-quality metrics (csrc/metrics.hip.h): Y-channel PSNR / SSIM of uint8 image pairs, and the Y plane alone
// ================================================================================================
static bool met_image(MetImage& im, int64_t sn, int64_t sh, int64_t sw, int64_t sc, int bgr) {
    if (sn < 0 || sh < 0 || sw < 0 || sc < 0) return false;
    im = MetImage{(long long)sn, (long long)sh, (long long)sw, (long long)sc, bgr ? 0 : 2, bgr ? 2 : 0};
    return true;
}

static bool met_window(int N, int H, int W, int crop, int& Hc, int& Wc) {
    if (N < 1 || H < 1 || W < 1 || crop < 0 || N > 65535) return false;
    Hc = H - 2 * crop;
    Wc = W - 2 * crop;
    return Hc >= 1 && Wc >= 1;                         // crop >= min(H, W) / 2 leaves nothing to measure
}

// ================================================================================================
// SSIM training loss (csrc/ssim_loss.hip.h)
// ================================================================================================
// The 1-D window exactly as cal_ssim.py:7-9 has it: exp(-(i - 5)^2 / 4.5) evaluated and normalised in float32 by torch
// (taps 0..5; the window is symmetric).  Constants, not arithmetic: the float32 sum these were divided by depends on torch's
// summation order (a sequential sum differs in the last bit), and a last bit of the window's sum is 1e-4 of B2 on a flat
// bright region (see the header of ssim_loss.hip.h).  tests/test_ssim_loss_cpu.py holds cpu_twin.ssim_window_1d() to them.
static const float SL_TAPS_F32[6] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f};

static SlGauss sl_window() {
    SlGauss gw;
    for (int i = 0; i < SL_TAPS; ++i) gw.g[i] = (double)SL_TAPS_F32[i <= 5 ? i : SL_TAPS - 1 - i];
    return gw;
}

// tiles of every plane folded into grid.x (any plane count); WM_EINVAL for an empty shape, WM_EUNSUPPORTED when the grid would
// not fit: a launch holds fewer than 2^32 threads in all, 2^24 - 1 workgroups of 256 (SL_MAX_TILES; 12.9e9 pixels)
static const long long SL_MAX_TILES = (1LL << 24) - 1;

static int sl_geom(int64_t planes, int H, int W, SlGeom& gm, long long& blocks) {
    if (planes < 1 || H < 1 || W < 1) return WM_EINVAL;
    gm.H = H; gm.W = W;
    gm.tilesX = (W + SL_TW - 1) / SL_TW;
    gm.tilesY = (H + SL_TH - 1) / SL_TH;
    const long long per_plane = (long long)gm.tilesX * gm.tilesY;
    if (per_plane > SL_MAX_TILES || planes > SL_MAX_TILES / per_plane) return WM_EUNSUPPORTED;
    blocks = (long long)planes * per_plane;
    gm.vec = 0;
    return WM_OK;
}

// 16-byte staging loads: W a multiple of 4 (then so is every row's and plane's offset) and each staged base 16-byte aligned
static int sl_vec(int W, std::initializer_list<const float*> staged) {
    if (W % 4 != 0) return 0;
    for (const float* p : staged)
        if (reinterpret_cast<uintptr_t>(p) & 15u) return 0;
    return 1;
}

extern "C" {

int wm_dwt2d_fwd(const void* x, void* ll, void* hl, void* lh, void* hh, int B, int C, int H, int W,
                 int dtype, void* stream) {
    if (H % 2 != 0 || W % 2 != 0) return WM_EINVAL;        // reference: RuntimeError on odd sizes
    HaarGeom g;
    const int64_t bs = (int64_t)C * (H / 2) * (W / 2);
    int rc = haar_geom(g, B, C, H / 2, W / 2, bs, bs, bs, bs);
    if (rc) return rc;
    if (g.rows == 0 || g.w == 0) return WM_OK;
    if (!x || !ll || !hl || !lh || !hh) return WM_ENULL;
    const void* s[4] = {ll, hl, lh, hh};
    const bool vec = haar_vec_ok(g, x, s);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(0, st);
    if (dtype == WM_F32) return launch_analysis<float, float, false>(x, ll, hl, lh, hh, g, vec, st);
    if (dtype == WM_BF16) return launch_analysis<bf16_t, bf16_t, true>(x, ll, hl, lh, hh, g, vec, st);
    return WM_EUNSUPPORTED;
}

int wm_dwt2d_bwd(const void* dll, const void* dhl, const void* dlh, const void* dhh, void* dx, int B,
                 int C, int H, int W, int dtype, void* stream) {
    if (H % 2 != 0 || W % 2 != 0) return WM_EINVAL;
    HaarGeom g;
    const int64_t bs = (int64_t)C * (H / 2) * (W / 2);
    int rc = haar_geom(g, B, C, H / 2, W / 2, bs, bs, bs, bs);
    if (rc) return rc;
    if (g.rows == 0 || g.w == 0) return WM_OK;
    if (!dx || !dll || !dhl || !dlh || !dhh) return WM_ENULL;
    const void* s[4] = {dll, dhl, dlh, dhh};
    const bool vec = haar_vec_ok(g, dx, s);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(1, st);
    // the 2x2 Haar matrix (with the 1/2 scaling) is orthogonal: d(analysis) = synthesis
    if (dtype == WM_F32) return launch_synthesis<float, float, false>(dll, dhl, dlh, dhh, dx, g, vec, st);
    if (dtype == WM_BF16) return launch_synthesis<bf16_t, bf16_t, false>(dll, dhl, dlh, dhh, dx, g, vec, st);
    return WM_EUNSUPPORTED;
}

int wm_idwt2d_fwd(const void* x1, const void* x2, const void* x3, const void* x4, int64_t bs1,
                  int64_t bs2, int64_t bs3, int64_t bs4, float* out, int B, int C, int h, int w,
                  int dtype, void* stream) {
    HaarGeom g;
    int rc = haar_geom(g, B, C, h, w, bs1, bs2, bs3, bs4);
    if (rc) return rc;
    if (g.rows == 0 || g.w == 0) return WM_OK;
    if (!x1 || !x2 || !x3 || !x4 || !out) return WM_ENULL;
    const void* s[4] = {x1, x2, x3, x4};
    const bool vec = haar_vec_ok(g, out, s);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(1, st);
    if (dtype == WM_F32) return launch_synthesis<float, float, false>(x1, x2, x3, x4, out, g, vec, st);
    if (dtype == WM_BF16) return launch_synthesis<bf16_t, float, true>(x1, x2, x3, x4, out, g, vec, st);
    return WM_EUNSUPPORTED;
}

int wm_idwt2d_bwd(const float* dout, void* d1, void* d2, void* d3, void* d4, int64_t bs1, int64_t bs2,
                  int64_t bs3, int64_t bs4, int B, int C, int h, int w, int dtype, void* stream) {
    HaarGeom g;
    int rc = haar_geom(g, B, C, h, w, bs1, bs2, bs3, bs4);
    if (rc) return rc;
    if (g.rows == 0 || g.w == 0) return WM_OK;
    if (!dout || !d1 || !d2 || !d3 || !d4) return WM_ENULL;
    const void* s[4] = {d1, d2, d3, d4};
    const bool vec = haar_vec_ok(g, dout, s);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(0, st);
    if (dtype == WM_F32) return launch_analysis<float, float, false>(dout, d1, d2, d3, d4, g, vec, st);
    if (dtype == WM_BF16) return launch_analysis<float, bf16_t, false>(dout, d1, d2, d3, d4, g, vec, st);
    return WM_EUNSUPPORTED;
}

int wm_image_pre_u8(const uint8_t* image, float* out, int h, int w, int Hp, int Wp, int swap_rb, void* stream) {
    if (h < 0 || w < 0 || Hp < h || Wp < w) return WM_EINVAL;
    if (Hp == 0 || Wp == 0) return WM_OK;
    if (h == 0 || w == 0) return WM_EINVAL;
    if (Hp - h > h - 1 || Wp - w > w - 1) return WM_EINVAL;            // reflect padding needs pad < size
    if (!image || !out) return WM_ENULL;
    if (Hp > 65535) return WM_EUNSUPPORTED;
    hipLaunchKernelGGL(image_pre_kernel, dim3((unsigned)((Wp + 255) / 256), (unsigned)Hp), dim3(256), 0, (hipStream_t)stream,
                       image, out, h, w, Hp, Wp, swap_rb);
    return launch_status();
}

int wm_image_post_u8(const float* in, uint8_t* image, int h, int w, int Hp, int Wp, int swap_rb, void* stream) {
    if (h < 0 || w < 0 || Hp < h || Wp < w) return WM_EINVAL;
    if (h == 0 || w == 0) return WM_OK;
    if (!in || !image) return WM_ENULL;
    if (h > 65535) return WM_EUNSUPPORTED;
    hipLaunchKernelGGL(image_post_kernel, dim3((unsigned)((w + 255) / 256), (unsigned)h), dim3(256), 0, (hipStream_t)stream,
                       in, image, h, w, Hp, Wp, swap_rb);
    return launch_status();
}

// N images per launch from a device table (csrc/images_io.hip.h).  The limits are those of the single-image kernels above and of the
// metrics: at most 65535 rows of pixels (Hp, the largest destination's h) and 65535 images (grid.y of wm_image_pre_u8 /
// wm_image_post_u8, grid.z of wm_psnr_ssim_y_u8), and at most 65535 * 32 columns.
static bool io_extent_ok(int n, int rows, int cols) { return n <= 65535 && rows <= 65535 && cols <= 65535 * IO_TILE; }

int wm_images_pre_u8(const int64_t* table, float* out, int N, int Hp, int Wp, int swap_rb, void* stream) {
    if (N < 0 || Hp < 0 || Wp < 0) return WM_EINVAL;
    if (N == 0 || Hp == 0 || Wp == 0) return WM_OK;
    if (!table || !out) return WM_ENULL;
    if ((reinterpret_cast<uintptr_t>(table) & 7u) || (reinterpret_cast<uintptr_t>(out) & 3u)) return WM_EALIGN;
    if (!io_extent_ok(N, Hp, Wp)) return WM_EUNSUPPORTED;
    static_assert(sizeof(long long) == sizeof(int64_t), "the table's fields are read as long long");
    hipLaunchKernelGGL(images_pre_kernel, dim3((unsigned)((Wp + IO_TILE - 1) / IO_TILE), (unsigned)((Hp + IO_TILE - 1) / IO_TILE), (unsigned)N),
                       dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const long long*>(table), out, Hp, Wp, swap_rb);
    return launch_status();
}

int wm_images_post_u8(const int64_t* table, const float* src0, int N0, int Hp0, int Wp0, const float* src1, int N1, int Hp1, int Wp1,
                      int rows, int h_max, int w_max, int swap_rb, void* stream) {
    if (rows < 0 || h_max < 0 || w_max < 0 || N0 < 0 || Hp0 < 0 || Wp0 < 0 || N1 < 0 || Hp1 < 0 || Wp1 < 0) return WM_EINVAL;
    if (rows == 0 || h_max == 0 || w_max == 0) return WM_OK;
    if (!table || !src0 || (N1 > 0 && !src1)) return WM_ENULL;
    if ((reinterpret_cast<uintptr_t>(table) & 7u) || ((reinterpret_cast<uintptr_t>(src0) | reinterpret_cast<uintptr_t>(src1)) & 3u)) return WM_EALIGN;
    if (!io_extent_ok(rows, h_max, w_max)) return WM_EUNSUPPORTED;
    const IoSource s0{src0, N0, Hp0, Wp0}, s1{N1 > 0 ? src1 : nullptr, N1, Hp1, Wp1};
    hipLaunchKernelGGL(images_post_kernel, dim3((unsigned)((w_max + IO_TILE - 1) / IO_TILE), (unsigned)((h_max + IO_TILE - 1) / IO_TILE), (unsigned)rows),
                       dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const long long*>(table), s0, s1, swap_rb);
    return launch_status();
}

// tiles of every sample's two images folded into grid.x; the same launch bound as the SSIM loss (SL_MAX_TILES workgroups of 256)
int wm_paired_patches_u8(const int64_t* table, float* lq, float* gt, int B, int P, int swap_rb, void* stream) {
    if (B < 0 || P <= 0) return WM_EINVAL;
    if (B == 0) return WM_OK;
    if (!table || !lq || !gt) return WM_ENULL;
    if ((reinterpret_cast<uintptr_t>(table) & 7u) || ((reinterpret_cast<uintptr_t>(lq) | reinterpret_cast<uintptr_t>(gt)) & 3u)) return WM_EALIGN;
    const long long tiles = ((long long)P + PB_TILE - 1) / PB_TILE;
    if (tiles * tiles > SL_MAX_TILES || 2LL * B > SL_MAX_TILES / (tiles * tiles)) return WM_EUNSUPPORTED;
    static_assert(sizeof(long long) == sizeof(int64_t), "the table's fields are read as long long");
    hipLaunchKernelGGL(paired_patches_kernel, dim3((unsigned)(tiles * tiles * 2 * B)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const long long*>(table), lq, gt, P, (int)tiles, swap_rb);
    return launch_status();
}

// mean |a - b| over n elements -> out[0] (zeroed here, by a kernel); ga = gout[0] * sign(a - b) / n
int wm_l1_mean_fwd(const float* a, const float* b, float* out, int64_t n, void* stream) {
    if (n < 0) return WM_EINVAL;
    if (!out) return WM_ENULL;
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = zero_out(out, sizeof(float), st);
    if (e != hipSuccess) return (int)e;
    if (n == 0) return WM_OK;                                     // (torch returns nan for an empty mean; callers never ask)
    if (!a || !b) return WM_ENULL;
    const int vec = (n % 4 == 0) && aligned16(a) && aligned16(b) ? 1 : 0;
    long long blocks = ((vec ? n / 4 : n) + 256 * 8 - 1) / (256 * 8);
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(l1_mean_fwd_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, a, b, out, (long long)n, 1.0f / (float)n, vec);
    return launch_status();
}
size_t wm_l1_mean_fwd_det_workspace_bytes(int64_t n) { return n > 0 ? 1024 * sizeof(float) : 0; }    // one float per workgroup
int wm_l1_mean_fwd_det(const float* a, const float* b, float* out, void* workspace, size_t workspace_bytes, int64_t n, void* stream) {
    if (n < 0) return WM_EINVAL;
    if (!out) return WM_ENULL;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        const hipError_t e = zero_out(out, sizeof(float), st);
        return e == hipSuccess ? WM_OK : (int)e;
    }
    if (!a || !b || !workspace) return WM_ENULL;
    if (workspace_bytes < wm_l1_mean_fwd_det_workspace_bytes(n)) return WM_EWORKSPACE;
    const int vec = (n % 4 == 0) && aligned16(a) && aligned16(b) ? 1 : 0;
    long long blocks = ((vec ? n / 4 : n) + 256 * 8 - 1) / (256 * 8);
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    float* part = (float*)workspace;
    hipLaunchKernelGGL(l1_mean_fwd_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, a, b, part, (long long)n, 1.0f / (float)n, vec);
    return det_finish(part, blocks, 1, DetOut{out, nullptr, nullptr, kDetSplit, 1, 0, 0}, st);
}
int wm_l1_mean_bwd(const float* a, const float* b, const float* gout, float* ga, int64_t n, void* stream) {
    if (n < 0) return WM_EINVAL;
    if (n == 0) return WM_OK;
    if (!a || !b || !gout || !ga) return WM_ENULL;
    const int vec = (n % 4 == 0) && aligned16(a) && aligned16(b) && aligned16(ga) ? 1 : 0;
    long long blocks = ((vec ? n / 4 : n) + 256 * 4 - 1) / (256 * 4);
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(l1_mean_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, b, gout, ga, (long long)n,
                       1.0f / (float)n, vec);
    return launch_status();
}

size_t wm_ssim_workspace_bytes(int64_t planes, int H, int W) {
    SlGeom gm;
    long long blocks;
    if (sl_geom(planes, H, W, gm, blocks) != WM_OK) return 0;
    return (size_t)blocks * sizeof(double);
}

int wm_ssim_mean_fwd(const float* a, const float* b, float* out, float* p1, float* p2, float* q, float* r, void* workspace,
                     size_t workspace_bytes, int64_t planes, int H, int W, void* stream) {
    SlGeom gm;
    long long blocks;
    const int rc = sl_geom(planes, H, W, gm, blocks);
    if (rc) return rc;
    if (!a || !b || !out || !workspace) return WM_ENULL;
    if ((q == nullptr) != (r == nullptr) || ((p1 || p2) && !q)) return WM_ENULL;      // q and r come together, with p1 and / or p2
    if (q && !p1 && !p2) return WM_EINVAL;
    if (reinterpret_cast<uintptr_t>(workspace) & 7u) return WM_EALIGN;
    if (workspace_bytes < (size_t)blocks * sizeof(double)) return WM_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)workspace;
    gm.vec = sl_vec(W, {a, b});
    hipLaunchKernelGGL(ssim_loss_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, b, gm, sl_window(), p1, p2, q, r, part);
    const int rc2 = launch_status();
    if (rc2) return rc2;
    const double n = (double)planes * (double)H * (double)W;
    hipLaunchKernelGGL(ssim_loss_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)part, blocks, n, out);
    return launch_status();
}

int wm_ssim_mean_bwd(const float* x, const float* other, const float* p, const float* q, const float* r, const float* gout,
                     float* gx, int64_t planes, int H, int W, void* stream) {
    SlGeom gm;
    long long blocks;
    const int rc = sl_geom(planes, H, W, gm, blocks);
    if (rc) return rc;
    if (!x || !other || !p || !q || !r || !gout || !gx) return WM_ENULL;
    const double n = (double)planes * (double)H * (double)W;
    gm.vec = sl_vec(W, {p, q, r});
    hipLaunchKernelGGL(ssim_loss_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, other, p, q, r, gout, gx,
                       gm, sl_window(), 1.0 / n);
    return launch_status();
}

size_t wm_psnr_ssim_y_workspace_bytes(int N, int H, int W, int crop) {
    int Hc, Wc;
    if (!met_window(N, H, W, crop, Hc, Wc)) return 0;
    const size_t tiles = (size_t)((Wc + MET_TW - 1) / MET_TW) * (size_t)((Hc + MET_TH - 1) / MET_TH);
    return (size_t)N * tiles * 2 * sizeof(double);
}

int wm_psnr_ssim_y_u8(const uint8_t* a, const uint8_t* b, int64_t sn, int64_t sh, int64_t sw, int64_t sc, int N, int H, int W,
                      int crop, int bgr, double* out, void* workspace, size_t workspace_bytes, void* stream) {
    int Hc, Wc;
    MetImage im;
    if (!met_window(N, H, W, crop, Hc, Wc) || !met_image(im, sn, sh, sw, sc, bgr)) return WM_EINVAL;
    if (!a || !b || !out || !workspace) return WM_ENULL;
    if ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(workspace)) & 7u) return WM_EALIGN;
    if (workspace_bytes < wm_psnr_ssim_y_workspace_bytes(N, H, W, crop)) return WM_EWORKSPACE;
    MetGauss gw;                                           // cv2.getGaussianKernel(11, 1.5): exp(-(i - 5)^2 / (2 1.5^2)), normalised
    double sum = 0.0;
    for (int i = 0; i < MET_TAPS; ++i) {
        const double x = i - (MET_TAPS - 1) * 0.5;
        gw.g[i] = exp(-0.5 / (1.5 * 1.5) * x * x);
        sum += gw.g[i];
    }
    for (int i = 0; i < MET_TAPS; ++i) gw.g[i] *= 1.0 / sum;
    const int tx = (Wc + MET_TW - 1) / MET_TW, ty = (Hc + MET_TH - 1) / MET_TH;
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)workspace;
    hipLaunchKernelGGL(psnr_ssim_tile_kernel, dim3((unsigned)tx, (unsigned)ty, (unsigned)N), dim3(256), 0, st, a, b, im, crop, Hc, Wc,
                       gw, part);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(psnr_ssim_finish_kernel, dim3((unsigned)N), dim3(256), 0, st, (const double*)part, tx * ty, (double)Hc * Wc,
                       out);
    return launch_status();
}

int wm_y_channel_u8(const uint8_t* img, int64_t sn, int64_t sh, int64_t sw, int64_t sc, int N, int H, int W, int bgr, float* y,
                    void* stream) {
    int Hc, Wc;
    MetImage im;
    if (!met_window(N, H, W, 0, Hc, Wc) || !met_image(im, sn, sh, sw, sc, bgr)) return WM_EINVAL;
    if (!img || !y) return WM_ENULL;
    if (reinterpret_cast<uintptr_t>(y) & 3u) return WM_EALIGN;
    const long long total = (long long)N * H * W;
    long long blocks = (total + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(y_channel_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, img, im, H, W, total, y);
    return launch_status();
}

}  // extern "C"
