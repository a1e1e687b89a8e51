// lfss.hip - C ABI over the LFSS glue: depth-wise 3x3, the fused block kernels, LayerNorm, gates and scaled adds.
#include "host_common.h"
#include "dwconv.hip.h"
#include "lfss.hip.h"
#include "lfss_mfma.hip.h"
#include "gates.hip.h"

using namespace wm;

template <int V> using int_c = std::integral_constant<int, V>;

// A runtime channel count as a compile-time one: f(c) with c() == C for C among the widths the caller supports (WIDTHS: their sum, each
// a power of two); false when C is none of them.  Widths outside WIDTHS are not instantiated.
template <unsigned WIDTHS, typename F>
static bool with_channels(int C, F&& f) {
    if constexpr ((WIDTHS & 64u) != 0) if (C == 64) { f(int_c<64>{}); return true; }
    if constexpr ((WIDTHS & 32u) != 0) if (C == 32) { f(int_c<32>{}); return true; }
    if constexpr ((WIDTHS & 16u) != 0) if (C == 16) { f(int_c<16>{}); return true; }
    if constexpr ((WIDTHS & 8u) != 0) if (C == 8) { f(int_c<8>{}); return true; }
    return false;
}
// One thread per position of (B, L), 256 per workgroup, kernel class `prof_class`: launch(int_c<C>{}, grid, block, stream) for C among
// WIDTHS.  An empty problem is WM_OK whatever C is.
template <unsigned WIDTHS, typename F>
static int launch_per_position(int prof_class, int B, int64_t L, int C, void* stream, F&& launch) {
    const long long total = (long long)B * L;
    if (total == 0) return WM_OK;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(prof_class, st);
    if (!with_channels<WIDTHS>(C, [&](auto c) { launch(c, grid, block, st); })) return WM_EUNSUPPORTED;
    return launch_status();
}

// rows per strip of the depth-wise kernels (dwconv.hip.h): 16 (every input row fetched 18 / 16 times), or 8 / 4 on small problems - a strip is a chain of dependent row
// fetches, and 16-row strips of a 64 x 64 map are 128-384 workgroups for 256 compute units (21 us per weight-gradient launch at
// BASELINE config 3's level 3, whatever the lanes did)
static int dw_strip_rows(int H, long long column_blocks, long long plane_groups) {
    const long long waves16 = column_blocks * ((H + kDwRows - 1) / kDwRows) * plane_groups;
    return waves16 >= 2048 ? kDwRows : (waves16 >= 1024 ? 8 : 4);
}

// Launch geometry of the depth-wise kernels: `vec` (16-byte accesses), lanes per strip row, groups of planes that share a wave, rows
// per strip (short_strips: dw_strip_rows; otherwise kDwRows)
struct DwGeometry { bool vec; int lpr, rows; long long pgroups; dim3 grid, block; };
static DwGeometry dw_geometry(int H, int W, long long planes, bool vec, bool short_strips) {
    DwGeometry g;
    g.vec = vec;
    g.lpr = !vec || W > 128 ? 64 : (W > 64 ? 32 : 16);          // narrow maps put 2 / 4 planes side by side in a wave
    g.pgroups = (planes + 64 / g.lpr - 1) / (64 / g.lpr);
    g.block = dim3(64, 4);
    const long long column_blocks = (W + 4 * g.lpr - 1) / (4 * g.lpr);
    g.rows = short_strips ? dw_strip_rows(H, column_blocks, g.pgroups) : kDwRows;
    g.grid = dim3((unsigned)column_blocks, (unsigned)((H + 4 * g.rows - 1) / (4 * g.rows)), (unsigned)(g.pgroups < 65535 ? g.pgroups : 65535));
    return g;
}
// the kernels' <VEC, LPR> for a geometry: f(std::bool_constant<VEC>{}, int_c<LPR>{})
template <typename F>
static void with_dw_lanes(const DwGeometry& g, F&& f) {
    if (!g.vec) f(std::false_type{}, int_c<64>{});
    else if (g.lpr == 64) f(std::true_type{}, int_c<64>{});
    else if (g.lpr == 32) f(std::true_type{}, int_c<32>{});
    else f(std::true_type{}, int_c<16>{});
}

// Launch geometry of the C = 32 matrix-core kernels (lfss_mfma.hip.h): groups of 64 positions, `gpw` of them per wave, enough
// waves to fill `target_waves` slots, four waves per workgroup.
struct Lfss32Grid { int ngl, gpw; long long ngroups; dim3 grid; };
static Lfss32Grid lfss32_grid(int B, long long L, int target_waves) {
    Lfss32Grid g;
    g.ngl = (int)((L + 63) / 64);
    g.ngroups = (long long)B * g.ngl;
    g.gpw = lfss_groups_per_wave(g.ngroups, target_waves);
    const long long waves = (g.ngroups + g.gpw - 1) / g.gpw;
    g.grid = dim3((unsigned)((waves + 3) / 4));
    return g;
}

// The C = 32 middle kernel (lfss_mid_mfma_kernel): RZ = false reads the gate plane z, RZ = true recomputes it from `tok` (ln_1 +
// in_proj rows [D, 2D)) and takes no z.
template <bool RZ>
static int lfss_mid32_launch(const void* ysum, int ny, int64_t ystride, const void* z, const float* tok, int tok_nchw, const float* ln1_w,
                             const float* ln1_b, float ln1_eps, const float* in_proj_weight, const float* out_norm_w,
                             const float* out_norm_b, float out_norm_eps, const float* out_proj_weight, const float* skip_scale,
                             const float* ln2_w, const float* ln2_b, float ln2_eps, const float* conv1_weight,
                             const float* conv1_bias, float* tok1, void* f, int B, int64_t L, int plane_dtype, hipStream_t st) {
    const Lfss32Grid g = lfss32_grid(B, L, 1024 * (RZ ? WM_LFSS_MID_RZ_WAVES : WM_LFSS_MID_WAVES));
    ProfScope ps(9, st);
#define WM_MID(NY) WM_PLANE_DISPATCH(plane_dtype, hipLaunchKernelGGL((lfss_mid_mfma_kernel<NY, TP, RZ>), g.grid, dim3(256), 0, st, \
                           (const TP*)ysum, (long long)ystride, (const TP*)z, tok, tok_nchw, out_norm_w, out_norm_b, out_norm_eps,    \
                           out_proj_weight, skip_scale, ln2_w, ln2_b, ln2_eps, conv1_weight, conv1_bias, tok1, (TP*)f, B,             \
                           (long long)L, g.ngl, g.ngroups, g.gpw, ln1_w, ln1_b, ln1_eps, in_proj_weight))
    if (ny == 4) WM_MID(4); else WM_MID(1);
#undef WM_MID
    return launch_status();
}

// The argument checks wm_lfss_mid_fwd and wm_lfss_mid_rz_fwd share (have_all: none of the pointers the form reads or writes is null).
// rz, the recomputing form: C == 32 only, and an empty problem is WM_OK before its pointers are looked at.
static int lfss_mid_check(bool rz, bool have_all, const float* tok, int tok_nchw, const float* tok1, int ny, int B, int64_t L, int C,
                          int plane_dtype) {
    if (B < 0 || L < 0 || (ny != 1 && ny != 4)) return WM_EINVAL;
    if (rz ? (C != 32 || (plane_dtype != WM_F32 && plane_dtype != WM_BF16))
           : (plane_dtype != WM_F32 && !(plane_dtype == WM_BF16 && C == 32))) return WM_EUNSUPPORTED;
    const bool empty = B == 0 || L == 0;
    if (rz && empty) return WM_OK;
    if (!empty && !have_all) return WM_ENULL;
    if ((!tok_nchw && !aligned16(tok)) || !aligned16(tok1)) return WM_EALIGN;
    return WM_OK;
}

extern "C" {

int wm_dwconv3x3_fwd(const void* x, const float* weight, const float* bias, void* y, int B, int C,
                     int H, int W, int act, int plane_dtype, void* stream) {
    if (B < 0 || C < 0 || H < 0 || W < 0) return WM_EINVAL;
    const int flip = (act >> 2) & 1;                  // act + 4: the taps rotated by 180 degrees (the input gradient's convolution)
    act &= 3;
    if (act < 0 || act > 2 || (plane_dtype != WM_F32 && plane_dtype != WM_BF16)) return WM_EUNSUPPORTED;
    const long long planes = (long long)B * C;
    if (planes == 0 || H == 0 || W == 0) return WM_OK;
    if (!x || !weight || !y) return WM_ENULL;
    // (vec - bf16: 8-byte accesses, covered by the same alignment test)
    const DwGeometry g = dw_geometry(H, W, planes, (W % 4 == 0) && aligned16(x) && aligned16(y), true);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(act == 1 ? 7 : 17, st);       // + SiLU: SS2D's conv2d (:486-487, hot path); the others belong to the HFE branch / the ffn
    auto launch = [&](auto act_c) {
        with_dw_lanes(g, [&](auto vec, auto lpr) {
            WM_PLANE_DISPATCH(plane_dtype, hipLaunchKernelGGL((dwconv3x3_kernel<act_c(), vec(), TP, lpr()>), g.grid, g.block, 0, st, (const TP*)x,
                                                              weight, bias, (TP*)y, C, H, W, planes, g.rows, flip));
        });
    };
    if (act == 1) launch(int_c<1>{}); else if (act == 2) launch(int_c<2>{}); else launch(int_c<0>{});
    return launch_status();
}

int wm_lfss_in_fwd(const float* tok, int tok_nchw, const float* ln_w, const float* ln_b, float ln_eps,
                   const float* in_proj_weight, void* x_, void* z_, int B, int64_t L, int C, int plane_dtype, void* stream) {
    if (B < 0 || L < 0) return WM_EINVAL;
    if (plane_dtype != WM_F32 && !(plane_dtype == WM_BF16 && C == 32)) return WM_EUNSUPPORTED;    // bf16 planes: C = 32 kernels
    float* x = (float*)x_; float* z = (float*)z_;
    // z == NULL (C == 32 only): the gate half is not written - the block's wm_lfss_mid_rz_fwd recomputes it
    if (B && L && (!tok || !ln_w || !ln_b || !in_proj_weight || !x || (!z && C != 32))) return WM_ENULL;
    if (!tok_nchw && !aligned16(tok)) return WM_EALIGN;
    if (C == 32 && B && L) {
        const Lfss32Grid g = lfss32_grid(B, L, 1024 * WM_LFSS_IN_WAVES);
        hipStream_t st = (hipStream_t)stream;
        ProfScope ps(5, st);
        WM_PLANE_DISPATCH(plane_dtype, hipLaunchKernelGGL(lfss_in_mfma_kernel<TP>, g.grid, dim3(256), 0, st, tok, tok_nchw, ln_w, ln_b,
                                                          ln_eps, in_proj_weight, (TP*)x_, (TP*)z_, B, (long long)L, g.ngl, g.ngroups, g.gpw));
        return launch_status();
    }
    return launch_per_position<16 | 8>(5, B, L, C, stream, [&](auto c, dim3 grid, dim3 block, hipStream_t st) {
        hipLaunchKernelGGL((lfss_in_kernel<c()>), grid, block, 0, st, tok, tok_nchw, ln_w, ln_b, ln_eps, in_proj_weight, x, z, B, (long long)L);
    });
}

// wm_lfss_in_fwd(z = NULL) + wm_dwconv3x3_fwd(act = SiLU) in one kernel (lfss_in_conv_mfma_kernel): C == 32, fp32 planes, W % 32 == 0
// (the widths the block's other folded convolution, wm_lfss_out_conv_fwd, serves) and at most 2^23 positions per image (32-bit byte
// offsets inside a half's 32 planes).  WM_EUNSUPPORTED otherwise: callers keep the two calls.
static bool lfss_in_conv_domain(int H, int W, int C, int plane_dtype) {
    return C == 32 && plane_dtype == WM_F32 && W % 32 == 0 && (long long)H * W <= (1ll << 23);
}

// rows per band: a workgroup is two walks x two channel halves; the even height in [8, 64] of least cost (UHD level 1: 34 rows, 32
// bands, 496 workgroups - one round).  Small maps get kInConvMinBand.
static int lfss_in_conv_band_rows(int B, int H, int W) {
    return row_walk_band_rows(B, H, W, kInConvCols, 2, kInConvMinBand, kInConvMaxBand, 2);
}

int wm_lfss_in_conv_band_rows(int B, int H, int W) {
    if (B < 0 || H < 0 || W < 0) return WM_EINVAL;
    if (!lfss_in_conv_domain(H, W, 32, WM_F32)) return WM_EUNSUPPORTED;
    return lfss_in_conv_band_rows(B, H, W);
}

int wm_lfss_in_conv_fwd(const float* tok, int tok_nchw, const float* ln_w, const float* ln_b, float ln_eps,
                        const float* in_proj_weight, const float* conv_weight, const float* conv_bias, float* xc, int B, int H, int W,
                        int C, int plane_dtype, void* stream) {
    if (B < 0 || H < 0 || W < 0) return WM_EINVAL;
    if (!lfss_in_conv_domain(H, W, C, plane_dtype)) return WM_EUNSUPPORTED;
    if (B == 0 || H == 0 || W == 0) return WM_OK;
    if (!tok || !ln_w || !ln_b || !in_proj_weight || !conv_weight || !xc) return WM_ENULL;
    if (!tok_nchw && !aligned16(tok)) return WM_EALIGN;
    const RowWalkGeom g = row_walk_geom(B, H, W, kInConvCols, lfss_in_conv_band_rows(B, H, W), 2, false);
    const dim3 grid((unsigned)g.nblocks);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(5, st);
    if (tok_nchw)
        hipLaunchKernelGGL(lfss_in_conv_mfma_kernel<true>, grid, dim3(256), 0, st, tok, ln_w, ln_b, ln_eps, in_proj_weight, conv_weight,
                           conv_bias, xc, B, H, W, g.nstrips, g.nbands, g.rows, g.nwalks);
    else
        hipLaunchKernelGGL(lfss_in_conv_mfma_kernel<false>, grid, dim3(256), 0, st, tok, ln_w, ln_b, ln_eps, in_proj_weight, conv_weight,
                           conv_bias, xc, B, H, W, g.nstrips, g.nbands, g.rows, g.nwalks);
    return launch_status();
}

int wm_lfss_mid_fwd(const void* ysum_, int ny, int64_t ystride, const void* z_, const float* tok, int tok_nchw, const float* out_norm_w,
                    const float* out_norm_b, float out_norm_eps, const float* out_proj_weight,
                    const float* skip_scale, const float* ln2_w, const float* ln2_b, float ln2_eps,
                    const float* conv1_weight, const float* conv1_bias, float* tok1, void* f_, int B, int64_t L,
                    int C, int plane_dtype, void* stream) {
    const bool have_all = ysum_ && z_ && tok && out_norm_w && out_norm_b && out_proj_weight && skip_scale && ln2_w && ln2_b && conv1_weight &&
                          conv1_bias && tok1 && f_;
    const int status = lfss_mid_check(false, have_all, tok, tok_nchw, tok1, ny, B, L, C, plane_dtype);
    if (status != WM_OK) return status;
    if (C == 32 && B && L)                                   // the shipped width: projections on the matrix cores
        return lfss_mid32_launch<false>(ysum_, ny, ystride, z_, tok, tok_nchw, nullptr, nullptr, 0.0f, nullptr, out_norm_w, out_norm_b,
                                        out_norm_eps, out_proj_weight, skip_scale, ln2_w, ln2_b, ln2_eps, conv1_weight, conv1_bias,
                                        tok1, f_, B, L, plane_dtype, (hipStream_t)stream);
    return launch_per_position<16 | 8>(9, B, L, C, stream, [&](auto c, dim3 grid, dim3 block, hipStream_t st) {
        hipLaunchKernelGGL((lfss_mid_kernel<c()>), grid, block, 0, st, (const float*)ysum_, ny, (long long)ystride, (const float*)z_, tok, tok_nchw,
                           out_norm_w, out_norm_b, out_norm_eps, out_proj_weight, skip_scale, ln2_w, ln2_b, ln2_eps, conv1_weight, conv1_bias, tok1,
                           (float*)f_, B, (long long)L);
    });
}

// wm_lfss_mid_fwd with the gate z RECOMPUTED from `tok` (ln_1 + in_proj rows [D, 2D) on the matrix cores, bit-identical to
// wm_lfss_in_fwd's z in fp32 planes) instead of read: C == 32 only (WM_EUNSUPPORTED otherwise: callers keep z and wm_lfss_mid_fwd).
int wm_lfss_mid_rz_fwd(const void* ysum_, int ny, int64_t ystride, const float* tok, int tok_nchw, const float* ln1_w,
                       const float* ln1_b, float ln1_eps, const float* in_proj_weight, const float* out_norm_w,
                       const float* out_norm_b, float out_norm_eps, const float* out_proj_weight,
                       const float* skip_scale, const float* ln2_w, const float* ln2_b, float ln2_eps,
                       const float* conv1_weight, const float* conv1_bias, float* tok1, void* f_, int B, int64_t L,
                       int C, int plane_dtype, void* stream) {
    const bool have_all = ysum_ && tok && ln1_w && ln1_b && in_proj_weight && out_norm_w && out_norm_b && out_proj_weight && skip_scale &&
                          ln2_w && ln2_b && conv1_weight && conv1_bias && tok1 && f_;
    const int status = lfss_mid_check(true, have_all, tok, tok_nchw, tok1, ny, B, L, C, plane_dtype);
    if (status != WM_OK || B == 0 || L == 0) return status;
    return lfss_mid32_launch<true>(ysum_, ny, ystride, nullptr, tok, tok_nchw, ln1_w, ln1_b, ln1_eps, in_proj_weight, out_norm_w,
                                   out_norm_b, out_norm_eps, out_proj_weight, skip_scale, ln2_w, ln2_b, ln2_eps, conv1_weight,
                                   conv1_bias, tok1, f_, B, L, plane_dtype, (hipStream_t)stream);
}

// wm_lfss_mid_rz_fwd that ends at tok1 (no ln_2, no conv1, no f): the middle kernel in front of wm_lfss_ffn_fwd, which recomputes f
// from tok1.  Only the form that path needs: C == 32, the four directions' outputs (ny == 4), fp32 planes.  tok1 is bit-identical to
// wm_lfss_mid_rz_fwd's.
int wm_lfss_mid_rz_tok_fwd(const void* ysum_, int ny, int64_t ystride, const float* tok, int tok_nchw, const float* ln1_w,
                           const float* ln1_b, float ln1_eps, const float* in_proj_weight, const float* out_norm_w,
                           const float* out_norm_b, float out_norm_eps, const float* out_proj_weight, const float* skip_scale,
                           float* tok1, int B, int64_t L, int C, int plane_dtype, void* stream) {
    if (B < 0 || L < 0) return WM_EINVAL;
    if (C != 32 || ny != 4 || plane_dtype != WM_F32) return WM_EUNSUPPORTED;
    if (B == 0 || L == 0) return WM_OK;
    if (!ysum_ || !tok || !ln1_w || !ln1_b || !in_proj_weight || !out_norm_w || !out_norm_b || !out_proj_weight || !skip_scale || !tok1)
        return WM_ENULL;
    if ((!tok_nchw && !aligned16(tok)) || !aligned16(tok1)) return WM_EALIGN;
    const Lfss32Grid g = lfss32_grid(B, L, 1024 * WM_LFSS_MID_RZ_WAVES);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(9, st);
    hipLaunchKernelGGL((lfss_mid_mfma_kernel<4, float, true, false>), g.grid, dim3(256), 0, st, (const float*)ysum_, (long long)ystride,
                       (const float*)nullptr, tok, tok_nchw, out_norm_w, out_norm_b, out_norm_eps, out_proj_weight, skip_scale,
                       (const float*)nullptr, (const float*)nullptr, 0.0f, (const float*)nullptr, (const float*)nullptr, tok1,
                       (float*)nullptr, B, (long long)L, g.ngl, g.ngroups, g.gpw, ln1_w, ln1_b, ln1_eps, in_proj_weight);
    return launch_status();
}

// The gated ffn behind wm_lfss_mid_rz_tok_fwd in one kernel (lfss_ffn_mfma_kernel): ln_2 -> conv1 -> depth-wise 3x3 -> GELU gate ->
// conv3 -> second skip connection, f and fc never stored.  C == 32, fp32 planes, W % 32 == 0 and at most 2^23 positions per image
// (32-bit byte offsets inside an image's output).  WM_EUNSUPPORTED otherwise: callers keep wm_lfss_mid_rz_fwd + wm_lfss_out_conv_fwd.
static bool lfss_ffn_domain(int H, int W, int C, int plane_dtype) {
    return C == 32 && plane_dtype == WM_F32 && W % 32 == 0 && (long long)H * W <= (1ll << 23);
}

// rows per band: four walks per workgroup; the height in [4, 64] of least cost (UHD level 1: 34 rows, 2048 walks - one round)
static int lfss_ffn_band_rows(int B, int H, int W) {
    return row_walk_band_rows(B, H, W, kFfnCols, 4, kFfnMinBand, kFfnMaxBand, 1);
}

int wm_lfss_ffn_band_rows(int B, int H, int W) {
    if (B < 0 || H < 0 || W < 0) return WM_EINVAL;
    if (!lfss_ffn_domain(H, W, 32, WM_F32)) return WM_EUNSUPPORTED;
    return lfss_ffn_band_rows(B, H, W);
}

int wm_lfss_ffn_fwd(const float* tok1, const float* ln2_w, const float* ln2_b, float ln2_eps, const float* conv1_weight,
                    const float* conv1_bias, const float* conv2_weight, const float* conv2_bias, const float* conv3_weight,
                    const float* conv3_bias, const float* skip_scale2, float* out, int out_nchw, int B, int H, int W, int C,
                    int plane_dtype, int band_rows, void* stream) {
    if (B < 0 || H < 0 || W < 0 || band_rows < 0) return WM_EINVAL;
    if (!lfss_ffn_domain(H, W, C, plane_dtype)) return WM_EUNSUPPORTED;
    if (B == 0 || H == 0 || W == 0) return WM_OK;
    if (!tok1 || !ln2_w || !ln2_b || !conv1_weight || !conv1_bias || !conv2_weight || !conv3_weight || !conv3_bias || !skip_scale2 || !out)
        return WM_ENULL;
    if (!aligned16(tok1) || (!out_nchw && !aligned16(out))) return WM_EALIGN;
    const RowWalkGeom g = row_walk_geom(B, H, W, kFfnCols, band_rows ? band_rows : lfss_ffn_band_rows(B, H, W), 4, true);
    const dim3 grid((unsigned)g.nblocks);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(11, st);
    if (out_nchw)
        hipLaunchKernelGGL(lfss_ffn_mfma_kernel<true>, grid, dim3(256), 0, st, tok1, ln2_w, ln2_b, ln2_eps, conv1_weight, conv1_bias,
                           conv2_weight, conv2_bias, conv3_weight, conv3_bias, skip_scale2, out, B, H, W, g.nstrips, g.nbands, g.rows, g.nwalks);
    else
        hipLaunchKernelGGL(lfss_ffn_mfma_kernel<false>, grid, dim3(256), 0, st, tok1, ln2_w, ln2_b, ln2_eps, conv1_weight, conv1_bias,
                           conv2_weight, conv2_bias, conv3_weight, conv3_bias, skip_scale2, out, B, H, W, g.nstrips, g.nbands, g.rows, g.nwalks);
    return launch_status();
}

int wm_lfss_out_fwd(const void* fc_,const float* tok1, const float* conv3_weight, const float* conv3_bias,
                    const float* skip_scale2, float* out, int out_nchw, int B, int64_t L, int C, int plane_dtype, void* stream) {
    if (B < 0 || L < 0) return WM_EINVAL;
    if (plane_dtype != WM_F32 && !(plane_dtype == WM_BF16 && C == 32)) return WM_EUNSUPPORTED;
    const float* fc = (const float*)fc_;
    if (B && L && (!fc || !tok1 || !conv3_weight || !conv3_bias || !skip_scale2 || !out)) return WM_ENULL;
    if (!aligned16(tok1) || (!out_nchw && !aligned16(out))) return WM_EALIGN;
    if (C == 32 && B && L) {
        const Lfss32Grid g = lfss32_grid(B, L, 2048);
        hipStream_t st = (hipStream_t)stream;
        ProfScope ps(11, st);
        WM_PLANE_DISPATCH(plane_dtype, hipLaunchKernelGGL(lfss_out_mfma_kernel<TP>, g.grid, dim3(256), 0, st, (const TP*)fc_, tok1, conv3_weight,
                                                          conv3_bias, skip_scale2, out, out_nchw, B, (long long)L, g.ngl, g.ngroups, g.gpw));
        return launch_status();
    }
    return launch_per_position<16 | 8>(11, B, L, C, stream, [&](auto c, dim3 grid, dim3 block, hipStream_t st) {
        hipLaunchKernelGGL((lfss_out_kernel<c()>), grid, block, 0, st, fc, tok1, conv3_weight, conv3_bias, skip_scale2, out, out_nchw, B, (long long)L);
    });
}

int wm_lfss_out_conv_fwd(const void* f_, const float* conv2_weight, const float* conv2_bias, const float* tok1,
                         const float* conv3_weight, const float* conv3_bias, const float* skip_scale2, float* out,
                         int out_nchw, int B, int H, int W, int C, int plane_dtype, void* stream) {
    if (B < 0 || H < 0 || W < 0) return WM_EINVAL;
    if (C != 32 || W % 32 != 0) return WM_EUNSUPPORTED;          // callers fall back to wm_dwconv3x3_fwd + wm_lfss_out_fwd
    if (plane_dtype != WM_F32 && plane_dtype != WM_BF16) return WM_EUNSUPPORTED;
    const long long L = (long long)H * W;
    if (B == 0 || L == 0) return WM_OK;
    if (L > 0x1fffffffLL) return WM_EUNSUPPORTED;                // 32-bit byte offsets inside one channel plane
    if (!f_ || !conv2_weight || !tok1 || !conv3_weight || !conv3_bias || !skip_scale2 || !out) return WM_ENULL;
    if (!aligned16(tok1) || (!out_nchw && !aligned16(out))) return WM_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(11, st);
    // accumulating row-window form (round 6, lfss_out_conv_acc_kernel<4>: four output rows of a 64-column strip per wave pass, the
    // closing product accumulated in registers over groups of eight gated channels, one coalesced load per tap row + lane shifts):
    // W % 64 == 0 and >= 2^18 positions.  Measured (profiles/r06/lfss_out_conv_forms.txt, ms per call at UHD levels 1 / 2): banded
    // one-row form 0.464 / 0.087 (round 4), row windows in LDS R = 2 0.405 / 0.088 (round 4-5; deleted), this form R = 2 0.401 /
    // 0.084, R = 4 0.346 / 0.069; its double-buffered variant 0.338-0.351 / 0.074 (not kept).  Bit-identical outputs in all forms.
    if (W % 64 == 0 && (long long)B * L >= (1ll << 18)) {
        constexpr int R = 4;
        const int nstrips = W / 64, nbands = (H + R - 1) / R;
        // bands per walk (a wave walks consecutive bands of its strip): enough walks for two rounds of the 2,048 resident waves
        int bpw = (int)(((long long)B * nbands * nstrips + 4095) / 4096);
        if (bpw < 1) bpw = 1;
        if (bpw > 8) bpw = 8;
        const int nchunks = (nbands + bpw - 1) / bpw;
        const long long nwalks = (long long)B * nchunks * nstrips;
        WM_PLANE_DISPATCH(plane_dtype, hipLaunchKernelGGL((lfss_out_conv_acc_kernel<R, TP>), dim3((unsigned)((nwalks + 3) / 4)), dim3(256), 0,
                                                          st, (const TP*)f_, conv2_weight, conv2_bias, tok1, conv3_weight, conv3_bias,
                                                          skip_scale2, out, out_nchw, B, H, W, nstrips, nbands, bpw, nchunks, nwalks));
        return launch_status();
    }
    // groups per image row for the kernel's banded (column-major) group order (0: linear order, maps whose width is not a multiple of 64)
    const int gpr = (W % 64 == 0) ? W / 64 : 0;
    const Lfss32Grid g = lfss32_grid(B, L, 2048);
    WM_PLANE_DISPATCH(plane_dtype, hipLaunchKernelGGL(lfss_out_conv_mfma_kernel<TP>, g.grid, dim3(256), 0, st, (const TP*)f_, conv2_weight,
                                                      conv2_bias, tok1, conv3_weight, conv3_bias, skip_scale2, out, out_nchw, B, H, W,
                                                      g.ngl, g.ngroups, g.gpw, gpr));
    return launch_status();
}

int wm_layernorm2d_fwd(const float* x, const float* weight, const float* bias, float eps, float* y, int B,
                       int64_t L, int C, void* stream) {
    if (B < 0 || L < 0) return WM_EINVAL;
    if (B && L && (!x || !weight || !bias || !y)) return WM_ENULL;
    // (C == 64: SS2D.out_norm on (B, D, L) planes, NCHW training path)
    return launch_per_position<64 | 32 | 16 | 8>(16, B, L, C, stream, [&](auto c, dim3 grid, dim3 block, hipStream_t st) {
        hipLaunchKernelGGL((layernorm2d_kernel<c()>), grid, block, 0, st, x, weight, bias, eps, y, B, (long long)L);
    });
}

int wm_dwconv3x3_wgrad(const float* x, const float* gy, float* dW, float* db, int B, int C, int H, int W,
                       void* stream) {
    if (B < 0 || C < 0 || H < 0 || W < 0) return WM_EINVAL;
    if (C == 0) return WM_OK;
    if (!dW) return WM_ENULL;
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = zero_pair(dW, (size_t)C * 9, db, (size_t)C, st);
    if (e != hipSuccess) return (int)e;
    const long long planes = (long long)B * C;
    if (planes == 0 || H == 0 || W == 0) return WM_OK;
    if (!x || !gy) return WM_ENULL;
    // (kDwRows rows per strip: shorter strips on small maps are more atomics - twice the time at config 3's level 3)
    const DwGeometry g = dw_geometry(H, W, planes, (W % 4 == 0) && aligned16(x) && aligned16(gy), false);
    with_dw_lanes(g, [&](auto vec, auto lpr) {
        hipLaunchKernelGGL((dwconv3x3_wgrad_kernel<vec(), lpr()>), g.grid, g.block, 0, st, x, gy, dW, db, C, H, W, planes, g.rows);
    });
    return launch_status();
}

size_t wm_dwconv3x3_wgrad_det_workspace_bytes(int B, int C, int H, int W) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    // (the widest grid of the two access forms: the workspace does not depend on the pointers' alignment)
    const DwGeometry gv = dw_geometry(H, W, (long long)B * C, W % 4 == 0, false), gs = dw_geometry(H, W, (long long)B * C, false, false);
    const size_t nv = (size_t)gv.grid.x * gv.grid.y, ns = (size_t)gs.grid.x * gs.grid.y;
    return (size_t)B * (nv > ns ? nv : ns) * 10 * C * sizeof(float);
}

int wm_dwconv3x3_wgrad_det(const float* x, const float* gy, float* dW, float* db, void* workspace, size_t workspace_bytes, int B, int C,
                           int H, int W, void* stream) {
    if (B < 0 || C < 0 || H < 0 || W < 0) return WM_EINVAL;
    if (C == 0) return WM_OK;
    if (!dW) return WM_ENULL;
    hipStream_t st = (hipStream_t)stream;
    const long long planes = (long long)B * C;
    if (planes == 0 || H == 0 || W == 0) {
        const hipError_t e = zero_pair(dW, (size_t)C * 9, db, (size_t)C, st);
        return e == hipSuccess ? WM_OK : (int)e;
    }
    if (!x || !gy || !workspace) return WM_ENULL;
    if (workspace_bytes < wm_dwconv3x3_wgrad_det_workspace_bytes(B, C, H, W)) return WM_EWORKSPACE;
    const DwGeometry g = dw_geometry(H, W, planes, (W % 4 == 0) && aligned16(x) && aligned16(gy), false);
    float* part = (float*)workspace;
    with_dw_lanes(g, [&](auto vec, auto lpr) {
        hipLaunchKernelGGL((dwconv3x3_wgrad_kernel<vec(), lpr(), true>), g.grid, g.block, 0, st, x, gy, part, (float*)nullptr, C, H, W,
                           planes, g.rows);
    });
    return det_finish(part, (long long)B * g.grid.x * g.grid.y, 10LL * C, DetOut{dW, db, nullptr, kDetDw, 0, 0, 0}, st);
}

// workgroups of the two LayerNorm backward launches (the atomic and the deterministic form share them)
static long long ln2d_bwd_blocks(long long total, int C) {
    const int tpp = C >= 32 ? 2 : 1;                     // threads per pixel (layernorm2d_bwd_pair_kernel)
    long long blocks = (total * tpp + 255) / 256;
    return blocks > 512 ? 512 : blocks;                  // grid-stride: few blocks -> few atomics per channel
}
static long long ln_tok_bwd_blocks(long long T, int C) {
    const int tpb = 256 / (C / 4);
    long long blocks = (T + tpb - 1) / tpb;
    return blocks > 1024 ? 1024 : blocks;                // grid-stride: few blocks -> few atomics per channel
}

size_t wm_layernorm2d_bwd_det_workspace_bytes(int B, int64_t L, int C) {
    if (B <= 0 || L <= 0 || (C != 8 && C != 16 && C != 32 && C != 64)) return 0;
    return (size_t)ln2d_bwd_blocks((long long)B * L, C) * 2 * C * sizeof(float);
}

int wm_layernorm2d_bwd_det(const float* x, const float* weight, const float* gy, float eps, float* gx, float* dweight, float* dbias,
                           void* workspace, size_t workspace_bytes, int B, int64_t L, int C, void* stream) {
    if (B < 0 || L < 0) return WM_EINVAL;
    if (C != 8 && C != 16 && C != 32 && C != 64) return WM_EUNSUPPORTED;
    if (!dweight || !dbias) return WM_ENULL;
    hipStream_t st = (hipStream_t)stream;
    const long long total = (long long)B * L;
    if (total == 0) {
        const hipError_t e = zero_pair(dweight, (size_t)C, dbias, (size_t)C, st);
        return e == hipSuccess ? WM_OK : (int)e;
    }
    if (!x || !weight || !gy || !gx || !workspace) return WM_ENULL;
    if (workspace_bytes < wm_layernorm2d_bwd_det_workspace_bytes(B, L, C)) return WM_EWORKSPACE;
    const long long blocks = ln2d_bwd_blocks(total, C);
    const dim3 grid((unsigned)blocks), block(256);
    float* part = (float*)workspace;
    with_channels<64 | 32 | 16 | 8>(C, [&](auto c) {
        constexpr int CC = c();
        if constexpr (CC >= 32) hipLaunchKernelGGL((layernorm2d_bwd_pair_kernel<CC, true>), grid, block, 0, st, x, weight, gy, eps, gx, part, (float*)nullptr, B, (long long)L);
        else hipLaunchKernelGGL((layernorm2d_bwd_kernel<CC, true>), grid, block, 0, st, x, weight, gy, eps, gx, part, (float*)nullptr, B, (long long)L);
    });
    return det_finish(part, blocks, 2LL * C, DetOut{dweight, dbias, nullptr, kDetSplit, C, 0, 0}, st);
}

int wm_layernorm2d_bwd(const float* x, const float* weight, const float* gy, float eps, float* gx, float* dweight,
                       float* dbias, int B, int64_t L, int C, void* stream) {
    if (B < 0 || L < 0) return WM_EINVAL;
    if (C != 8 && C != 16 && C != 32 && C != 64) return WM_EUNSUPPORTED;
    if (!dweight || !dbias) return WM_ENULL;
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = zero_pair(dweight, (size_t)C, dbias, (size_t)C, st);
    if (e != hipSuccess) return (int)e;
    const long long total = (long long)B * L;
    if (total == 0) return WM_OK;
    if (!x || !weight || !gy || !gx) return WM_ENULL;
    const dim3 grid((unsigned)ln2d_bwd_blocks(total, C)), block(256);
    with_channels<64 | 32 | 16 | 8>(C, [&](auto c) {
        constexpr int CC = c();
        if constexpr (CC >= 32) hipLaunchKernelGGL((layernorm2d_bwd_pair_kernel<CC>), grid, block, 0, st, x, weight, gy, eps, gx, dweight, dbias, B, (long long)L);
        else hipLaunchKernelGGL((layernorm2d_bwd_kernel<CC>), grid, block, 0, st, x, weight, gy, eps, gx, dweight, dbias, B, (long long)L);
    });
    return launch_status();
}

int wm_layernorm_tok_fwd(const float* x, const float* weight, const float* bias, float eps, float* y, int64_t T, int C,
                         void* stream) {
    if (T < 0) return WM_EINVAL;
    if (C != 8 && C != 16 && C != 32 && C != 64) return WM_EUNSUPPORTED;
    if (T == 0) return WM_OK;
    if (!x || !weight || !bias || !y) return WM_ENULL;
    if (!aligned16(x) || !aligned16(y) || !aligned16(weight) || !aligned16(bias)) return WM_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int tpb = 256 / (C / 4);
    long long blocks = (T + tpb - 1) / tpb;
    if (blocks > 256 * 32) blocks = 256 * 32;
    const dim3 grid((unsigned)blocks), block(256);
    with_channels<64 | 32 | 16 | 8>(C, [&](auto c) {
        hipLaunchKernelGGL((layernorm_tok_kernel<c()>), grid, block, 0, st, (const float4*)x, (const float4*)weight, (const float4*)bias, eps,
                           (float4*)y, (long long)T);
    });
    return launch_status();
}

int wm_layernorm_tok_bwd(const float* x, const float* weight, const float* gy, float eps, float* gx, float* dweight,
                         float* dbias, int64_t T, int C, void* stream) {
    if (T < 0) return WM_EINVAL;
    if (C != 8 && C != 16 && C != 32 && C != 64) return WM_EUNSUPPORTED;
    if (!dweight || !dbias) return WM_ENULL;
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = zero_pair(dweight, (size_t)C, dbias, (size_t)C, st);
    if (e != hipSuccess) return (int)e;
    if (T == 0) return WM_OK;
    if (!x || !weight || !gy || !gx) return WM_ENULL;
    if (!aligned16(x) || !aligned16(gy) || !aligned16(gx) || !aligned16(weight)) return WM_EALIGN;
    const dim3 grid((unsigned)ln_tok_bwd_blocks(T, C)), block(256);
    with_channels<64 | 32 | 16 | 8>(C, [&](auto c) {
        hipLaunchKernelGGL((layernorm_tok_bwd_kernel<c()>), grid, block, 0, st, (const float4*)x, (const float4*)weight, (const float4*)gy, eps,
                           (float4*)gx, dweight, dbias, (long long)T);
    });
    return launch_status();
}

size_t wm_layernorm_tok_bwd_det_workspace_bytes(int64_t T, int C) {
    if (T <= 0 || (C != 8 && C != 16 && C != 32 && C != 64)) return 0;
    return (size_t)ln_tok_bwd_blocks(T, C) * 2 * C * sizeof(float);
}

int wm_layernorm_tok_bwd_det(const float* x, const float* weight, const float* gy, float eps, float* gx, float* dweight, float* dbias,
                             void* workspace, size_t workspace_bytes, int64_t T, int C, void* stream) {
    if (T < 0) return WM_EINVAL;
    if (C != 8 && C != 16 && C != 32 && C != 64) return WM_EUNSUPPORTED;
    if (!dweight || !dbias) return WM_ENULL;
    hipStream_t st = (hipStream_t)stream;
    if (T == 0) {
        const hipError_t e = zero_pair(dweight, (size_t)C, dbias, (size_t)C, st);
        return e == hipSuccess ? WM_OK : (int)e;
    }
    if (!x || !weight || !gy || !gx || !workspace) return WM_ENULL;
    if (!aligned16(x) || !aligned16(gy) || !aligned16(gx) || !aligned16(weight)) return WM_EALIGN;
    if (workspace_bytes < wm_layernorm_tok_bwd_det_workspace_bytes(T, C)) return WM_EWORKSPACE;
    const long long blocks = ln_tok_bwd_blocks(T, C);
    const dim3 grid((unsigned)blocks), block(256);
    float* part = (float*)workspace;
    with_channels<64 | 32 | 16 | 8>(C, [&](auto c) {
        hipLaunchKernelGGL((layernorm_tok_bwd_kernel<c(), true>), grid, block, 0, st, (const float4*)x, (const float4*)weight, (const float4*)gy,
                           eps, (float4*)gx, part, (float*)nullptr, (long long)T);
    });
    return det_finish(part, blocks, 2LL * C, DetOut{dweight, dbias, nullptr, kDetSplit, C, 0, 0}, st);
}

// act: 1 = SiLU, 2 = GELU (erf).  a / b / out (and g / ga / gb) are (B, per_b) with batch strides in elements.
int wm_gate_fwd(const float* a, const float* b, float* out, int act, int B, int64_t per_b, int64_t stride_a, int64_t stride_b,
                int64_t stride_out, void* stream) {
    if (B < 0 || per_b < 0) return WM_EINVAL;
    if (act < 1 || act > 3) return WM_EUNSUPPORTED;
    if (B == 0 || per_b == 0) return WM_OK;
    if (!a || !b || !out) return WM_ENULL;
    if (B > 65535) return WM_EUNSUPPORTED;
    GateArgs p{a, b, nullptr, out, nullptr, nullptr, per_b, stride_a, stride_b, 0, stride_out, 0, 0};
    const bool vec = per_b % 4 == 0 && stride_a % 4 == 0 && stride_b % 4 == 0 && stride_out % 4 == 0 && aligned16(a) &&
                     aligned16(b) && aligned16(out);
    const dim3 grid((unsigned)((per_b + 1023) / 1024), (unsigned)B), block(256);
    hipStream_t st = (hipStream_t)stream;
#define WM_GATE(ACT) do { if (vec) hipLaunchKernelGGL((gate_kernel<ACT, false, true>), grid, block, 0, st, p);          \
                          else hipLaunchKernelGGL((gate_kernel<ACT, false, false>), grid, block, 0, st, p); } while (0)
    if (act == 1) WM_GATE(1); else if (act == 2) WM_GATE(2); else WM_GATE(3);
#undef WM_GATE
    return launch_status();
}

int wm_gate_bwd(const float* a, const float* b, const float* g, float* ga, float* gb, int act, int B, int64_t per_b,
                int64_t stride_a, int64_t stride_b, int64_t stride_g, int64_t stride_ga, int64_t stride_gb, void* stream) {
    if (B < 0 || per_b < 0) return WM_EINVAL;
    if (act < 1 || act > 3) return WM_EUNSUPPORTED;
    if (B == 0 || per_b == 0) return WM_OK;
    if (!a || !b || !g || !ga || !gb) return WM_ENULL;
    if (B > 65535) return WM_EUNSUPPORTED;
    GateArgs p{a, b, g, nullptr, ga, gb, per_b, stride_a, stride_b, stride_g, 0, stride_ga, stride_gb};
    const bool vec = per_b % 4 == 0 && stride_a % 4 == 0 && stride_b % 4 == 0 && stride_g % 4 == 0 && stride_ga % 4 == 0 &&
                     stride_gb % 4 == 0 && aligned16(a) && aligned16(b) && aligned16(g) && aligned16(ga) && aligned16(gb);
    const dim3 grid((unsigned)((per_b + 1023) / 1024), (unsigned)B), block(256);
    hipStream_t st = (hipStream_t)stream;
#define WM_GATE(ACT) do { if (vec) hipLaunchKernelGGL((gate_kernel<ACT, true, true>), grid, block, 0, st, p);           \
                          else hipLaunchKernelGGL((gate_kernel<ACT, true, false>), grid, block, 0, st, p); } while (0)
    if (act == 1) WM_GATE(1); else if (act == 2) WM_GATE(2); else WM_GATE(3);
#undef WM_GATE
    return launch_status();
}

int wm_scale_add_fwd(const float* x, const float* scale, const float* o, float* out, int B, int C, int64_t L, void* stream) {
    if (B < 0 || C < 0 || L < 0) return WM_EINVAL;
    if (B == 0 || C == 0 || L == 0) return WM_OK;
    if (!x || !scale || !o || !out) return WM_ENULL;
    if ((long long)B * C > 65535) return WM_EUNSUPPORTED;
    const bool vec = L % 4 == 0 && aligned16(x) && aligned16(o) && aligned16(out);
    const dim3 grid((unsigned)((L + 1023) / 1024), (unsigned)(B * C)), block(256);
    if (vec) hipLaunchKernelGGL(scale_add_fwd_kernel<true>, grid, block, 0, (hipStream_t)stream, x, scale, o, out, C, (long long)L);
    else hipLaunchKernelGGL(scale_add_fwd_kernel<false>, grid, block, 0, (hipStream_t)stream, x, scale, o, out, C, (long long)L);
    return launch_status();
}

// blocks per plane of the scale_add backward: <= 8 (scale_add_bwd_kernel), >= ~2048 in all if the map allows
static long long scale_add_bwd_bpp(int B, int C, int64_t L) {
    long long bpp = (L + 1023) / 1024;
    const long long want = (2048 + (long long)B * C - 1) / ((long long)B * C);
    const long long cap = want > 8 ? want : 8;
    return bpp > cap ? cap : bpp;
}

size_t wm_scale_add_bwd_det_workspace_bytes(int B, int C, int64_t L) {
    if (B <= 0 || C <= 0 || L <= 0) return 0;
    return (size_t)B * scale_add_bwd_bpp(B, C, L) * C * sizeof(float);
}

int wm_scale_add_bwd_det(const float* g, const float* x, const float* scale, float* gx, float* gscale, void* workspace,
                         size_t workspace_bytes, int B, int C, int64_t L, void* stream) {
    if (B < 0 || C < 0 || L < 0) return WM_EINVAL;
    if (C == 0) return WM_OK;
    if (!gscale) return WM_ENULL;
    hipStream_t st = (hipStream_t)stream;
    if (B == 0 || L == 0) {
        const hipError_t e = zero_out(gscale, (size_t)C * sizeof(float), st);
        return e == hipSuccess ? WM_OK : (int)e;
    }
    if (!g || !x || !scale || !gx || !workspace) return WM_ENULL;
    if ((long long)B * C > 65535) return WM_EUNSUPPORTED;
    if (workspace_bytes < wm_scale_add_bwd_det_workspace_bytes(B, C, L)) return WM_EWORKSPACE;
    const bool vec = L % 4 == 0 && aligned16(g) && aligned16(x) && aligned16(gx);
    const long long bpp = scale_add_bwd_bpp(B, C, L);
    const dim3 grid((unsigned)bpp, (unsigned)(B * C)), block(256);
    float* part = (float*)workspace;
    if (vec) hipLaunchKernelGGL((scale_add_bwd_kernel<true, true>), grid, block, 0, st, g, x, scale, gx, part, C, (long long)L);
    else hipLaunchKernelGGL((scale_add_bwd_kernel<false, true>), grid, block, 0, st, g, x, scale, gx, part, C, (long long)L);
    return det_finish(part, (long long)B * bpp, C, DetOut{gscale, nullptr, nullptr, kDetSplit, C, 0, 0}, st);
}

int wm_scale_add_bwd(const float* g, const float* x, const float* scale, float* gx, float* gscale, int B, int C, int64_t L,
                     void* stream) {
    if (B < 0 || C < 0 || L < 0) return WM_EINVAL;
    if (C == 0) return WM_OK;
    if (!gscale) return WM_ENULL;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = zero_out(gscale, (size_t)C * sizeof(float), st);
    if (e != hipSuccess) return (int)e;
    if (B == 0 || L == 0) return WM_OK;
    if (!g || !x || !scale || !gx) return WM_ENULL;
    if ((long long)B * C > 65535) return WM_EUNSUPPORTED;
    const bool vec = L % 4 == 0 && aligned16(g) && aligned16(x) && aligned16(gx);
    const dim3 grid((unsigned)scale_add_bwd_bpp(B, C, L), (unsigned)(B * C)), block(256);
    if (vec) hipLaunchKernelGGL(scale_add_bwd_kernel<true>, grid, block, 0, st, g, x, scale, gx, gscale, C, (long long)L);
    else hipLaunchKernelGGL(scale_add_bwd_kernel<false>, grid, block, 0, st, g, x, scale, gx, gscale, C, (long long)L);
    return launch_status();
}

}  // extern "C"
