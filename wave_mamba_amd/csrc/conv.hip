// conv.hip - C ABI over the dense convolutions (first-generation and wave-specialised kernels), the patchify convolution and the
// depth-wise 3x3 folded into a 1x1 (dw_pw.hip.h) and its mirror image behind a LayerNorm (pw_dw.hip.h).
#include "host_common.h"
#include "conv2d.hip.h"
#include "conv2d_ws.hip.h"
#include "patchify.hip.h"
#include "dw_pw.hip.h"
#include "pw_dw.hip.h"

using namespace wm;

// The operands every entry over Conv2dArgs has; what is particular to an entry (a second source, epilogue operands, LayerNorm
// parameters, ...) it states itself, and everything it does not state keeps the struct's default (null / 0).
static Conv2dArgs conv_args(const void* xa, int Ca, const void* wfrag, const float* bias, void* y, int Cout, int H, int W) {
    Conv2dArgs a;
    a.xa = (const float*)xa; a.wfrag = (const uint4*)wfrag; a.bias = bias; a.y = (float*)y;
    a.Ca = Ca; a.Cout = Cout; a.H = H; a.W = W;
    a.nch = (Ca + 15) / 16; a.mtot = (Cout + 31) / 32;
    return a;
}

// The last two checks of every entry over Conv2dArgs: the batch is a grid dimension and pixel offsets are 32-bit; the kernels load
// the fragments 16 bytes at a time.
static int conv_tail_check(int B, int H, int W, const void* wfrag) {
    if (B > 65535 || (long long)H * W >= (1ll << 31)) return WM_EUNSUPPORTED;
    if (!aligned16(wfrag)) return WM_EALIGN;
    return WM_OK;
}

template <int KS, int RW, int MT, bool G1X1 = false, bool F16 = false, bool LNIN = false>
static int conv2d_launch(const wm::Conv2dArgs& a, int B, hipStream_t st) {
    constexpr int PAD = KS / 2;
    constexpr int smem = ((4 * RW + 2 * PAD) * (wm::kCvTW + 2 * PAD) * 4 + (KS * KS + (G1X1 ? 1 : 0)) * MT * 2 * 64) * 16;   // input planes + weights
    static bool configured[64] = {};
    if (smem > 65536) {
        const int rc = wm::lds_optin((const void*)wm::conv2d_mfma_kernel<KS, RW, MT, G1X1, F16, LNIN>, smem, configured);
        if (rc) return rc;
    }
    const int ntiles = ((a.W + wm::kCvTW - 1) / wm::kCvTW) * ((a.H + 4 * RW - 1) / (4 * RW));
    const dim3 grid((unsigned)(((ntiles + 7) / 8) * 8), (unsigned)B);
    hipLaunchKernelGGL((wm::conv2d_mfma_kernel<KS, RW, MT, G1X1, F16, LNIN>), grid, dim3(256), smem, st, a);
    return launch_status();
}

// Which 3x3 kernel: the persistent wave-specialised one (conv2d_ws.hip.h, one workgroup per compute unit) where it
// pays - enough 64 x 8 tiles that every compute unit pipelines a few (UHD levels 1 and 2 and full resolution; at level 3
// a workgroup gets one or two tiles and the first-generation kernel is 20-30 % faster), at most one epilogue operand and
// then a single 32-channel row tile (two launches re-reading the input lose to the first-generation kernel's one) - and
// where its 32-bit offsets hold.  wm_conv2d_select() pins the choice (parity tests run both on the same inputs: the
// accumulation order per output element is the same, so the results are bit-identical).
// rows per consumer wave (tile = 64 x 2 RW pixels) of the wave-specialised launches: two row tiles, one row tile, gated
#ifndef WM_CONV_WS_RW2
#define WM_CONV_WS_RW2 4
#endif
#ifndef WM_CONV_WS_RW1
#define WM_CONV_WS_RW1 4
#endif
#ifndef WM_CONV_WS_RWG
#define WM_CONV_WS_RWG 2
#endif
#ifndef WM_CONV_WS_NPW1
#define WM_CONV_WS_NPW1 4              // producer waves of the one-row-tile launches
#endif
#ifndef WM_CONV_RW1
#define WM_CONV_RW1 3                  // first-generation 3x3, one row tile: 4 RW rows per tile (conv2d_walk)
#endif
static std::atomic<int> g_conv_select{0};
static int conv_select_mode() { return g_conv_select.load(std::memory_order_relaxed); }
// 64 x th tiles of a wave-specialised launch over the whole batch
static long long conv_ws_ntiles(const wm::Conv2dArgs& a, int B, int th) {
    return (long long)B * ((a.W + wm::kWsTW - 1) / wm::kWsTW) * ((a.H + th - 1) / th);
}
// th: tile rows of the launch that would run (2 x row tiles per workgroup)
static bool conv_ws_enabled(const wm::Conv2dArgs& a, int B, int th) {
    const int mode = conv_select_mode();
    if (mode == 1) return false;
    // 32-bit byte offsets inside one batch element of every tensor; gather indices in two registers
    const long long cmax = std::max(std::max(a.Ca, a.xb ? a.Cbsrc : 0), a.Cout);
    if (cmax * a.H * a.W * 4 >= (1ll << 32) || (a.xb_idx && a.Cb > 128)) return false;
    if (a.gate && a.res) return false;
    if (mode == 2) return true;
    if ((a.gate || a.res) && a.mtot > 1) return false;
    return conv_ws_ntiles(a, B, th) >= 768;
}

template <int RW, int MT, bool G1X1 = false, bool EPI = false, int NPW = 4, bool F16 = false, bool DWTE = false, bool IWTI = false>
static int conv2d_ws_launch(const wm::Conv2dArgs& a, int B, hipStream_t st) {
    using Cfg = wm::ConvWsCfg<RW, MT, G1X1, NPW>;
    static bool configured[64] = {};
    int ncu = 0;
    int rc = wm::lds_optin((const void*)wm::conv3x3_ws_kernel<RW, MT, G1X1, EPI, NPW, F16, DWTE, IWTI>, Cfg::LDS_BYTES, configured);
    if (!rc) rc = wm::device_cus(&ncu);
    if (rc) return rc;
    const long long ntiles = conv_ws_ntiles(a, B, Cfg::TH);
    if (ntiles >= (1ll << 31)) return WM_EUNSUPPORTED;
    const int cus = std::max(8, ncu & ~7);
    const int G = (int)std::min<long long>(cus, ((ntiles + 7) / 8) * 8);
    hipLaunchKernelGGL((wm::conv3x3_ws_kernel<RW, MT, G1X1, EPI, NPW, F16, DWTE, IWTI>), dim3((unsigned)G), dim3(256 + 64 * NPW), Cfg::LDS_BYTES, st, a, B);
    return launch_status();
}

// The walk over the 32-channel row tiles of a dense convolution, ks in {1, 3}: which kernel takes how many tiles per launch.
// F16: the training form (no epilogue operand, so its EPI kernel does not exist); LNIN: LayerNorm2d inside the staging (1x1 only).
template <bool F16, bool LNIN>
static int conv2d_walk(wm::Conv2dArgs& a, int B, int ks, hipStream_t st) {
    for (int mb = 0, n; mb < a.mtot; mb += n) {
        a.mbase = mb;
        const int left = a.mtot - mb;
        int rc = WM_EUNSUPPORTED;                            // (every branch below launches)
        n = 1;                                               // row tiles this launch takes
        if (LNIN || ks == 1) {
            // 1x1 is bandwidth-bound: never read the input twice (3 row tiles in one launch on an 8-row tile)
            if (left >= 3) { rc = conv2d_launch<1, 2, 3, false, F16, LNIN>(a, B, st); n = 3; }
            else if (left == 2) { rc = conv2d_launch<1, 4, 2, false, F16, LNIN>(a, B, st); n = 2; }
            else rc = conv2d_launch<1, 4, 1, false, F16, LNIN>(a, B, st);
        } else if constexpr (!LNIN) {
            // first generation, 32 output channels: 12-row tiles (49 KB of LDS: three workgroups per compute unit, staging slots
            // 93 % used) beat 16-row tiles (two workgroups, 80 %) by 4-13 %; 64 channels keep 16 rows (two accumulator sets)
            if (conv_ws_enabled(a, B, 8)) {
                const bool epi = !F16 && (a.gate || a.res);
                if (epi) { if constexpr (!F16) rc = conv2d_ws_launch<WM_CONV_WS_RW1, 1, false, true>(a, B, st); }
                else if (left >= 2) { rc = conv2d_ws_launch<WM_CONV_WS_RW2, 2, false, false, 4, F16>(a, B, st); n = 2; }
                else rc = conv2d_ws_launch<WM_CONV_WS_RW1, 1, false, false, WM_CONV_WS_NPW1, F16>(a, B, st);
            } else if (left >= 2) { rc = conv2d_launch<3, 4, 2, false, F16>(a, B, st); n = 2; }
            else rc = conv2d_launch<3, WM_CONV_RW1, 1, false, F16>(a, B, st);
        }
        if (rc) return rc;
    }
    return WM_OK;
}

extern "C" {

// nn.Sequential(nn.PixelUnshuffle(r), nn.Conv2d(r r Cin, Cout, 1)) of the UNet's image inputs (reference :1014-1025, :1043-1045) in one
// kernel: an r x r / stride r convolution read straight from the image (patchify.hip.h).
int wm_patchify_conv_fwd(const float* img, const float* weight, const float* bias, float* y, int B, int Cin, int Cout, int H, int W,
                         int r, void* stream) {
    if (B < 0 || Cin <= 0 || Cout <= 0 || H < 0 || W < 0) return WM_EINVAL;
    if (r != 2 && r != 4 && r != 8) return WM_EUNSUPPORTED;
    if (H % r || W % r) return WM_EINVAL;
    if (Cout != 16 && Cout != 32 && Cout != 48 && Cout != 64) return WM_EUNSUPPORTED;
    const size_t lds = (size_t)Cin * r * r * Cout * sizeof(float);
    if (lds > 64 * 1024) return WM_EUNSUPPORTED;
    if (B == 0 || H == 0 || W == 0) return WM_OK;
    if (!img || !weight || !y) return WM_ENULL;
    if (!aligned16(img)) return WM_EALIGN;
    if ((long long)B * Cin * H * W >= (1ll << 40)) return WM_EUNSUPPORTED;
    const int Ho = H / r, Wo = W / r;
    const int spr = (Wo + 255) / 256;
    const long long nsegs = (long long)B * Ho * spr;
    const int spb = (int)((nsegs + 4095) / 4096);
    const long long blocks = (nsegs + spb - 1) / spb;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(18, st);
#define WM_PF(R, CO) hipLaunchKernelGGL((patchify_conv_kernel<R, CO>), dim3((unsigned)blocks), dim3(256), lds, st, img, weight, bias, y, \
                                        B, Cin, H, W, spr, nsegs, spb)
#define WM_PFR(R) do { if (Cout == 16) WM_PF(R, 16); else if (Cout == 32) WM_PF(R, 32); else if (Cout == 48) WM_PF(R, 48); else WM_PF(R, 64); } while (0)
    if (r == 2) WM_PFR(2); else if (r == 4) WM_PFR(4); else WM_PFR(8);
#undef WM_PFR
#undef WM_PF
    return launch_status();
}

size_t wm_conv2d_wfrag_bytes(int Cout, int Cin, int ks) {
    if (Cout <= 0 || Cin <= 0 || (ks != 1 && ks != 3)) return 0;
    return (size_t)((Cin + 15) / 16) * ks * ks * ((Cout + 31) / 32) * 2 * 64 * 16;
}

int wm_conv2d_prep(const float* weight, void* wfrag, int Cout, int Cin, int ks, void* stream) {
    if (Cout <= 0 || Cin <= 0) return WM_EINVAL;
    if (ks != 1 && ks != 3) return WM_EUNSUPPORTED;
    if (!weight || !wfrag) return WM_ENULL;
    if (!aligned16(wfrag)) return WM_EALIGN;
    const int nch = (Cin + 15) / 16, mtot = (Cout + 31) / 32;
    const long long total = (long long)nch * ks * ks * mtot * 128;
    hipLaunchKernelGGL(conv2d_prep_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       weight, (uint4*)wfrag, Cout, Cin, ks * ks, nch, mtot);
    return launch_status();
}

int wm_conv2d_fwd(const float* xa, const float* xb, const int* xb_index, const void* wfrag, const float* bias,
                  const float* gate, const float* residual, float* y, int B, int Ca, int Cb, int Cb_src, int Cout,
                  int H, int W, int ks, void* stream) {
    if (B < 0 || Ca <= 0 || Cb < 0 || Cout <= 0 || H < 0 || W < 0 || Cb_src < 0) return WM_EINVAL;
    if (ks != 1 && ks != 3) return WM_EUNSUPPORTED;
    if (B == 0 || H == 0 || W == 0) return WM_OK;
    if (!xa || !wfrag || !y || (Cb > 0 && !xb)) return WM_ENULL;
    if (Cb > 0 && Ca % 8 != 0) return WM_EUNSUPPORTED;   // an 8-channel fragment never straddles the two sources
    if (Cb > 0 && !xb_index && Cb_src != Cb) return WM_EINVAL;
    if (const int rc = conv_tail_check(B, H, W, wfrag)) return rc;
    hipStream_t st = (hipStream_t)stream;
    Conv2dArgs a = conv_args(xa, Ca, wfrag, bias, y, Cout, H, W);
    if (Cb > 0) { a.xb = xb; a.xb_idx = xb_index; }
    a.Cb = Cb; a.Cbsrc = Cb_src; a.nch = (Ca + Cb + 15) / 16;
    a.gate = gate; a.res = residual;
    ProfScope ps(ks == 3 ? 13 : 14, st);
    return conv2d_walk<false, false>(a, B, ks, st);
}

// y = conv1x1(LayerNorm2d(x)) + bias (+ residual): the LayerNorm of a 32-channel map inside the 1x1 kernel's staging (conv2d.hip.h, LNIN).
int wm_conv2d_ln_fwd(const float* x, const float* ln_weight, const float* ln_bias, float ln_eps, const void* wfrag, const float* bias,
                     const float* residual, float* y, int B, int Cin, int Cout, int H, int W, void* stream) {
    if (B < 0 || Cin <= 0 || Cout <= 0 || H < 0 || W < 0) return WM_EINVAL;
    if (Cin != 32) return WM_EUNSUPPORTED;                 // callers run wm_layernorm2d_fwd + wm_conv2d_fwd
    if (B == 0 || H == 0 || W == 0) return WM_OK;
    if (!x || !ln_weight || !ln_bias || !wfrag || !y) return WM_ENULL;
    if (const int rc = conv_tail_check(B, H, W, wfrag)) return rc;
    hipStream_t st = (hipStream_t)stream;
    Conv2dArgs a = conv_args(x, Cin, wfrag, bias, y, Cout, H, W);
    a.res = residual;
    a.ln_w = ln_weight; a.ln_b = ln_bias; a.ln_eps = ln_eps;
    ProfScope ps(14, st);
    return conv2d_walk<false, true>(a, B, 1, st);
}

// y = conv1x1(act(dwconv3x3(x) + dw_bias)) + bias (+ residual) in one kernel (dw_pw.hip.h): bit-identical to wm_dwconv3x3_fwd +
// wm_conv2d_fwd, without the plane between them.
int wm_dwconv_conv1x1_fwd(const float* x, int64_t x_batch_stride, const float* dw_weight, const float* dw_bias, int act,
                          const void* wfrag, const float* bias, const float* residual, float* y, int B, int C, int Cout, int H,
                          int W, void* stream) {
    if (B < 0 || C <= 0 || Cout <= 0 || H < 0 || W < 0 || x_batch_stride < 0) return WM_EINVAL;
    if (act != 0 && act != 2) return WM_EINVAL;
    if (C != 32 || Cout != 32) return WM_EUNSUPPORTED;
    if (B == 0 || H == 0 || W == 0) return WM_OK;
    if (!x || !dw_weight || !wfrag || !y) return WM_ENULL;
    if ((long long)H * W >= (1ll << 26)) return WM_EUNSUPPORTED;    // 32-bit element offsets inside a batch element
    if (B > 1 && x_batch_stride < (long long)C * H * W) return WM_EINVAL;
    if (!aligned16(wfrag)) return WM_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    DwPwArgs a;
    a.x = x; a.xbs = x_batch_stride; a.dw_w = dw_weight; a.dw_b = dw_bias; a.wfrag = (const uint4*)wfrag; a.bias = bias;
    a.res = residual; a.y = y; a.H = H; a.W = W;
    // rows per band (a band re-reads two input rows and re-forms their taps): the tallest of 16, 8, 4 that still gives every SIMD of
    // a 256-unit chip a wave (UHD level 1: 4080 walks of 16 rows, level 2: 2040 of 8, level 3: 1020 of 4)
    int rows = 4;
    for (int r = 16; r > 4; r >>= 1)
        if (row_walk_geom(B, H, W, kCvTW, r, 4, true).nwalks >= 1024) { rows = r; break; }
    const RowWalkGeom g = row_walk_geom(B, H, W, kCvTW, rows, 4, true);
    a.nstrips = g.nstrips; a.nbands = g.nbands; a.rows = g.rows; a.nwalks = g.nwalks;
    if (g.nblocks >= (1ll << 31)) return WM_EUNSUPPORTED;
    const dim3 grid((unsigned)g.nblocks);
    ProfScope ps(14, st);
    if (act == 2) {
        if (residual) hipLaunchKernelGGL((dw_pw_kernel<true, true>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((dw_pw_kernel<true, false>), grid, dim3(256), 0, st, a);
    } else {
        if (residual) hipLaunchKernelGGL((dw_pw_kernel<false, true>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((dw_pw_kernel<false, false>), grid, dim3(256), 0, st, a);
    }
    return launch_status();
}

// y[:, :Cdw] = dwconv3x3(conv1x1(LayerNorm2d(x)) + bias)[:, :Cdw] + dw_bias, y[:, Cdw:] = (conv1x1(LayerNorm2d(x)) + bias)[:, Cdw:] in one
// kernel (pw_dw.hip.h): bit-identical to wm_conv2d_ln_fwd + wm_dwconv3x3_fwd on the first Cdw channels, without the plane between them.
int wm_ln_conv1x1_dwconv_fwd(const float* x, const float* ln_weight, const float* ln_bias, float ln_eps, const void* wfrag,
                             const float* bias, const float* dw_weight, const float* dw_bias, float* y, int B, int Cin, int Cout,
                             int Cdw, int H, int W, int band_rows, void* stream) {
    if (B < 0 || Cin <= 0 || Cout <= 0 || Cdw <= 0 || H < 0 || W < 0 || band_rows < 0) return WM_EINVAL;
    const bool qkv = Cout == 96 && Cdw == 64, pin = Cout == 32 && Cdw == 32;
    if (Cin != 32 || !(qkv || pin)) return WM_EUNSUPPORTED;          // the two HFE heads; callers run the two calls otherwise
    if (B == 0 || H == 0 || W == 0) return WM_OK;
    if (!x || !ln_weight || !ln_bias || !wfrag || !dw_weight || !y) return WM_ENULL;
    if ((long long)H * W >= (1ll << 25)) return WM_EUNSUPPORTED;     // a 32-plane output tile is one raw buffer of < 2^32 bytes
    if (!aligned16(wfrag)) return WM_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    PwDwArgs a;
    a.x = x; a.ln_w = ln_weight; a.ln_b = ln_bias; a.ln_eps = ln_eps; a.wfrag = (const uint4*)wfrag; a.bias = bias;
    a.dw_w = dw_weight; a.dw_b = dw_bias; a.y = y; a.H = H; a.W = W;
    // rows per band (a band recomputes two x rows of its neighbours): 8 where that still deals every SIMD of a 256-unit chip two
    // walks, else 4 - UHD levels 1 and 2: 8704 / 2176 walks of 8 rows, level 3: 1088 of 4.  Taller bands measured slower at every
    // level, by up to a third: at 2176 walks of 32 rows level 1 is 544 workgroups for the 512 the chip holds at two waves per SIMD -
    // a second, nearly empty round (tools/bench_hfe_heads.py --band-rows, profiles/hfe_heads/per_call_band_rows.txt)
    const int rows = band_rows ? band_rows : (row_walk_geom(B, H, W, kPwDwCols, 8, 4, true).nwalks >= 2048 ? 8 : 4);
    const RowWalkGeom g = row_walk_geom(B, H, W, kPwDwCols, rows, 4, true);
    a.nstrips = g.nstrips; a.nbands = g.nbands; a.rows = g.rows; a.nwalks = g.nwalks;
    if (g.nblocks >= (1ll << 31)) return WM_EUNSUPPORTED;
    const dim3 grid((unsigned)g.nblocks);
    ProfScope ps(14, st);
    if (qkv) hipLaunchKernelGGL((pw_dw_kernel<3, 2>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((pw_dw_kernel<1, 1>), grid, dim3(256), 0, st, a);
    return launch_status();
}

// The training form (conv2d.hip.h, fp16 split with per-tensor power-of-two scales): y = conv(x, w) + bias, ks in {1, 3}; wfrag from
// cv_amax_prep_kernel with the SAME amax buffer {max |x|, max |w|} (device floats).
static int conv2d_fwd_f16(const float* x, const void* wfrag, const float* amax, const float* bias, float* y, int B, int Cin, int Cout,
                          int H, int W, int ks, void* stream) {
    if (B < 0 || Cin <= 0 || Cout <= 0 || H < 0 || W < 0) return WM_EINVAL;
    if (ks != 1 && ks != 3) return WM_EUNSUPPORTED;
    if (B == 0 || H == 0 || W == 0) return WM_OK;
    if (!x || !wfrag || !y || !amax) return WM_ENULL;
    if (const int rc = conv_tail_check(B, H, W, wfrag)) return rc;
    hipStream_t st = (hipStream_t)stream;
    Conv2dArgs a = conv_args(x, Cin, wfrag, bias, y, Cout, H, W);
    a.amax = amax;
    ProfScope ps(ks == 3 ? 13 : 14, st);
    return conv2d_walk<true, false>(a, B, ks, st);
}

// The training step's convolution (fp16 split): `amax` (two floats; a slot of the caller's zeroed arena skips the memset node) and the
// fragments in separate buffers, magnitudes + weight preparation in ONE launch (cv_amax_prep_kernel), then the convolution; dgrad: the
// input-gradient convolution of the forward weight `weight` (conv2d.hip.h: cv_prep_item).  Two launches per convolution where round 4 had
// four (memset, magnitudes, preparation, convolution) - and six with autograd's flipped copy of the weight.
int wm_conv2d_f16_steps(const float* x, const float* weight, const float* bias, float* y, float* amax, void* wfrag, int B, int Cin,
                        int Cout, int H, int W, int ks, int dgrad, void* stream) {
    if (B < 0 || Cin <= 0 || Cout <= 0 || H < 0 || W < 0) return WM_EINVAL;
    if (ks != 1 && ks != 3) return WM_EUNSUPPORTED;
    if (wm_conv2d_wfrag_bytes(Cout, Cin, ks) == 0) return WM_EUNSUPPORTED;
    if (B == 0 || H == 0 || W == 0) return WM_OK;
    if (!x || !weight || !y || !amax || !wfrag) return WM_ENULL;
    if (!aligned16(wfrag)) return WM_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    if (zero_out(amax, 2 * sizeof(float), st) != hipSuccess) return WM_EHIP;
    const long long nx = (long long)B * Cin * H * W, nw = (long long)Cout * Cin * ks * ks;
    long long blocks = (nx / 4 + 256 * 8 - 1) / (256 * 8);           // >= 8 float4 per thread
    blocks = blocks < 1 ? 1 : (blocks > 512 ? 512 : blocks);
    const int nch = (Cin + 15) / 16, mtot = (Cout + 31) / 32;
    const long long items = (long long)nch * ks * ks * mtot * 128;
    const int nprep = (int)(items <= 512 ? 1 : (items >= 32 * 512 ? 32 : (items + 511) / 512));   // ~2 fragment items per thread
    hipLaunchKernelGGL(cv_amax_prep_kernel, dim3((unsigned)blocks + nprep), dim3(256), 0, st, x, nx, weight, nw, (unsigned*)amax,
                       (uint4*)wfrag, Cout, Cin, ks * ks, nch, mtot, dgrad ? 1 : 0, nprep);
    int rc = launch_status();
    if (rc) return rc;
    return conv2d_fwd_f16(x, wfrag, amax, bias, y, B, Cin, Cout, H, W, ks, stream);
}

// (ll, hl, lh, hh) = dwt(conv3x3(img) + bias): the wave-specialised kernel with the analysis epilogue (conv2d_ws.hip.h, DWTE) - the
// first-generation kernel has no such form, so a call it would have to serve is refused.
int wm_conv2d_dwt_fwd(const void* img, const void* wfrag, const float* bias, void* ll, void* hl, void* lh, void* hh, int B, int Cin,
                      int Cout, int H, int W, int dtype, void* stream) {
    if (B < 0 || Cin <= 0 || Cout <= 0 || H < 0 || W < 0) return WM_EINVAL;
    if (H % 2 || W % 2) return WM_EINVAL;
    if (dtype != WM_F32 || Cout != 32) return WM_EUNSUPPORTED;
    if (B == 0 || H == 0 || W == 0) return WM_OK;
    if (!img || !wfrag || !ll || !hl || !lh || !hh) return WM_ENULL;
    if (const int rc = conv_tail_check(B, H, W, wfrag)) return rc;
    hipStream_t st = (hipStream_t)stream;
    Conv2dArgs a = conv_args(img, Cin, wfrag, bias, ll, Cout, H, W);        // (Cout = 32: one row tile, mbase stays 0)
    a.yband[0] = (float*)hl; a.yband[1] = (float*)lh; a.yband[2] = (float*)hh;
    // the kernel's 32-bit byte offsets inside one batch element of the input and of the full-resolution output it stands for
    if (conv_select_mode() == 1 || (long long)std::max(Cin, Cout) * H * W * 4 >= (1ll << 32)) return WM_EUNSUPPORTED;
    ProfScope ps(13, st);
    return conv2d_ws_launch<WM_CONV_WS_RW1, 1, false, false, WM_CONV_WS_NPW1, false, true>(a, B, st);
}

// y = conv3x3(iwt(low, high)) + bias (+ residual): the wave-specialised kernel whose producers form the input tile from the bands
// (conv2d_ws.hip.h, IWTI); refused where the first-generation kernel would have to serve the call.
int wm_idwt_conv2d_fwd(const void* low, const void* high, const void* wfrag, const float* bias, const float* residual, float* y, int B,
                       int Cin, int Cout, int H, int W, int dtype, void* stream) {
    if (B < 0 || Cin <= 0 || Cout <= 0 || H < 0 || W < 0) return WM_EINVAL;
    if (H % 2 || W % 2) return WM_EINVAL;
    if (dtype != WM_F32 || Cin != 32) return WM_EUNSUPPORTED;
    if (B == 0 || H == 0 || W == 0) return WM_OK;
    if (!low || !high || !wfrag || !y) return WM_ENULL;
    if (const int rc = conv_tail_check(B, H, W, wfrag)) return rc;
    hipStream_t st = (hipStream_t)stream;
    Conv2dArgs a = conv_args(low, Cin, wfrag, bias, y, Cout, H, W);
    a.xb = (const float*)high; a.Cbsrc = 3 * Cin;            // the bands feed the same Cin / 16 chunks: Cb stays 0 and nch as built
    a.res = residual;
    // 32-bit byte offsets inside one batch element of `high` (3 Cin planes of H W / 4), of y and of the residual
    if (conv_select_mode() == 1 || (long long)std::max(Cin, Cout) * H * W * 4 >= (1ll << 32)) return WM_EUNSUPPORTED;
    ProfScope ps(13, st);
    for (int mb = 0; mb < a.mtot; ++mb) {
        a.mbase = mb;
        const int rc = residual ? conv2d_ws_launch<WM_CONV_WS_RW1, 1, false, true, 4, false, false, true>(a, B, st)
                                : conv2d_ws_launch<WM_CONV_WS_RW1, 1, false, false, WM_CONV_WS_NPW1, false, false, true>(a, B, st);
        if (rc) return rc;
    }
    return WM_OK;
}

int wm_conv2d_gated_fwd(const float* xa, const float* xb, const int* xb_index, const void* wfrag3, const void* wfrag1,
                        const float* bias1, float* y, int B, int Ca, int Cb, int Cb_src, int Cout, int H, int W,
                        void* stream) {
    if (B < 0 || Ca <= 0 || Cb < 0 || Cout <= 0 || H < 0 || W < 0 || Cb_src < 0) return WM_EINVAL;
    if (B == 0 || H == 0 || W == 0) return WM_OK;
    if (!xa || !wfrag3 || !wfrag1 || !y || (Cb > 0 && !xb)) return WM_ENULL;
    if (Cb > 0 && Ca % 8 != 0) return WM_EUNSUPPORTED;
    if (Cb > 0 && !xb_index && Cb_src != Cb) return WM_EINVAL;
    if (const int rc = conv_tail_check(B, H, W, wfrag3)) return rc;
    if (!aligned16(wfrag1)) return WM_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    Conv2dArgs a = conv_args(xa, Ca, wfrag3, nullptr, y, Cout, H, W);
    if (Cb > 0) { a.xb = xb; a.xb_idx = xb_index; }
    a.Cb = Cb; a.Cbsrc = Cb_src; a.nch = (Ca + Cb + 15) / 16;
    a.wfrag1 = (const uint4*)wfrag1; a.bias1 = bias1;
    ProfScope ps(13, st);
    for (int mb = 0; mb < a.mtot;) {
        // two accumulator sets per wave: 64 channels x 8-row tiles read the input once (0.79 ms against 0.90 ms for
        // two 32-channel x 16-row launches at UHD level 1, 64 -> 64); a last odd row tile takes the 16-row form
        a.mbase = mb;
        int rc;
        const bool two = a.mtot - mb >= 2;                   // an odd tail runs one 32-channel tile on 8-row tiles
        if (conv_ws_enabled(a, B, two ? 2 * WM_CONV_WS_RWG : 8)) {
            if (two) { rc = conv2d_ws_launch<WM_CONV_WS_RWG, 2, true>(a, B, st); mb += 2; }
            else { rc = conv2d_ws_launch<4, 1, true>(a, B, st); mb += 1; }
        } else if (a.mtot - mb >= 2) { rc = conv2d_launch<3, 2, 2, true>(a, B, st); mb += 2; }
        else { rc = conv2d_launch<3, 4, 1, true>(a, B, st); mb += 1; }
        if (rc) return rc;
    }
    return WM_OK;
}

int wm_conv2d_select(int mode) {
    if (mode < 0 || mode > 2) return WM_EINVAL;
    g_conv_select.store(mode, std::memory_order_relaxed);
    return WM_OK;
}

#if WM_CV_STAMP
int wm_debug_conv_stamps(unsigned long long* out) {      // host buffer of 2 * 128 * 8 values
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(wm::g_cv_stamps), sizeof(unsigned long long) * 2 * 128 * 8);
}
#endif

}  // extern "C"
