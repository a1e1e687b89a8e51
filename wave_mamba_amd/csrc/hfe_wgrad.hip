// hfe_wgrad.hip - C ABI over the HFE branch (Gram products, matching, attention fold, SKFF), plane sums and the dense weight gradient.
#include "host_common.h"
#include "gram.hip.h"
#include "hfe.hip.h"
#include "conv_wgrad.hip.h"

namespace wm {
// waves / blocks / slice of a Gram launch
static void gram_plan(int64_t L, long long& nblk, long long& slice) {
    // >= 512 positions per wave on large maps; small maps are latency-bound (one round trip per 32 positions of a
    // wave), so they get down to 128 positions per wave, up to 2048 waves
    long long waves = (L + 511) / 512, wsmall = (L + 127) / 128;
    if (wsmall > 2048) wsmall = 2048;
    if (waves < wsmall) waves = wsmall;
    if (waves > 4096) waves = 4096;
    if (waves < 1) waves = 1;
    waves = ((waves + kGramWaves - 1) / kGramWaves) * kGramWaves;
    slice = (L + waves - 1) / waves;
    slice = ((slice + 31) / 32) * 32;
    if (slice < 32) slice = 32;
    nblk = waves / kGramWaves;
}
}  // namespace wm

using namespace wm;

// blocks per plane of the SKFF reduction / apply kernels: ~16 blocks per compute unit in flight over all planes
static long long skff_bpp_cap(long long planes) { return (256 * 16 + planes - 1) / planes; }

extern "C" {

size_t wm_gram_workspace_bytes(int B, int C, int64_t L) {
    if (B <= 0 || C <= 0 || C > 32 || L < 0) return 0;
    long long nblk, slice;
    gram_plan(L, nblk, slice);
    return (size_t)B * nblk * kGramPart * sizeof(float);
}

int wm_gram_fwd(const float* X, const float* Y, float* G, float* nx, float* ny, void* workspace, size_t workspace_bytes,
                int B, int C, int64_t L, void* stream) {
    if (B < 0 || C < 0 || L < 0) return WM_EINVAL;
    if (C > 32) return WM_EUNSUPPORTED;
    if (B == 0 || C == 0) return WM_OK;
    if (!X || !Y || !G || !nx || !ny || !workspace) return WM_ENULL;
    if (!aligned16(X) || !aligned16(Y) || !aligned16(workspace)) return WM_EALIGN;
    long long nblk, slice;
    gram_plan(L, nblk, slice);
    if (workspace_bytes < (size_t)B * nblk * kGramPart * sizeof(float)) return WM_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)workspace;
    if (L % 4 == 0)
        hipLaunchKernelGGL(gram32_kernel<true>, dim3((unsigned)nblk, (unsigned)B), dim3(64 * kGramWaves), 0, st, X, Y, part, C,
                           (long long)L, slice);
    else
        hipLaunchKernelGGL(gram32_kernel<false>, dim3((unsigned)nblk, (unsigned)B), dim3(64 * kGramWaves), 0, st, X, Y, part, C,
                           (long long)L, slice);
    hipLaunchKernelGGL(gram_reduce_kernel, dim3(kGramPart / 64, (unsigned)B), dim3(256), 0, st, (const float*)part, G, nx, ny,
                       C, (int)nblk);
    return launch_status();
}

// ---- dense convolution weight gradient (conv_wgrad.hip.h) -----------------------------------------------------------
// position sub-ranges (= partials per input tile) of the weight-gradient launch; *blocks = workgroups along x
static int conv_wgrad_parts(long long nunits, int ntiles_in, int* upw, int* blocks) {
    // About one 4-wave workgroup per compute unit: a wave's fixed cost - its OT x TAPS KB partial and the finish kernel's
    // pass over it - is what more of them buy (tools/bench_conv_wgrad.py).  A workgroup holds tpw input tiles x gpw
    // position sub-ranges.
#ifndef WM_CW_TARGET
#define WM_CW_TARGET 256
#endif
#ifndef WM_CW_MINUNITS
#define WM_CW_MINUNITS 4
#endif
    const int tpw = cw_tiles_per_wg(ntiles_in), gpw = kCwWaves / tpw;
    const int ygroups = (ntiles_in + tpw - 1) / tpw;
    long long wgs = WM_CW_TARGET / ygroups;
    if (wgs < 1) wgs = 1;
    long long parts = wgs * gpw;
    const long long most = nunits / WM_CW_MINUNITS;
    if (parts > most) parts = most;
    if (parts < 1) parts = 1;
    const long long per = (nunits + parts - 1) / parts;
    *upw = (int)per;
    parts = (nunits + per - 1) / per;
    *blocks = (int)((parts + gpw - 1) / gpw);
    return (int)parts;
}
size_t wm_conv2d_wgrad_workspace_bytes(int B, int Cin, int Cout, int H, int W, int ks) {
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || (ks != 1 && ks != 3) || W % 32 != 0) return 0;
    const int OT = (Cout + 15) / 16;
    if (OT > 6 || (OT != 1 && OT != 2 && OT != 4 && OT != 6)) return 0;
    int upw, blocks;
    const int np = conv_wgrad_parts((long long)B * H * (W / 32), (Cin + 15) / 16, &upw, &blocks);
    return ((size_t)((Cin + 15) / 16) * np * OT * ks * ks * 256 + (size_t)np * kCwBiasRow) * sizeof(float);
}
int wm_conv2d_wgrad(const float* gy, const float* x, float* dW, float* db, void* workspace, size_t workspace_bytes, int B, int Cin,
                    int Cout, int H, int W, int ks, void* stream) {
    if (B < 0 || Cin <= 0 || Cout <= 0 || H < 0 || W < 0) return WM_EINVAL;
    if (ks != 1 && ks != 3) return WM_EUNSUPPORTED;
    if (!dW) return WM_ENULL;
    hipStream_t st = (hipStream_t)stream;
    if (B == 0 || H == 0 || W == 0) {
        hipError_t e = zero_async(dW, (size_t)Cout * Cin * ks * ks * sizeof(float), st);
        if (e == hipSuccess && db) e = zero_async(db, (size_t)Cout * sizeof(float), st);
        return e == hipSuccess ? WM_OK : (int)e;
    }
    const size_t need = wm_conv2d_wgrad_workspace_bytes(B, Cin, Cout, H, W, ks);
    if (need == 0) return WM_EUNSUPPORTED;                        // W % 32 != 0, more than 96 output channels, ...
    if ((long long)B * (Cin > Cout ? Cin : Cout) * H * W > 0x7fffffffffLL || (long long)B * H * (W / 32) > 0x7fffff00LL) return WM_EUNSUPPORTED;
    if (!gy || !x || !workspace) return WM_ENULL;
    if (workspace_bytes < need) return WM_EWORKSPACE;
    if (!aligned16(gy) || !aligned16(x) || !aligned16(workspace)) return WM_EALIGN;
    ConvWgradArgs a;
    a.gy = gy; a.x = x; a.part = (float*)workspace; a.dW = dW; a.B = B; a.Cin = Cin; a.Cout = Cout; a.H = H; a.W = W;
    a.nunits = (long long)B * H * (W / 32);
    int blocks = 1;
    a.nparts = conv_wgrad_parts(a.nunits, (Cin + 15) / 16, &a.upw, &blocks);
    const int OT = (Cout + 15) / 16, ITN = (Cin + 15) / 16;
    a.bpart = (float*)workspace + (size_t)ITN * a.nparts * OT * ks * ks * 256;
    a.db = db;
    const int ygroups = (ITN + cw_tiles_per_wg(ITN) - 1) / cw_tiles_per_wg(ITN);
#define WM_CW(KS, OTV, CO0, NCO)                                                                                         \
    do {                                                                                                                 \
        a.co0 = (CO0); a.nco = (NCO);                                                                                    \
        hipLaunchKernelGGL((conv_wgrad_kernel<KS, OTV>), dim3((unsigned)blocks, (unsigned)ygroups), dim3(64 * kCwWaves), 0, st, a); \
        hipLaunchKernelGGL((conv_wgrad_finish_kernel<KS, OTV>), dim3((unsigned)(OTV * KS * KS * 16), (unsigned)ITN), dim3(256), 0, st, a); \
    } while (0)
    if (ks == 3) {
        if (OT == 1) WM_CW(3, 1, 0, Cout); else if (OT == 2) WM_CW(3, 2, 0, Cout); else if (OT == 4) WM_CW(3, 4, 0, Cout);
        else { WM_CW(3, 4, 0, 64); WM_CW(3, 2, 64, Cout - 64); }     // 65 .. 96 output channels: two passes (same workspace, stream order)
    } else {
        if (OT == 1) WM_CW(1, 1, 0, Cout); else if (OT == 2) WM_CW(1, 2, 0, Cout); else if (OT == 4) WM_CW(1, 4, 0, Cout); else WM_CW(1, 6, 0, Cout);
    }
#undef WM_CW
    return launch_status();
}

// blocks per plane of the plane-sum launch
static long long plane_sums_bpp(long long planes, long long HW) {
    long long bpp = (HW / 4 + 256 * 8 - 1) / (256 * 8);
    const long long cap = (256 * 16 + planes - 1) / planes;
    if (bpp > cap) bpp = cap;
    return bpp < 1 ? 1 : bpp;
}

size_t wm_plane_sums_det_workspace_bytes(int B, int C, int H, int W) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)B * plane_sums_bpp((long long)B * C, (long long)H * W) * C * sizeof(float);
}

int wm_plane_sums_det(const float* x, float* sums, void* workspace, size_t workspace_bytes, int B, int C, int H, int W, void* stream) {
    if (B < 0 || C < 0 || H < 0 || W < 0) return WM_EINVAL;
    if (C == 0) return WM_OK;
    if (!sums) return WM_ENULL;
    hipStream_t st = (hipStream_t)stream;
    const long long HW = (long long)H * W, planes = (long long)B * C;
    if (planes == 0 || HW == 0) {
        const hipError_t e = zero_out(sums, (size_t)C * sizeof(float), st);
        return e == hipSuccess ? WM_OK : (int)e;
    }
    if (!x || !workspace) return WM_ENULL;
    if (planes > 65535) return WM_EUNSUPPORTED;
    if (workspace_bytes < wm_plane_sums_det_workspace_bytes(B, C, H, W)) return WM_EWORKSPACE;
    const bool vec = (HW % 4 == 0) && aligned16(x);
    const long long bpp = plane_sums_bpp(planes, HW);
    float* part = (float*)workspace;
    hipLaunchKernelGGL(plane_sums_kernel<true>, dim3((unsigned)bpp, (unsigned)planes), dim3(256), 0, st, x, part, C, HW, vec);
    return det_finish(part, (long long)B * bpp, C, DetOut{sums, nullptr, nullptr, kDetSplit, C, 0, 0}, st);
}

int wm_plane_sums(const float* x, float* sums, int B, int C, int H, int W, void* stream) {
    if (B < 0 || C < 0 || H < 0 || W < 0) return WM_EINVAL;
    if (C == 0) return WM_OK;
    if (!sums) return WM_ENULL;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = zero_out(sums, (size_t)C * sizeof(float), st);
    if (e != hipSuccess) return (int)e;
    const long long HW = (long long)H * W, planes = (long long)B * C;
    if (planes == 0 || HW == 0) return WM_OK;
    if (!x) return WM_ENULL;
    if (planes > 65535) return WM_EUNSUPPORTED;
    const bool vec = (HW % 4 == 0) && aligned16(x);
    const long long bpp = plane_sums_bpp(planes, HW);
    hipLaunchKernelGGL(plane_sums_kernel<false>, dim3((unsigned)bpp, (unsigned)planes), dim3(256), 0, st, x, sums, C, HW, vec);
    return launch_status();
}

int wm_match_index(const float* G, const float* nx, const float* ny, int* index, int B, int C, void* stream) {
    if (B < 0 || C < 0) return WM_EINVAL;
    if (B == 0 || C == 0) return WM_OK;
    if (!G || !nx || !ny || !index) return WM_ENULL;
    hipLaunchKernelGGL(match_argmin_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, G, nx, ny, index, C);
    return launch_status();
}

int wm_attn_fold(const float* G, const float* nq, const float* nk, const float* temperature, const float* Wpo,
                 float* Wout, int B, int C, int heads, void* stream) {
    if (B < 0 || C <= 0 || heads <= 0 || C % heads != 0) return WM_EINVAL;
    if (C > 64) return WM_EUNSUPPORTED;
    if (B == 0) return WM_OK;
    if (!G || !nq || !nk || !temperature || !Wpo || !Wout) return WM_ENULL;
    hipLaunchKernelGGL(attn_fold_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, G, nq, nk, temperature,
                       Wpo, Wout, C, heads);
    return launch_status();
}

size_t wm_skff_workspace_bytes(int B, int C) {
    if (B <= 0 || C <= 0) return 0;
    const long long planes = (long long)B * C;
    return (size_t)(planes * skff_bpp_cap(planes) + 3 * planes) * sizeof(float);
}

int wm_skff_fwd(const float* x0, const float* x1, const float* x2, const float* Wdu, const float* prelu,
                const float* Wfc, float* out, void* workspace, size_t workspace_bytes, int B, int C, int d, int H, int W,
                void* stream) {
    if (B < 0 || C <= 0 || d <= 0 || H < 0 || W < 0) return WM_EINVAL;
    if (C > 64 || d > 16) return WM_EUNSUPPORTED;
    if (B == 0 || H == 0 || W == 0) return WM_OK;
    if (!x0 || !x1 || !x2 || !Wdu || !prelu || !Wfc || !out || !workspace) return WM_ENULL;
    if (workspace_bytes < wm_skff_workspace_bytes(B, C)) return WM_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const long long HW = (long long)H * W, planes = (long long)B * C;
    if (planes > 65535) return WM_EUNSUPPORTED;
    const bool vec = (HW % 4 == 0) && aligned16(x0) && aligned16(x1) && aligned16(x2) && aligned16(out);
    long long bpp = (HW / 4 + 256 * 8 - 1) / (256 * 8);              // >= 8 float4 per thread
    const long long cap = skff_bpp_cap(planes);
    if (bpp > cap) bpp = cap;
    if (bpp < 1) bpp = 1;
    float* wts = (float*)workspace;                      // (B, 3, C)
    float* part = wts + (size_t)3 * planes;              // (B, C, bpp) block partials of the plane sums
    const dim3 grid((unsigned)bpp, (unsigned)planes), block(256);
    ProfScope ps(15, st);
    hipLaunchKernelGGL(chansum3_kernel, grid, block, 0, st, x0, x1, x2, part, HW, vec);
    hipLaunchKernelGGL(skff_weights_kernel, dim3((unsigned)B), dim3(64), 0, st, (const float*)part, (int)bpp, Wdu, prelu, Wfc,
                       wts, C, d, (float)(1.0 / (double)HW));
    hipLaunchKernelGGL(skff_apply_kernel, grid, block, 0, st, x0, x1, x2, wts, out, C, HW, vec);
    return launch_status();
}

}  // extern "C"
