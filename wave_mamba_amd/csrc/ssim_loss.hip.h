// ssim_loss.hip.h - the SSIM training loss (mean SSIM of float image planes) and its input gradients, for gfx950.
//
// Reference: basicsr/models/cal_ssim.py, SSIM(window_size = 11, size_average = True) - what FeMaSRModel builds as self.ssim
// (basicsr/models/femasr_model.py:29) and train_wavemamba_uhdll.yml:99-100 weights by 0.25 (`pixel_ssim_opt`).  Per plane (:17-35):
//   mu1 = w * a, mu2 = w * b, e11 = w * a^2, e22 = w * b^2, e12 = w * ab     w = g g^T, 11 x 11, ZERO padding of 5
//   A1 = 2 mu1 mu2 + C1, A2 = 2 (e12 - mu1 mu2) + C2, B1 = mu1^2 + mu2^2 + C1, B2 = (e11 - mu1^2) + (e22 - mu2^2) + C2
//   S = A1 A2 / (B1 B2),  C1 = 0.01^2, C2 = 0.03^2;  the result is the mean of S over every plane and pixel.
// This is not the evaluation metric of metrics.hip.h (uint8 Y plane, replicate border, 0..255 constants, no gradient).
//
// Forward: one workgroup per SL_TH x SL_TW output tile - the tile and its 5-pixel halo of a and b into LDS (zero outside the
// image; 16-byte loads where W % 4 == 0 and the planes are 16-byte aligned: sl_stage), the 11-tap row filter of the five
// moments into LDS, the column filter and the map in registers (three rows per thread: the 13 row-filtered values of a column
// serve three outputs), the tile's sum of S to a workspace slot.  When a gradient is wanted the same pass stores dS/dmu1 (P1),
// dS/dmu2 (P2), dS/de11 = dS/de22 (Q) and dS/de12 (R) as fp32 planes.  A second kernel adds the slots in a fixed order: no
// atomics, nothing zeroed, two calls are bit-identical, capturable into a graph.
// Backward (w is symmetric, so the adjoint of each filter is the filter):
//   ga = gout / n * [ w * P1 + 2 a (w * Q) + b (w * R) ],   gb the same with P2 and a, b exchanged
// one kernel per gradient: the three maps with a zero halo into LDS, row pass, column pass, combine.
//
// Arithmetic: fp32 inputs and maps, float64 (SlAcc) filter accumulators and a float64 map (as the metric kernel).  The
// reference's own fp32 loses e11 - mu1^2 on flat bright regions (up to 4e-4 of the gradient at 40 x 130); float64 moments do
// not.  The taps are the reference's: float32 values (SlGauss), whose sum is 1 - 3.1e-8 - B2 is 9e-4 on a flat region and
// feels it.
#pragma once
#include <hip/hip_runtime.h>

namespace wm {

constexpr int SL_TW = 32, SL_TH = 24, SL_HALO = 5, SL_TAPS = 11, SL_RPT = 3;      // SL_RPT rows per thread in the column pass
constexpr int SL_YR = SL_TH + 2 * SL_HALO, SL_YC = SL_TW + 2 * SL_HALO;           // 34 x 42 staged values per plane
static_assert(SL_TW * (SL_TH / SL_RPT) == 256 && SL_TH % SL_RPT == 0, "one thread per column and group of SL_RPT rows");

using SlAcc = double;            // the type of the filter accumulators, the row-filtered maps in LDS and the per-pixel map

struct SlGauss {
    SlAcc g[SL_TAPS];             // host-computed: float32(exp(-(i - 5)^2 / 4.5)) / their float32 sum, widened
};

struct SlGeom {
    int H, W, tilesX, tilesY;     // blockIdx.x = (plane * tilesY + ty) * tilesX + tx
    int vec;                      // W % 4 == 0 and every staged plane 16-byte aligned (the host checks): stage with 16-byte loads
};

constexpr int SL_VPR = (SL_YC + 3 + 3) / 4;                                      // 12 float4 cover a halo row from column x0 - 8
static_assert(SL_TW % 4 == 0 && SL_HALO <= 8 && 4 * SL_VPR - 8 >= SL_TW + SL_HALO, "the aligned span holds the halo row");

// Tile + halo of one plane into LDS, zero outside the image (F.conv2d's padding).  gm.vec: x0 - 8 is a multiple of 4 and so is W,
// so each aligned group of four floats lies wholly inside a row of the image or wholly outside: one 16-byte load per group, the
// 3 + 3 floats beyond the halo dropped.  Otherwise (any W, any 4-byte-aligned plane) one load per element.  Same values either way.
__device__ inline void sl_stage(const float* __restrict__ src, const SlGeom& gm, int y0, int x0, float (&dst)[SL_YR][SL_YC]) {
    if (gm.vec) {
        for (int i = threadIdx.x; i < SL_YR * SL_VPR; i += 256) {
            const int r = i / SL_VPR, k = i - r * SL_VPR;
            const int gy = y0 + r - SL_HALO, gx = x0 - 8 + 4 * k;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (gy >= 0 && gy < gm.H && gx >= 0 && gx < gm.W) v = *reinterpret_cast<const float4*>(src + (long long)gy * gm.W + gx);
            const int c = 4 * k - (8 - SL_HALO);                                   // dst column of v.x: gx - (x0 - SL_HALO)
            if (c >= 0 && c < SL_YC) dst[r][c] = v.x;
            if (c + 1 >= 0 && c + 1 < SL_YC) dst[r][c + 1] = v.y;
            if (c + 2 >= 0 && c + 2 < SL_YC) dst[r][c + 2] = v.z;
            if (c + 3 >= 0 && c + 3 < SL_YC) dst[r][c + 3] = v.w;
        }
        return;
    }
    for (int i = threadIdx.x; i < SL_YR * SL_YC; i += 256) {
        const int r = i / SL_YC, c = i - r * SL_YC;
        const int gy = y0 + r - SL_HALO, gx = x0 + c - SL_HALO;
        const bool in = gy >= 0 && gy < gm.H && gx >= 0 && gx < gm.W;
        dst[r][c] = in ? src[(long long)gy * gm.W + gx] : 0.0f;
    }
}

// Column pass of K row-filtered maps at column c, rows rb .. rb + SL_RPT - 1: taps in ascending order for every output.
template <int K>
__device__ inline void sl_columns(const SlAcc (&hm)[K][SL_YR][SL_TW], const SlGauss& gw, int rb, int c, SlAcc (&m)[SL_RPT][K]) {
#pragma unroll
    for (int o = 0; o < SL_RPT; ++o)
#pragma unroll
        for (int k = 0; k < K; ++k) m[o][k] = SlAcc(0.0);
#pragma unroll
    for (int j = 0; j < SL_TAPS + SL_RPT - 1; ++j) {
        SlAcc v[K];
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = hm[k][rb + j][c];
#pragma unroll
        for (int o = 0; o < SL_RPT; ++o) {
            if (j - o >= 0 && j - o < SL_TAPS) {
#pragma unroll
                for (int k = 0; k < K; ++k) m[o][k] += gw.g[j - o] * v[k];
            }
        }
    }
}

// grid (planes * tilesY * tilesX), block 256.  part[blockIdx.x] = the sum of S over the tile's pixels inside the image.
// q != nullptr: the derivative maps are stored too (q and r always, p1 / p2 where given).
// No contraction: identical images give bit-equal moments, A1 = B1 and A2 = B2, and S = 1 exactly.
__global__ __launch_bounds__(256) void ssim_loss_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b, SlGeom gm,
                                                            SlGauss gw, float* __restrict__ p1, float* __restrict__ p2,
                                                            float* __restrict__ q, float* __restrict__ r,
                                                            double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ float sa[SL_YR][SL_YC], sb[SL_YR][SL_YC];
    __shared__ SlAcc hm[5][SL_YR][SL_TW];
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % gm.tilesX, ty = (blockIdx.x / gm.tilesX) % gm.tilesY;
    const long long plane = blockIdx.x / ((unsigned)gm.tilesX * (unsigned)gm.tilesY);
    const int x0 = tx * SL_TW, y0 = ty * SL_TH;
    const long long base = plane * ((long long)gm.H * gm.W);

    // 1. a, b over tile + halo
    sl_stage(a + base, gm, y0, x0, sa);
    sl_stage(b + base, gm, y0, x0, sb);
    __syncthreads();

    // 2. row filter of mu1, mu2, E[a^2], E[b^2], E[ab] over every halo row
    for (int i = tid; i < SL_YR * SL_TW; i += 256) {
        const int rr = i / SL_TW, c = i - rr * SL_TW;
        SlAcc m0 = SlAcc(0.0), m1 = SlAcc(0.0), m2 = SlAcc(0.0), m3 = SlAcc(0.0), m4 = SlAcc(0.0);
#pragma unroll
        for (int t = 0; t < SL_TAPS; ++t) {
            const SlAcc g = gw.g[t], x1 = (SlAcc)sa[rr][c + t], x2 = (SlAcc)sb[rr][c + t];
            m0 += g * x1;
            m1 += g * x2;
            m2 += g * (x1 * x1);
            m3 += g * (x2 * x2);
            m4 += g * (x1 * x2);
        }
        hm[0][rr][c] = m0; hm[1][rr][c] = m1; hm[2][rr][c] = m2; hm[3][rr][c] = m3; hm[4][rr][c] = m4;
    }
    __syncthreads();

    // 3. column filter, the map and (for a gradient) its four derivatives
    const int c = tid & (SL_TW - 1), rb = (tid / SL_TW) * SL_RPT;
    SlAcc m[SL_RPT][5];
    sl_columns<5>(hm, gw, rb, c, m);
    const SlAcc C1 = SlAcc(0.01) * SlAcc(0.01), C2 = SlAcc(0.03) * SlAcc(0.03);
    double ssum = 0.0;
#pragma unroll
    for (int o = 0; o < SL_RPT; ++o) {
        const int oy = y0 + rb + o, ox = x0 + c;
        if (oy >= gm.H || ox >= gm.W) continue;
        const SlAcc mu1 = m[o][0], mu2 = m[o][1];
        const SlAcc mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
        const SlAcc A1 = 2 * mu1_mu2 + C1, A2 = 2 * (m[o][4] - mu1_mu2) + C2;
        const SlAcc B1 = mu1_sq + mu2_sq + C1, B2 = (m[o][2] - mu1_sq) + (m[o][3] - mu2_sq) + C2;
        const SlAcc den = B1 * B2;
        const SlAcc S = (A1 * A2) / den;
        ssum += (double)S;
        if (q != nullptr) {
            const long long at = base + (long long)oy * gm.W + ox;
            const SlAcc inv_den = SlAcc(1.0) / den, inv_b2 = SlAcc(1.0) / B2;
            const SlAcc da = SlAcc(2.0) * (A2 - A1) * inv_den, db = SlAcc(2.0) * S * (SlAcc(1.0) / B1 - inv_b2);
            if (p1 != nullptr) p1[at] = (float)(mu2 * da - mu1 * db);
            if (p2 != nullptr) p2[at] = (float)(mu1 * da - mu2 * db);
            q[at] = (float)(-S * inv_b2);
            r[at] = (float)(SlAcc(2.0) * A1 * inv_den);
        }
    }

    // 4. fixed-order workgroup sum -> this tile's slot
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) ssum += __shfl_xor(ssum, off);
    if ((tid & 63) == 0) red[tid >> 6] = ssum;
    __syncthreads();
    if (tid == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// grid (1), block 256: out[0] = float(sum of the `nparts` slots in a fixed order / n) (a division: n ones give exactly 1).
__global__ __launch_bounds__(256) void ssim_loss_finish_kernel(const double* __restrict__ part, long long nparts, double n,
                                                               float* __restrict__ out) {
    __shared__ double rs[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (long long i = tid; i < nparts; i += 256) s += part[i];
    rs[tid] = s;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) rs[tid] += rs[tid + w];
        __syncthreads();
    }
    if (tid == 0) out[0] = (float)(rs[0] / n);
}

// grid (planes * tilesY * tilesX), block 256.  gx = gout[0] * inv_n * [ w * p + 2 x (w * q) + other (w * r) ].
__global__ __launch_bounds__(256) void ssim_loss_bwd_kernel(const float* __restrict__ x, const float* __restrict__ other,
                                                            const float* __restrict__ p, const float* __restrict__ q,
                                                            const float* __restrict__ r, const float* __restrict__ gout,
                                                            float* __restrict__ gx, SlGeom gm, SlGauss gw, SlAcc inv_n) {
    __shared__ float sm[3][SL_YR][SL_YC];
    __shared__ SlAcc hm[3][SL_YR][SL_TW];
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % gm.tilesX, ty = (blockIdx.x / gm.tilesX) % gm.tilesY;
    const long long plane = blockIdx.x / ((unsigned)gm.tilesX * (unsigned)gm.tilesY);
    const int x0 = tx * SL_TW, y0 = ty * SL_TH;
    const long long base = plane * ((long long)gm.H * gm.W);
    const SlAcc scale = (SlAcc)gout[0] * inv_n;

    sl_stage(p + base, gm, y0, x0, sm[0]);
    sl_stage(q + base, gm, y0, x0, sm[1]);
    sl_stage(r + base, gm, y0, x0, sm[2]);
    __syncthreads();

    for (int i = tid; i < SL_YR * SL_TW; i += 256) {
        const int rr = i / SL_TW, c = i - rr * SL_TW;
        SlAcc m0 = SlAcc(0.0), m1 = SlAcc(0.0), m2 = SlAcc(0.0);
#pragma unroll
        for (int t = 0; t < SL_TAPS; ++t) {
            const SlAcc g = gw.g[t];
            m0 += g * (SlAcc)sm[0][rr][c + t];
            m1 += g * (SlAcc)sm[1][rr][c + t];
            m2 += g * (SlAcc)sm[2][rr][c + t];
        }
        hm[0][rr][c] = m0; hm[1][rr][c] = m1; hm[2][rr][c] = m2;
    }
    __syncthreads();

    const int c = tid & (SL_TW - 1), rb = (tid / SL_TW) * SL_RPT;
    SlAcc m[SL_RPT][3];
    sl_columns<3>(hm, gw, rb, c, m);
#pragma unroll
    for (int o = 0; o < SL_RPT; ++o) {
        const int oy = y0 + rb + o, ox = x0 + c;
        if (oy >= gm.H || ox >= gm.W) continue;
        const long long at = base + (long long)oy * gm.W + ox;
        const SlAcc xv = (SlAcc)x[at], ov = (SlAcc)other[at];
        gx[at] = (float)(scale * (m[o][0] + SlAcc(2.0) * xv * m[o][1] + ov * m[o][2]));
    }
}

}  // namespace wm
