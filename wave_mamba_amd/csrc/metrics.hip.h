// metrics.hip.h - Y-channel PSNR and SSIM of uint8 image pairs (the reference's evaluation metrics) for gfx950.
//
// Reference: comput_psnr_ssim.py as inference_wavemamba.py:116-117 calls it (crop_border = 1, test_y_channel = True):
//   crop img[c:-c, c:-c] (:426-428, :642-644) -> to_y_channel (:374-385 -> matlab_functions.bgr2ycbcr, y_only):
//     x = float32(u8) / 255 (float32);  y64 = ((x_b 24.966 + x_g 128.553) + x_r 65.481) + 16 (float64);
//     Y = float32(float32(y64 / 255) * 255)
//   PSNR (:430-438): 20 log10(255 / sqrt(mean((Y1 - Y2)^2))), inf when the mean is 0.  The reference forms this mean in float32
//     (its Y planes are float32); here it is float64 (~5e-6 dB apart at UHD).
//   SSIM (_ssim_cly :558-593): float64; window outer(g, g), g = cv2.getGaussianKernel(11, 1.5); cv2.filter2D with
//     BORDER_REPLICATE (same size, no trim) of Y1, Y2, Y1^2, Y2^2, Y1 Y2; C1 = (0.01 255)^2, C2 = (0.03 255)^2; the map's mean.
//
// One fused pass per TH x TW output tile: Y of both images over the tile and its 5-pixel halo (indices clamped to the crop
// window = the replicate border) into LDS as float32 (Y is exactly a float32), the 11-tap row filter of the five moments into LDS
// as float64, the 11-tap column filter and the SSIM map in registers, and per-workgroup float64 sums of the map and of
// (Y1 - Y2)^2 written to a workspace.  A second kernel adds each image's partials in a fixed order: no atomics, so two calls give
// bit-identical results; nothing is zeroed, nothing is synchronised (capturable into a graph).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wm {

constexpr int MET_TW = 32, MET_TH = 24, MET_HALO = 5, MET_TAPS = 11;
constexpr int MET_YR = MET_TH + 2 * MET_HALO, MET_YC = MET_TW + 2 * MET_HALO;   // 34 x 42 Y values per image

struct MetGauss {
    double g[MET_TAPS];           // the normalised 1-D window (host-computed: exp(-(i - 5)^2 / 4.5) / sum)
};

// Strided uint8 image batch: element (n, h, w, ch) at n * sn + h * sh + w * sw + ch * sc (HWC and CHW alike).
struct MetImage {
    long long sn, sh, sw, sc;
    int cb, cr;                   // channel index of blue / red (BGR: 0 / 2, RGB: 2 / 0)
};

// The reference's Y chain, bit for bit: no fused multiply-adds (hipcc contracts by default).
__device__ inline float met_y_of(const uint8_t* __restrict__ px, const MetImage& im) {
#pragma clang fp contract(off)
    const float xb = (float)px[im.cb * im.sc] / 255.0f;
    const float xg = (float)px[im.sc] / 255.0f;
    const float xr = (float)px[im.cr * im.sc] / 255.0f;
    const double y64 = (((double)xb * 24.966 + (double)xg * 128.553) + (double)xr * 65.481) + 16.0;
    const float y = (float)(y64 / 255.0);
    return y * 255.0f;
}

// SSIM map at one pixel from the five filtered moments (no contraction: identical images give exactly 1).
__device__ inline double met_ssim_of(double mu1, double mu2, double e11, double e22, double e12) {
#pragma clang fp contract(off)
    const double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
    const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
    const double s1 = e11 - mu1_sq, s2 = e22 - mu2_sq, s12 = e12 - mu1_mu2;
    return ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2));
}

// grid (ceil(Wc / TW), ceil(Hc / TH), N), block 256.  a, b: the images; (Hc, Wc) the crop window starting at (crop, crop).
// part[((n * tilesY + ty) * tilesX + tx) * 2 + {0, 1}] = (sum of the SSIM map, sum of (Y1 - Y2)^2) over the tile's valid pixels.
__global__ __launch_bounds__(256) void psnr_ssim_tile_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, MetImage im,
                                                             int crop, int Hc, int Wc, MetGauss gw, double* __restrict__ part) {
    __shared__ float ya[MET_YR][MET_YC], yb[MET_YR][MET_YC];
    __shared__ double hm[5][MET_YR][MET_TW];
    __shared__ double red[2][4];
    const int tid = threadIdx.x, n = blockIdx.z;
    const int x0 = blockIdx.x * MET_TW, y0 = blockIdx.y * MET_TH;
    const long long base = (long long)n * im.sn;

    // 1. Y over tile + halo, indices clamped to the window (BORDER_REPLICATE)
    for (int i = tid; i < MET_YR * MET_YC; i += 256) {
        const int r = i / MET_YC, c = i - r * MET_YC;
        const int gy = min(max(y0 + r - MET_HALO, 0), Hc - 1), gx = min(max(x0 + c - MET_HALO, 0), Wc - 1);
        const long long off = base + (long long)(crop + gy) * im.sh + (long long)(crop + gx) * im.sw;
        ya[r][c] = met_y_of(a + off, im);
        yb[r][c] = met_y_of(b + off, im);
    }
    __syncthreads();

    // 2. row filter of mu1, mu2, E[x1^2], E[x2^2], E[x1 x2] over every halo row; (Y1 - Y2)^2 at the valid tile pixels
    double dsum = 0.0;
    for (int i = tid; i < MET_YR * MET_TW; i += 256) {
        const int r = i / MET_TW, c = i - r * MET_TW;
        double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
#pragma unroll
        for (int t = 0; t < MET_TAPS; ++t) {
            const double g = gw.g[t], x1 = (double)ya[r][c + t], x2 = (double)yb[r][c + t];
            m0 += g * x1;
            m1 += g * x2;
            m2 += g * (x1 * x1);
            m3 += g * (x2 * x2);
            m4 += g * (x1 * x2);
        }
        hm[0][r][c] = m0; hm[1][r][c] = m1; hm[2][r][c] = m2; hm[3][r][c] = m3; hm[4][r][c] = m4;
        const int oy = y0 + r - MET_HALO;
        if (r >= MET_HALO && r < MET_HALO + MET_TH && oy < Hc && x0 + c < Wc) {
            const double d = (double)ya[r][c + MET_HALO] - (double)yb[r][c + MET_HALO];
            dsum += d * d;
        }
    }
    __syncthreads();

    // 3. column filter + SSIM map over the valid tile pixels
    double ssum = 0.0;
    for (int i = tid; i < MET_TH * MET_TW; i += 256) {
        const int r = i / MET_TW, c = i - r * MET_TW;
        if (y0 + r >= Hc || x0 + c >= Wc) continue;
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int t = 0; t < MET_TAPS; ++t) {
            const double g = gw.g[t];
#pragma unroll
            for (int k = 0; k < 5; ++k) m[k] += g * hm[k][r + t][c];
        }
        ssum += met_ssim_of(m[0], m[1], m[2], m[3], m[4]);
    }

    // 4. fixed-order workgroup sums -> this tile's partials
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        ssum += __shfl_xor(ssum, off);
        dsum += __shfl_xor(dsum, off);
    }
    if ((tid & 63) == 0) { red[0][tid >> 6] = ssum; red[1][tid >> 6] = dsum; }
    __syncthreads();
    if (tid == 0) {
        const long long p = ((long long)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        part[2 * p] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        part[2 * p + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

// grid (N), block 256: out[n] = (PSNR, SSIM) from the `tiles` partials of image n, summed in a fixed order.
__global__ __launch_bounds__(256) void psnr_ssim_finish_kernel(const double* __restrict__ part, int tiles, double npix,
                                                               double* __restrict__ out) {
    __shared__ double rs[256], rd[256];
    const int tid = threadIdx.x, n = blockIdx.x;
    const double* p = part + 2 * (long long)n * tiles;
    double s = 0.0, d = 0.0;
    for (int i = tid; i < tiles; i += 256) { s += p[2 * i]; d += p[2 * i + 1]; }
    rs[tid] = s; rd[tid] = d;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) { rs[tid] += rs[tid + w]; rd[tid] += rd[tid + w]; }
        __syncthreads();
    }
    if (tid == 0) {
        const double mse = rd[0] / npix;
        out[2 * n] = mse == 0.0 ? (double)INFINITY : 20.0 * log10(255.0 / sqrt(mse));
        out[2 * n + 1] = rs[0] / npix;
    }
}

// y (N, H, W) float32 = to_y_channel of every pixel; grid-stride over N H W pixels, block 256.
__global__ __launch_bounds__(256) void y_channel_kernel(const uint8_t* __restrict__ img, MetImage im, int H, int W, long long total,
                                                        float* __restrict__ y) {
    const long long hw = (long long)H * W;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long n = i / hw, rem = i - n * hw, h = rem / W, w = rem - h * W;
        y[i] = met_y_of(img + n * im.sn + h * im.sh + w * im.sw, im);
    }
}

}  // namespace wm
