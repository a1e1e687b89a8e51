// pw_dw.hip.h - LayerNorm2d, a 1x1 convolution and the depth-wise 3x3 (+ bias) that alone reads its first Cdw output channels, in one
// kernel: the mirror image of dw_pw.hip.h, for gfx950.  x (B, 32, H, W) fp32, NCHW.  One of the row-walking kernels: the scheme,
// what it costs to keep and the shared pieces are in row_walk.hip.h.
//   y[:, :Cdw] = dwconv3x3(conv1x1(LayerNorm2d(x)) + b_pw)[:, :Cdw] + b_dw
//   y[:, Cdw:] = (conv1x1(LayerNorm2d(x)) + b_pw)[:, Cdw:]
//
// Call sites (the two "heads" of an HFE block): norm1 -> attn.qkv (32 -> 96) -> qkv_dwconv on the q | k channels (Cdw = 64; the value
// third leaves as the 1x1 wrote it: dw_pw_kernel reads it later), and norm2 -> ffn.project_in[0] (32 -> 32) -> project_in[1] (Cdw = 32).
// As two launches (conv2d_mfma_kernel<1, ., ., LNIN>, dwconv3x3_kernel<0>) a position moves 1024 / 512 B: the plane between the 1x1 and
// the depth-wise convolution is written once and read once.  Here it never exists: 512 / 256 B.
//
// Bit-identical to the pair; every element takes the pair's path.  LayerNorm: conv2d_mfma_kernel's LNIN block - the mean by plain adds
// and the variance by an fmaf chain, both over the channels in order 0 .. 31, rstd = 1 / sqrtf(var / 32 + eps), then
// fmaf((v - mean) rstd, w, b).  1x1: cv_split<false>, conv2d_prep_kernel's fragments, per 16-channel chunk the three products (cv_mma3)
// onto a zero accumulator, then + bias.  Depth-wise: dw_taps9's chain (dw_chain_step); zero padding is zero, not the 1x1 of a
// normalised zero pixel.
//
// Particular to this kernel: the depth-wise input is a 1x1 OUTPUT, so a strip is HaloStrip<kPwDwCols = 30> on one 32-pixel tile.
// Lane (pixel = lane & 31, k-half = lane >> 5) is the B-operand lane of v_mfma_f32_32x32x16_bf16 and loads, of both 16-channel chunks,
// the 8 channels 16 cc + 8 (lane >> 5) + j of its pixel; the other 16 arrive from lane ^ 32 by v_permlane32_swap, and every lane runs
// the whole 32-term chains.  After the six products of a 32-channel row tile the accumulator holds 16 output channels of the lane's OWN
// pixel, so the horizontal taps are DPP moves (what the first / last pixel lane of a half takes is another channel's: those are the
// halo lanes).  All NT row tiles run in the one wave (LayerNorm once per pixel), so the q | k head carries 64 partial sums.  Beside the
// taps, the 1x1 fragments, the bias and the LayerNorm weights are re-read from LDS per row; an x row is loaded two rows ahead of its use
// (two register buffers, the loop unrolled by two).  H W < 2^25: a 32-plane output tile is one raw buffer of less than 2^32 bytes.
#pragma once
#include "conv2d.hip.h"
#include "row_walk.hip.h"

namespace wm {

struct PwDwArgs {
    const float* x;                   // (B, 32, H, W)
    const float* ln_w;                // (32) LayerNorm2d weight, bias
    const float* ln_b;
    float ln_eps;
    const uint4* wfrag;               // conv2d_prep_kernel output of the (32 NT, 32, 1, 1) weight
    const float* bias;                // (32 NT) or null
    const float* dw_w;                // (32 NDW, 1, 3, 3)
    const float* dw_b;                // (32 NDW) or null
    float* y;                         // (B, 32 NT, H, W)
    int H, W;                         // H W < 2^25
    int nstrips, nbands, rows;        // kPwDwCols-column strips, bands of `rows` output rows
    long long nwalks;                 // B * nbands * nstrips (strips fastest)
};

constexpr int kPwDwCols = kCvTW - 2;   // output columns per strip

// NT: 32-channel row tiles of the 1x1 (Cout = 32 NT); NDW: the first NDW of them pass through the depth-wise convolution
template <int NT, int NDW>
__global__ __launch_bounds__(256, 2) void pw_dw_kernel(const PwDwArgs a) {
    static_assert(NDW >= 1 && NDW <= NT, "the depth-wise convolution reads the first NDW row tiles");
    constexpr int C = 32;
    __shared__ uint4 s_A[2 * NT * 2 * 64];                               // prepared 1x1 weights: [chunk][tile][split][lane]
    __shared__ __attribute__((aligned(16))) float s_tap[NDW * 32 * 12];  // [channel][9 taps | bias | 0 0]
    __shared__ __attribute__((aligned(16))) float s_bias[NT * 32];       // 1x1 bias in accumulator order: [tile][lane >> 5][register]
    __shared__ __attribute__((aligned(16))) float s_ln[2 * 2 * 16];      // [lane >> 5][weight | bias][8 cc + j] of channel 16 cc + 8 (lane >> 5) + j
    const int lane = threadIdx.x & 63, px = lane & 31, kh = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const RowWalk wk = row_walk(a.nwalks, a.nstrips, a.nbands, wv);
    const int H = a.H, W = a.W, HW = H * W;
    const float* __restrict__ xb = a.x + wk.b * C * HW;
    float* __restrict__ yb = a.y + wk.b * (NT * 32) * HW;

    const HaloStrip<kPwDwCols> hs(wk.strip, px, W);
    const unsigned xoff = 4u * (8 * kh * HW + hs.colc(W));
    // a row tile's 32 output planes as one raw buffer; D layout: row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) - the lane's part of
    // it in the lane's offset, the register's in the scalar offset; an offset >= nrec is dropped
    const unsigned plane_bytes = 4u * HW, nrec = 32u * plane_bytes;
    const unsigned lane_off = 4u * (4 * kh * HW + min(hs.col, W - 1));
    __amdgpu_buffer_rsrc_t rs[NT];
#pragma unroll
    for (int m = 0; m < NT; ++m) rs[m] = raw_rsrc(yb + (long long)m * 32 * HW, (int)nrec);

    const int r0 = wk.band * a.rows, r_end = min(H, r0 + a.rows);
    auto load_row = [&](int rho, float (&nx)[16]) {                     // channel 16 cc + 8 kh + j at [8 cc + j]; clamped, masked when consumed
        const unsigned ro = 4u * (min(max(rho, 0), H - 1) * W);
#pragma unroll
        for (int c = 0; c < 16; ++c) nx[c] = *at_bytes(xb + (16 * (c >> 3) + (c & 7)) * HW, xoff + ro);
    };
    float nxa[16], nxb[16];
    load_row(r0 - 1, nxa);                                              // on their way while the workgroup stages its constants
    __builtin_amdgcn_sched_barrier(0);
    load_row(r0, nxb);
    __builtin_amdgcn_sched_barrier(0);

    cv_stage_acc_bias<NT>(s_bias, a.bias);
    stage_dw_taps<NDW * 32>(s_tap, a.dw_w, a.dw_b);
    if (threadIdx.x < 64) {
        const int h = threadIdx.x >> 5, e = threadIdx.x & 15, c = 16 * (e >> 3) + 8 * h + (e & 7);
        s_ln[threadIdx.x] = (threadIdx.x & 16) ? a.ln_b[c] : a.ln_w[c];
    }
    for (int i = threadIdx.x; i < 2 * NT * 2 * 64; i += 256) s_A[i] = a.wfrag[i];
    __syncthreads();
    if (!wk.live) return;

    // the chains of output rows r + 1 (p0: bias + kernel row 0 so far) and r (p1: + kernel row 1) after x row r, of channel
    // 32 m + 4 kh + (i & 3) + 8 (i >> 2) at [16 m + i]
    float p0[NDW * 16], p1[NDW * 16];
#pragma unroll
    for (int q = 0; q < NDW * 16; ++q) p0[q] = p1[q] = 0.0f;           // (the band's first two x rows end and continue rows above it: not stored)

    // x row rho (in `nx`) enters the window: output row rho - 1 of the depth-wise tiles and row rho of the others leave
    auto step = [&](int rho, float (&nx)[16]) {
        int lo = lane, ko = kh;                                         // opaque: what is read from LDS through them stays in the loop
        asm volatile("" : "+v"(lo), "+v"(ko));
        Frag16 Bh[2], Bl[2];
        {   // LayerNorm2d of the lane's pixel: all 32 channels, in channel order
            float f[32];
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(nx[c]), __float_as_uint(nx[c]), false, false);
                f[16 * (c >> 3) + (c & 7)] = __uint_as_float(r[0]);     // the lower half's: channel 16 cc + j
                f[16 * (c >> 3) + 8 + (c & 7)] = __uint_as_float(r[1]); // the upper half's: channel 16 cc + 8 + j
            }
            float mean = 0.0f;
#pragma unroll
            for (int c = 0; c < 32; ++c) mean += f[c];
            mean *= (1.0f / 32.0f);
            float var = 0.0f;
#pragma unroll
            for (int c = 0; c < 32; ++c) { const float q = f[c] - mean; var = fmaf(q, q, var); }
            const float rstd = 1.0f / sqrtf(var * (1.0f / 32.0f) + a.ln_eps);
            const float4* l4 = reinterpret_cast<const float4*>(s_ln + 32 * ko);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 wq = l4[q], bq = l4[4 + q];
                const float lw[4] = {wq.x, wq.y, wq.z, wq.w}, lb[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = 4 * q + j;
                    cv_split<false>(fmaf((nx[c] - mean) * rstd, lw[j], lb[j]), Bh[c >> 3], Bl[c >> 3], c & 7);
                }
            }
        }
        load_row(rho + 2, nx);                                          // two rows ahead, ahead of this row's stores
        __builtin_amdgcn_sched_barrier(0);
        const bool rowin = rho >= 0 && rho < H;                         // (wave-uniform)
        const bool keep = hs.colin && rowin;                               // else: zero padding
        const bool orow_dw = rho - 1 >= r0 && rho - 1 < r_end, orow_pw = rho >= r0 && rho < r_end;
        const unsigned voff_dw = (hs.st_ok && orow_dw) ? lane_off + 4u * ((rho - 1) * W) : nrec;
        const unsigned voff_pw = (hs.st_ok && orow_pw) ? lane_off + 4u * (rho * W) : nrec;
#pragma unroll
        for (int m = 0; m < NT; ++m) {
            f32x16_t acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                Frag16 Ah, Al;
                Ah.u = s_A[((cc * NT + m) * 2 + 0) * 64 + lo];
                Al.u = s_A[((cc * NT + m) * 2 + 1) * 64 + lo];
                acc = cv_mma3(Ah, Al, Bh[cc], Bl[cc], acc);
            }
            const float4* b4 = reinterpret_cast<const float4*>(s_bias + 32 * m + 16 * ko);
            const float* tap = s_tap + (32 * m + 4 * ko) * 12;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 bq = b4[q];
                const float bv[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i = 4 * q + j, ch = cv_acc_row(i);
                    float v = acc[i] + bv[j];
                    if (m < NDW) {
                        asm("" : "+v"(v));                             // the value the pair stored: the depth-wise chains start from these bits
                        const float xm = keep ? v : 0.0f;
                        const float t3[3] = {dpp_from_lower_lane(0.0f, xm), xm, dpp_from_upper_lane(0.0f, xm)};
                        float t[10];
                        load_dw_taps(tap, ch, t);
                        const int pq = 16 * (m < NDW ? m : 0) + i;
                        v = dw_chain_step(p0[pq], p1[pq], t, t3);
                        asm volatile("" : "+v"(p0[pq]), "+v"(p1[pq]));   // (pinned where they are formed)
                    }
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs[m], (int)(m < NDW ? voff_dw : voff_pw),
                                                          (int)(ch * plane_bytes), 0);
                    if (m < NDW) __builtin_amdgcn_sched_barrier(0);     // one channel's taps and neighbours in registers at a time
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };

#pragma unroll 1
    for (int rho = r0 - 1; rho <= r_end; rho += 2) {                    // (an odd count's last step is one row past the band: nothing stored)
        step(rho, nxa);
        step(rho + 1, nxb);
    }
}

}  // namespace wm
