// dw_pw.hip.h - a depth-wise 3x3 convolution (+ bias, + optional exact GELU) folded into the 1x1 convolution that is its only
// reader:  y = conv1x1(act(dwconv3x3(x) + b_dw)) + b_pw (+ residual),  32 -> 32 channels, NCHW fp32, for gfx950.  One of the
// row-walking kernels: the scheme, what it costs to keep and the shared pieces are in row_walk.hip.h.
//
// Call sites (HFE branch): FeedForward.project_out = [depth-wise 3x3, GELU, 1x1] with the block's residual, and the value third
// of CMTAttention.qkv_dwconv under the folded project_out.  As two launches (dwconv3x3_kernel, conv2d_mfma_kernel<1, 4, 1>) a
// position moves 640 B: the 32-channel plane between them is written once and read once.  Here it never exists: 384 B.
//
// Bit-identical to the pair.  Every element takes the pair's path: dw_taps9's chain (dw_chain_step), gelu_erf, cv_split<false>,
// then per 16-channel chunk the three products (cv_mma3) onto a zero accumulator, then + bias, then + residual.
//
// Particular to this kernel: the depth-wise input is LOADED, so a strip is 32 whole columns with no halo lanes.  Lane (pixel =
// lane & 31, k-half = lane >> 5) is the B-operand lane of v_mfma_f32_32x32x16_bf16 for its pixel and holds, of both chunks, the 8
// channels 16 cc + 8 (lane >> 5) + j: it forms the depth-wise values of exactly those 16 channels, so the B fragments are built in
// registers - no staging through LDS.  An input row is one 128-byte load per channel and half-wave; in a half's first / last lane
// the DPP neighbour is the other half's pixel 31 / 0, another channel: those take the strip's outer columns from one more load per
// channel, as lfss_out_conv_acc_kernel does.  A band re-reads two rows of its neighbours, from cache.  LDS holds only constants:
// the taps, the prepared 1x1 weights and the bias.
#pragma once
#include <type_traits>
#include "conv2d.hip.h"
#include "row_walk.hip.h"

namespace wm {

struct DwPwArgs {
    const float* x;                   // (B, >= 32, H, W): channel 0 of the 32 input planes of batch element 0
    long long xbs;                    // its batch stride in elements (a channel slice of a wider tensor: not 32 H W)
    const float* dw_w;                // (32, 1, 3, 3)
    const float* dw_b;                // (32) or null
    const uint4* wfrag;               // conv2d_prep_kernel output of the (32, 32, 1, 1) weight
    const float* bias;                // (32) or null
    const float* res;                 // (B, 32, H, W) or null
    float* y;                         // (B, 32, H, W)
    int H, W;                         // 32 H W < 2^31: offsets inside a batch element are 32-bit
    int nstrips, nbands, rows;        // 32-column strips, bands of `rows` output rows
    long long nwalks;                 // B * nbands * nstrips (strips fastest)
};

#ifndef WM_DWPW_WAVES
#define WM_DWPW_WAVES 3                // waves per SIMD the register allocation aims at
#endif

template <bool GELU, bool RES>
__global__ __launch_bounds__(256, WM_DWPW_WAVES) void dw_pw_kernel(const DwPwArgs a) {
    constexpr int C = 32;
    __shared__ __attribute__((aligned(16))) float s_tap[C * 12];      // [channel][9 taps | bias | 0 0]
    __shared__ uint4 s_A[4 * 64];                                      // prepared 1x1 weights: [chunk][split][lane]
    __shared__ __attribute__((aligned(16))) float s_bias[C];          // 1x1 bias in accumulator order: [lane >> 5][register]
    const int lane = threadIdx.x & 63, px = lane & 31, kh = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const RowWalk wk = row_walk(a.nwalks, a.nstrips, a.nbands, wv);
    const int H = a.H, W = a.W, HW = H * W;
    const float* __restrict__ xb = a.x + wk.b * a.xbs;
    const float* __restrict__ rb = RES ? a.res + wk.b * C * HW : nullptr;
    float* __restrict__ yb = a.y + wk.b * C * HW;

    // the lane's column, and the outer column of its side of the strip (clamped: loads are unconditional, masked when consumed)
    const int col = wk.strip * kCvTW + px;
    const bool colok = col < W;
    const int hcol = wk.strip * kCvTW + (px < 16 ? -1 : kCvTW);
    const bool hok = hcol >= 0 && hcol < W;
    // byte offsets per lane: 9 H W floats at the most, H W < 2^26 keeps them below 2^32
    const unsigned xoff = 4u * (8 * kh * HW + min(col, W - 1)), xhoff = 4u * (8 * kh * HW + min(max(hcol, 0), W - 1));
    const unsigned ooff = 4u * (4 * kh * HW + min(col, W - 1));        // D layout: row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)

    const int h0 = wk.band * a.rows, hend = min(H, h0 + a.rows);
    float cur[16], ecur[16];                                           // channel 16 cc + 8 kh + j at [8 cc + j]: centre, outer column
    {   // the band's first input row is on its way while the workgroup stages its constants
        const unsigned ro = 4u * (min(max(h0 - 1, 0), H - 1) * W);
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const float* __restrict__ pl = xb + (16 * (c >> 3) + (c & 7)) * HW;
            cur[c] = *at_bytes(pl, xoff + ro);
            ecur[c] = *at_bytes(pl, xhoff + ro);
        }
    }
    cv_stage_acc_bias<1>(s_bias, a.bias);
    stage_dw_taps<C>(s_tap, a.dw_w, a.dw_b);
    s_A[threadIdx.x] = a.wfrag[threadIdx.x];
    __syncthreads();
    if (!wk.live) return;

    float p0[16], p1[16];                                              // chains of output rows r + 1 and r after input row r
#pragma unroll
    for (int c = 0; c < 16; ++c) p0[c] = p1[c] = 0.0f;

    // input row r is in `cur` / `ecur`; each channel's registers take row r + 1 as soon as they are consumed, so a row's loads
    // have one row's arithmetic to arrive in and no second set of registers.  EMIT closes output row r - 1.
    auto step = [&](int r, auto emit_c) {
        constexpr bool EMIT = decltype(emit_c)::value;
        const unsigned oro = 4u * (max(r - 1, 0) * W), ron = 4u * (min(max(r + 1, 0), H - 1) * W);
        float rv[16];
        const bool rowok = r >= 0 && r < H;                            // uniform
        const bool ok = rowok && colok, eok = rowok && hok;
        Frag16 Bh[2], Bl[2];
        // the lane's 160 taps stay in the loop behind an opaque per-lane OFFSET: the pointer stays an LDS pointer and the channel
        // offsets land in the instructions' offset fields
        int toff = 8 * kh * 12;
        asm volatile("" : "+v"(toff));
        const float* tap = s_tap + toff;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            if constexpr (EMIT && RES) if (c == 8) {                                // the row's residual: half a row of arithmetic ahead of its use
#pragma unroll
                for (int i = 0; i < 16; ++i) rv[i] = *at_bytes(rb + (cv_acc_row(i)) * HW, ooff + oro);
            }
            float t[10];
            load_dw_taps(tap, 16 * (c >> 3) + (c & 7), t);
            const float cv = ok ? cur[c] : 0.0f, ev = eok ? ecur[c] : 0.0f;
            const float* __restrict__ pl = xb + (16 * (c >> 3) + (c & 7)) * HW;      // wave-uniform plane base
            cur[c] = *at_bytes(pl, xoff + ron);
            ecur[c] = *at_bytes(pl, xhoff + ron);
            float left = dpp_from_lower_lane(cv, cv), right = dpp_from_upper_lane(cv, cv);
            if (px == 0) left = ev;
            if (px == kCvTW - 1) right = ev;
            const float row[3] = {left, cv, right};
            float v = dw_chain_step(p0[c], p1[c], t, row);
            asm volatile("" : "+v"(p0[c]), "+v"(p1[c]));               // (pinned where they are formed)
            if constexpr (EMIT) {
                if constexpr (GELU) v = gelu_erf(v);
                asm("" : "+v"(v));                                     // the value the pair stored: the split below starts from these bits
                cv_split<false>(v, Bh[c >> 3], Bl[c >> 3], c & 7);
            }
            __builtin_amdgcn_sched_barrier(0);                         // one channel's temporaries at a time
        }
        if constexpr (EMIT) {
            f32x16_t acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                Frag16 Ah, Al;
                Ah.u = s_A[(cc * 2 + 0) * 64 + lane];
                Al.u = s_A[(cc * 2 + 1) * 64 + lane];
                acc = cv_mma3(Ah, Al, Bh[cc], Bl[cc], acc);
            }
            const float4* b4 = reinterpret_cast<const float4*>(s_bias + 16 * kh);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 bq = b4[q];
                const float bv[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i = 4 * q + j;
                    float v = acc[i] + bv[j];
                    if constexpr (RES) v += rv[i];
                    if (colok) *at_bytes(yb + (cv_acc_row(i)) * HW, ooff + oro) = v;
                }
            }
        }
    };

    step(h0 - 1, std::false_type{});
    step(h0, std::false_type{});
#pragma unroll 1
    for (int r = h0 + 1; r <= hend; ++r) step(r, std::true_type{});
}

}  // namespace wm
