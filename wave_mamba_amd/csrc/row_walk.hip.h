// row_walk.hip.h - what the row-walking fused kernels share, for gfx950: lfss_in_conv_mfma_kernel and lfss_ffn_mfma_kernel
// (lfss_mfma.hip.h), dw_pw_kernel (dw_pw.hip.h) and pw_dw_kernel (pw_dw.hip.h).  Each folds a depth-wise 3x3 convolution into the
// 1x1 projection before or behind it, bit-identical to the unfused pair, so that the plane between the two never reaches memory.
//
// The scheme.  A wave owns a strip of columns and a band of output rows - a walk = (batch, band, strip), strips fastest - and
// meets each input row of the band (and one above, one below) once, top to bottom.  A lane is one pixel of the row: the horizontal
// taps come from the adjacent lanes by DPP (dwconv.hip.h), the vertical direction is three running dw_taps3 chains per channel -
// row r closes output row r - 1, continues row r and opens row r + 1, so two partial sums per channel live across rows and every
// output is dw_taps9's one fmaf chain.  Where the depth-wise input is itself a 1x1 OUTPUT the halo is recomputed, not loaded: the
// strip's first and last pixel lanes are halo columns that store nothing (HaloStrip), strips overlap by one column each side and
// bands by one row each side.
//
// What these kernels paid for, stated once (each kernel's comment names only what is particular to it):
//   * no branch around a memory operation in the row loop: loads come from clamped addresses and are masked where the row is
//     consumed (zero padding enters the chains as zero operands); stores are raw buffer stores whose offset is out of range for
//     a halo lane, a column past the image and a row outside the band.  Every address lies inside its tensor at every shape;
//   * addresses are wave-uniform plane bases (scalar registers) plus an unsigned 32-bit BYTE offset per lane (at_bytes): no
//     64-bit address arithmetic per access;
//   * constants are re-read from LDS per row behind an opaque offset (asm volatile at the site, the offset passed in): hoisted
//     out of the row loop - the compiler's choice for loop-invariant reads - they fill the register file and spill;
//   * the partial sums are pinned where they are formed (asm volatile at the site, behind dw_chain_step): they are read in the
//     next row only, and the optimiser otherwise sinks them - the channel's taps and neighbours with them - below the stores;
//   * one channel's (or pair's) taps and neighbours in registers at a time: a sched_barrier per channel, else all spill;
//   * a row is loaded ahead of its use into the registers the row just consumed leaves free, ahead of the row's stores;
//   * workgroup ids are dealt to the XCDs in contiguous runs (row_walk), so that neighbouring strips and bands share an L2.
//
// The pieces (each written once):
//   at_bytes                           element at a byte offset of a wave-uniform base
//   row_walk                           workgroup and wave -> live, (batch, band, strip); the XCD deal
//   HaloStrip                          a lane's column in an (N + 2)-lane strip that stores N columns: col, colin, st_ok, colc()
//   stage_dw_taps, load_dw_taps        the tap table [channel][9 taps | bias | 0 0] in LDS; one channel's ten values from it
//   dw_chain_step                      the three-chain update of one channel with one input row
// and beside them: dw_taps3 / dw_taps9, the DPP moves and raw_rsrc (dwconv.hip.h); cv_mma3, cv_acc_row and cv_stage_acc_bias for the
// split 1x1 of dw_pw / pw_dw (conv2d.hip.h, which defines a kernel and so stays out of the LFSS unit); RowWalkGeom,
// row_walk_geom and row_walk_band_rows on the host (host_common.h).
#pragma once
#include <hip/hip_runtime.h>
#include "dwconv.hip.h"        // dw_taps3

namespace wm {

// element at BYTE offset `boff` of a wave-uniform base
__device__ __forceinline__ const float* at_bytes(const float* base, unsigned boff) {
    return reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + boff);
}
__device__ __forceinline__ float* at_bytes(float* base, unsigned boff) {
    return reinterpret_cast<float*>(reinterpret_cast<char*>(base) + boff);
}

// Wave `wv` of this workgroup -> its walk.  Workgroup q runs on XCD q mod 8 (each with a private L2): every XCD gets a contiguous
// run of walks, so the rows a band shares with the next and the columns a strip shares with the next come from the L2 that a
// neighbouring workgroup of the same XCD filled.  Four walks per workgroup; the grid is a multiple of 8 (row_walk_geom).  A wave
// past the last walk is not `live`: it takes the last walk's addresses (its loads ahead of the staging barrier stay inside the
// tensors), helps stage the constants, and returns behind the barrier without a store.
struct RowWalk { bool live; int strip, band; long long b; };
__device__ __forceinline__ RowWalk row_walk(long long nwalks, int nstrips, int nbands, int wv) {
    const long long blk = (long long)(blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    const bool live = blk * 4 + wv < nwalks;
    const long long wk = live ? blk * 4 + wv : nwalks - 1;             // walk = (batch, band, strip), strips fastest
    const int strip = (int)(wk % nstrips);
    const long long wb = wk / nstrips;
    return {live, strip, (int)(wb % nbands), wb / nbands};
}

// Pixel lane `px` of an (N + 2)-lane strip that stores N columns: lanes 0 and N + 1 are the halo columns.
template <int N>
struct HaloStrip {
    int col;                           // the lane's image column
    bool colin, st_ok;                 // inside the image (else zero padding); the lane stores
    __device__ __forceinline__ HaloStrip(int strip, int px, int W)
        : col(strip * N - 1 + px), colin(col >= 0 && col < W), st_ok(px >= 1 && px <= N && col < W) {}
    __device__ __forceinline__ int colc(int W) const { return min(max(col, 0), W - 1); }      // clamped into the image (loads)
};

// The depth-wise taps of NC channels as [channel][9 taps | bias | 0 0] (all 256 threads, before the staging barrier): a channel is
// three ds_read_b128 (load_dw_taps; `s_tap` may carry the site's opaque offset).
template <int NC>
__device__ __forceinline__ void stage_dw_taps(float* s_tap, const float* __restrict__ w /*(NC, 3, 3)*/, const float* __restrict__ bias /*(NC) or null*/) {
    for (int e = threadIdx.x; e < NC * 12; e += 256) {
        const int c = e / 12, q = e - 12 * c;
        s_tap[e] = q < 9 ? w[c * 9 + q] : (q == 9 && bias ? bias[c] : 0.0f);
    }
}
__device__ __forceinline__ void load_dw_taps(const float* s_tap, int c, float (&w)[10] /* 9 taps, bias */) {
    const float* wk = s_tap + c * 12;
    const float4 w0 = *reinterpret_cast<const float4*>(wk), w1 = *reinterpret_cast<const float4*>(wk + 4),
                 w2 = *reinterpret_cast<const float4*>(wk + 8);
    w[0] = w0.x; w[1] = w0.y; w[2] = w0.z; w[3] = w0.w; w[4] = w1.x; w[5] = w1.y; w[6] = w1.z; w[7] = w1.w; w[8] = w2.x; w[9] = w2.y;
}

// Input row `row` (left, centre, right) of one channel with taps `t` (load_dw_taps): closes the chain of the output row above
// with kernel row 2 (returned), continues this row's (p1) with kernel row 1 and opens the next row's (p0) from the bias with
// kernel row 0.  The caller pins p0 and p1 behind it.
__device__ __forceinline__ float dw_chain_step(float& p0, float& p1, const float* t, const float* row) {
    const float v = dw_taps3(p1, t + 6, row);
    p1 = dw_taps3(p0, t + 3, row);
    p0 = dw_taps3(t[9], t, row);
    return v;
}

}  // namespace wm
