// scan_bwd_pieces.hip.h - what the two scan backwards share: the op-boundary scan (selscan_bwd.hip.h, a lane holds all NP
// states of its channel) and the fused SS2D core (ss2d_core_bwd.hip.h, a lane of wave w holds states 8 w .. 8 w + 7).
// Math and the two-level L-split: selscan_bwd.hip.h.  NH is the number of packed state PAIRS a lane holds, `p` either
// argument record (same workspace fields), `row` the lane's first chain.  Each kernel keeps its own text of the step
// arithmetic, the carry-in, the chunk's start record and start state, the forward sweep, its s_hs layout, its channel reduction,
// tile loading and the closing of the steps: as functions they change the kernels' loops (profiles/scan_bwd_pieces/README.md).
#pragma once
#include "selscan.hip.h"

namespace wm {

constexpr int kBT = 16;            // steps per backward chunk (= one LDS tile)
constexpr int kBS = 4;             // steps per register sub-tile
constexpr int kBRow = 20;          // padded LDS row

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float row_sum16(float x) {       // every lane of a 16-lane row gets the row sum
    x += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(x), 0x128, 0xf, 0xf, false));  // row_ror:8
    x += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(x), 0x124, 0xf, 0xf, false));
    x += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(x), 0x122, 0xf, 0xf, false));
    x += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(x), 0x121, 0xf, 0xf, false));
    return x;
}
// N (32 or 16) per-lane values -> their sums over the 64 lanes; afterwards every lane of 16-lane row r holds the totals of
// values (N / 4) r .. (N / 4) r + N / 4 - 1 in out: v_permlane32_swap, v_permlane16_swap, then the row sums
template <int N>
__device__ __forceinline__ void wave_reduce(const float (&v)[N], float (&out)[N / 4]) {
    float r1[N / 2];
#pragma unroll
    for (int j = 0; j < N / 2; ++j) {
        const u32x2 s = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[j]), __float_as_uint(v[j + N / 2]), false, false);
        r1[j] = __uint_as_float(s.x) + __uint_as_float(s.y);
    }
#pragma unroll
    for (int j = 0; j < N / 4; ++j) {
        const u32x2 s = __builtin_amdgcn_permlane16_swap(__float_as_uint(r1[j]), __float_as_uint(r1[j + N / 4]), false, false);
        out[j] = row_sum16(__uint_as_float(s.x) + __uint_as_float(s.y));
    }
}

// 16-byte load that is UNCONDITIONAL (clamped to the array's first element when `ok` is false) and zeroed afterwards: an
// `ok ? load : 0` compiles to a branch around the load with an s_waitcnt vmcnt(0) right behind it, so a tile's loads went
// out one at a time, each waiting out its own latency (tools/train_breakdown.py --detail: the kernels of this file had a
// floor of 30 / 63 us per launch however small the map).
__device__ __forceinline__ float4 bwd_ld4(const float* __restrict__ base, long long off, bool ok) {
    const float4 v = *reinterpret_cast<const float4*>(base + (ok ? off : 0LL));
    return make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
}

// two state pairs -> the four floats they are stored as
__device__ __forceinline__ float4 pack4(v2f a, v2f b) { return make_float4(a.x, a.y, b.x, b.y); }
template <int NH>
__device__ __forceinline__ void bwd_store4(float* o, const v2f (&v)[NH]) {
#pragma unroll
    for (int q = 0; q < NH / 2; ++q) *reinterpret_cast<float4*>(o + 4 * q) = pack4(v[2 * q], v[2 * q + 1]);
}

__device__ __forceinline__ float softplus_grad(float ddt, float xraw) {     // d softplus = sigmoid; 1 above the threshold
    return xraw > 20.0f ? ddt : ddt / (1.0f + __expf(-xraw));
}

// the block's P, H (forward carry) and, at the mirrored index, P, G (adjoint carry)
template <int NH, class Args>
__device__ __forceinline__ void bwd_store_block_summaries(const Args& p, long long chains, long long row, const v2f (&pf)[NH],
                                                          const v2f (&h)[NH], const v2f (&gl)[NH]) {
    const long long f = (long long)blockIdx.x * chains + row, m = (long long)(p.nblocks - 1 - (int)blockIdx.x) * chains + row;
#pragma unroll
    for (int q = 0; q < NH / 2; ++q) {
        const float4 P4 = pack4(pf[2 * q], pf[2 * q + 1]);
        *reinterpret_cast<float4*>(p.wsP + f + 4 * q) = P4;
        *reinterpret_cast<float4*>(p.wsPr + m + 4 * q) = P4;
        *reinterpret_cast<float4*>(p.wsH + f + 4 * q) = pack4(h[2 * q], h[2 * q + 1]);
        *reinterpret_cast<float4*>(p.wsG + m + 4 * q) = pack4(gl[2 * q], gl[2 * q + 1]);
    }
}

}  // namespace wm
