// det.hip.h - what the deterministic training mode adds that belongs to no kernel family, for gfx950:
//   det_finish_kernel          the fixed-order sum of the per-workgroup partials every wm_*_det entry point leaves in its workspace
//                              (the scheme of conv_wgrad_finish_kernel, skff_weights_kernel and gram_reduce_kernel, for any record)
//   channel_gather_fwd_kernel  y[b, j, :] = x[b, idx[b, j], :] - torch.gather over the channel axis with one index per (b, j)
//   channel_gather_bwd_kernel  gx[b, c, :] = sum_j [idx[b, j] == c] gy[b, j, :] in ascending j - its gradient, without atomics
// Reference: the two gathers of the HFE branch, /root/reference/basicsr/archs/wavemamba_arch.py:666 (Matching) and :713 (PAConv's
// cat([x, matched])); their backward is ATen's scatter-add there (atomic adds: the order of two sources of one channel is not fixed).
#pragma once
#include <hip/hip_runtime.h>

namespace wm {

// out[k] = sum_{j < nblk} part[j K + k].  S (a power of two <= 64) adjacent lanes share a value k: lane `seg` adds the partials
// j = seg, seg + S, ... in ascending j, then the S lane sums meet in a butterfly - an order fixed by (nblk, S) alone.
// grid (ceil(K S / 256)), block (256)
__global__ __launch_bounds__(256) void det_finish_kernel(const float* __restrict__ part, long long nblk, long long K, int S,
                                                         DetOut o) {
    const long long gt = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long k = gt / S;
    const int seg = (int)(gt % S);
    float acc = 0.0f;
    if (k < K)
        for (long long j = seg; j < nblk; j += S) acc += part[j * K + k];
    for (int off = S >> 1; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    if (k >= K || seg != 0) return;
    if (o.mode == kDetSplit) {
        if (k < o.a) o.o0[k] = acc;
        else if (o.o1) o.o1[k - o.a] = acc;
    } else if (o.mode == kDetDw) {
        const long long c = k / 10;
        const int i = (int)(k % 10);
        if (i < 9) o.o0[c * 9 + i] = acc;
        else if (o.o1) o.o1[c] = acc;
    } else {
        const long long d = k / o.a;
        const int t = (int)(k % o.a);
        if (t < o.b) o.o0[d * o.b + t] = acc;
        else if (t == o.c && o.o1) o.o1[d] = acc;
        else if (t == o.c + 1 && o.o2) o.o2[d] = acc;
    }
}

constexpr int kGatherMaxM = 1024;          // gathered channels per batch element (the list of one destination's sources lives in LDS)

// y[b, j, :] = x[b, idx[b, j], :]; an index outside [0, C) yields zeros.  grid (blocks per plane, M, B), block (256)
template <bool VEC>
__global__ __launch_bounds__(256) void channel_gather_fwd_kernel(const float* __restrict__ x, const int* __restrict__ idx,
                                                                 float* __restrict__ y, int C, int M, long long HW) {
    const int j = blockIdx.y, b = blockIdx.z;
    const int c = idx[(long long)b * M + j];
    const bool ok = c >= 0 && c < C;
    const float* src = x + ((long long)b * C + (ok ? c : 0)) * HW;
    float* dst = y + ((long long)b * M + j) * HW;
    const long long stride = (long long)gridDim.x * 256;
    if constexpr (VEC) {
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < HW / 4; i += stride) {
            const float4 v = reinterpret_cast<const float4*>(src)[i];
            reinterpret_cast<float4*>(dst)[i] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    } else {
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < HW; i += stride) dst[i] = ok ? src[i] : 0.0f;
    }
}

// gx[b, c, :] = the sum of the planes gy[b, j, :] with idx[b, j] == c, added in ascending j (a destination nobody names is zero).
// One workgroup per (plane segment, c, b): its first wave lists the sources of c in ascending j (ballot + prefix count), then
// every thread adds that list's planes for its elements - each plane of gy is read by exactly one destination, so gy is read
// once and gx written once.  Four sources are fetched ahead of their adds.  grid (blocks per plane, C, B), block (256)
template <bool VEC>
__global__ __launch_bounds__(256) void channel_gather_bwd_kernel(const float* __restrict__ gy, const int* __restrict__ idx,
                                                                 float* __restrict__ gx, int C, int M, long long HW) {
    __shared__ int s_list[kGatherMaxM];
    __shared__ int s_n;
    const int c = blockIdx.y, b = blockIdx.z;
    if (threadIdx.x < 64) {
        int n = 0;
        for (int base = 0; base < M; base += 64) {
            const int j = base + (int)threadIdx.x;
            const bool hit = j < M && idx[(long long)b * M + j] == c;
            const unsigned long long m = __ballot(hit);
            if (hit) s_list[n + __popcll(m & ((1ull << threadIdx.x) - 1ull))] = j;
            n += __popcll(m);
        }
        if (threadIdx.x == 0) s_n = n;
    }
    __syncthreads();
    const int n = s_n;
    const float* gb = gy + (long long)b * M * HW;
    float* dst = gx + ((long long)b * C + c) * HW;
    const long long stride = (long long)gridDim.x * 256;
    if constexpr (VEC) {
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < HW / 4; i += stride) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            int q = 0;
            for (; q + 4 <= n; q += 4) {
                float4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = reinterpret_cast<const float4*>(gb + (long long)s_list[q + u] * HW)[i];
#pragma unroll
                for (int u = 0; u < 4; ++u) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
            }
            for (; q < n; ++q) {
                const float4 v = reinterpret_cast<const float4*>(gb + (long long)s_list[q] * HW)[i];
                acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
            }
            reinterpret_cast<float4*>(dst)[i] = acc;
        }
    } else {
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < HW; i += stride) {
            float acc = 0.0f;
            for (int q = 0; q < n; ++q) acc += gb[(long long)s_list[q] * HW + i];
            dst[i] = acc;
        }
    }
}

}  // namespace wm
