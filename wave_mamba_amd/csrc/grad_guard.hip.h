// grad_guard.hip.h - the guarded optimizer step's device side, for gfx950: the global L2 norm of a list of fp32 gradient runs, a
// non-finite flag and the clipping divisor, left in device memory for the optimizer launch that follows in the same stream (or the
// same captured graph).  No host read, no atomics, no memset: bit-identical run to run.
//   grad_guard_partial_kernel   one workgroup per table row {address, count}: sum of squares in double + "a non-finite value" flag
//   grad_guard_finish_kernel    one workgroup: the rows' partials in a fixed order -> {norm, found_inf, grad_scale, 0}, skipped += found_inf
// Reference: none in the reference's training loop (femasr_model.py:157-185 steps unconditionally); the clipping coefficient is
// torch.nn.utils.clip_grad_norm_'s, inverted (the fused AdamW DIVIDES by grad_scale), the skip is torch.amp.GradScaler's found_inf.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wm {

constexpr int kGuardChunk = 4096;          // the host's row length (ops.GRAD_GUARD_CHUNK): 4 x 16 bytes per lane; the kernel takes any count

struct GuardPart { double sum; unsigned flag; unsigned pad; };           // one row's result (16 bytes)

__device__ __forceinline__ void guard_take(float x, double& acc, unsigned& bad) {
    // the bit pattern, not isfinite(): no floating-point setting of a build can fold an integer compare
    bad |= (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u ? 1u : 0u;
    const double d = (double)x;                                          // fp32 x fp32 is exact in double: 1e19 and 1e-30 both survive
    acc += d * d;
}

// The wave's 64 lanes in a butterfly, the workgroup's four waves as (0 + 1) + (2 + 3): an order fixed by the launch shape alone.
// Valid in thread 0.
__device__ __forceinline__ void guard_block_reduce(double& acc, unsigned& bad) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        acc += __shfl_xor(acc, off);
        bad |= __shfl_xor(bad, off);
    }
    __shared__ double s_acc[4];
    __shared__ unsigned s_bad[4];
    if ((threadIdx.x & 63) == 0) { s_acc[threadIdx.x >> 6] = acc; s_bad[threadIdx.x >> 6] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        acc = (s_acc[0] + s_acc[1]) + (s_acc[2] + s_acc[3]);
        bad = (s_bad[0] | s_bad[1]) | (s_bad[2] | s_bad[3]);
    }
}

// table[2 r] = the address of row r's first float (any 4-byte boundary: views into a flat buffer), table[2 r + 1] = its count (>= 0).
// Lanes below `head` take the floats in front of the first 16-byte boundary, then 16-byte loads over the aligned body, then lanes
// below `tail` the rest.  grid (n_rows), block (256)
__global__ __launch_bounds__(256) void grad_guard_partial_kernel(const long long* __restrict__ table, GuardPart* __restrict__ part) {
    const long long row = blockIdx.x;
    const unsigned long long addr = (unsigned long long)table[2 * row];
    const long long n = table[2 * row + 1];
    const float* p = reinterpret_cast<const float*>(addr);
    const int tid = (int)threadIdx.x;
    double acc = 0.0;
    unsigned bad = 0u;
    if (n > 0) {
        long long head = (long long)(((16u - (unsigned)(addr & 15u)) & 15u) >> 2);
        if (head > n) head = n;
        const long long body = (n - head) >> 2;
        const long long tail = n - head - 4 * body;
        if (tid < head) guard_take(p[tid], acc, bad);
        const float4* p4 = reinterpret_cast<const float4*>(p + head);
        for (long long i = tid; i < body; i += 256) {
            const float4 v = p4[i];
            guard_take(v.x, acc, bad); guard_take(v.y, acc, bad); guard_take(v.z, acc, bad); guard_take(v.w, acc, bad);
        }
        if (tid < tail) guard_take(p[head + 4 * body + tid], acc, bad);
    }
    guard_block_reduce(acc, bad);
    if (tid == 0) part[row] = GuardPart{acc, bad, 0u};
}

// Lane t adds the rows t, t + 256, ... in ascending order, then guard_block_reduce.  Reads only part[0 .. n_rows) and overwrites the
// record: nothing depends on what the workspace or the record held before.  n_rows == 0 writes {0, 0, 1, 0}.
// `skipped` (may be NULL): one thread's plain read-modify-write.  grid (1), block (256)
__global__ __launch_bounds__(256) void grad_guard_finish_kernel(const GuardPart* __restrict__ part, long long n_rows, float max_norm,
                                                                float* __restrict__ record, long long* __restrict__ skipped) {
    double acc = 0.0;
    unsigned bad = 0u;
    for (long long r = threadIdx.x; r < n_rows; r += 256) {
        const GuardPart g = part[r];
        acc += g.sum;
        bad |= g.flag;
    }
    guard_block_reduce(acc, bad);
    if (threadIdx.x != 0) return;
    const float norm = (float)sqrt(acc);                                   // finite elements can still overflow fp32 here: 4096 x 3e38
    const bool norm_bad = (__float_as_uint(norm) & 0x7f800000u) == 0x7f800000u;
    const bool found = bad != 0u || norm_bad;
    float scale = 1.0f;
    const bool clip = max_norm > 0.0f && (__float_as_uint(max_norm) & 0x7f800000u) != 0x7f800000u;
    if (clip && !found) scale = fmaxf(1.0f, (norm + 1e-6f) / max_norm);
    record[0] = norm;
    record[1] = found ? 1.0f : 0.0f;
    record[2] = scale;
    record[3] = 0.0f;
    if (skipped) skipped[0] = skipped[0] + (found ? 1 : 0);
}

}  // namespace wm
