// common.hip - process-wide state of the library (profiling hooks, zero arenas, the zero-fill kernel) and the
// entry points that belong to no kernel family.
#include "host_common.h"

// Zero-initialised accumulator outputs (parameter gradients that kernels add into with atomics, the two running maxima of
// wm_conv2d_f16_steps).  A caller that hands out such buffers from memory it has ALREADY zeroed registers that memory
// (wm_zero_arena_register): a buffer that lies inside a registered range is taken as zero and the memset node is skipped - a
// BASELINE config-3 training step issued 323 memsets of a few hundred bytes, 4.2 us of stream time each (round 5).
struct ZeroArenas {
    std::mutex mu;
    std::atomic<int> count{0};
    std::vector<std::pair<uintptr_t, uintptr_t>> ranges;            // [begin, end)
};
static ZeroArenas g_zero_arenas;

namespace wm {

Prof g_prof;                                                    // every unit's ProfScope records into this one

// ------------------------------------------------------------------------------------------------
// Zeroing of accumulate-into outputs: a KERNEL, never hipMemsetAsync.  Round 6: a hipMemsetAsync captured into a HIP graph
// (torch.cuda.graph around a training step, trainer.GraphedTrainStep) becomes a memset node whose fill pattern this runtime
// (ROCm 7.0.2 as bundled with torch 2.10) re-reads at every launch of the graph from memory it has meanwhile recycled: with any
// eager kernel launch between two replays the node filled the gradient buffers with 16-byte records of somebody else's kernel
// arguments (tools/repro_graph_memset_node.py: every fourth float of a depth-wise weight gradient = the low half of a temporary's
// address, -1.5e38) - NaN parameters two replays later.  A kernel node carries its arguments by value.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void zero_fill_kernel(uint32_t* __restrict__ p, size_t nwords, int vec) {
    const size_t stride = (size_t)gridDim.x * 256;
    if (vec) {                                                   // 16-byte aligned, nwords % 4 == 0
        uint4* q = reinterpret_cast<uint4*>(p);
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nwords / 4; i += stride) q[i] = make_uint4(0u, 0u, 0u, 0u);
    } else {
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nwords; i += stride) p[i] = 0u;
    }
}

// bytes % 4 == 0 and a 4-byte aligned pointer (every caller zeroes float buffers)
hipError_t zero_async(void* p, size_t bytes, hipStream_t st) {
    if (bytes == 0) return hipSuccess;
    if ((bytes & 3u) || (reinterpret_cast<uintptr_t>(p) & 3u)) return hipErrorInvalidValue;
    const size_t nwords = bytes / 4;
    const int vec = aligned16(p) && (nwords % 4 == 0) ? 1 : 0;
    const size_t items = vec ? nwords / 4 : nwords;
    size_t blocks = (items + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(zero_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<uint32_t*>(p), nwords, vec);
    return hipGetLastError();
}

static bool prezeroed(const void* p, size_t bytes) {
    if (g_zero_arenas.count.load(std::memory_order_acquire) == 0) return false;
    const uintptr_t b = reinterpret_cast<uintptr_t>(p), e = b + bytes;
    std::lock_guard<std::mutex> lk(g_zero_arenas.mu);
    for (const auto& r : g_zero_arenas.ranges)
        if (b >= r.first && e <= r.second) return true;
    return false;
}

hipError_t zero_out(void* p, size_t bytes, hipStream_t st) {
    if (bytes == 0 || prezeroed(p, bytes)) return hipSuccess;
    return zero_async(p, bytes, st);
}

// Zero two small gradient buffers: ONE memset node when the caller allocated them back to back (ops.py does: a training step
// issued 440 memsets of a few hundred bytes, ~4 us of GPU time each).
hipError_t zero_pair(float* a, size_t na, float* b, size_t nb, hipStream_t st) {
    if (b && b == a + na) return zero_out(a, (na + nb) * sizeof(float), st);
    hipError_t e = zero_out(a, na * sizeof(float), st);
    if (e == hipSuccess && b) e = zero_out(b, nb * sizeof(float), st);
    return e;
}

int lds_optin(const void* fn, int bytes, bool (&flags)[64]) {
    static std::mutex mu;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return WM_EHIP;
    std::lock_guard<std::mutex> lk(mu);
    if (!flags[dev]) {
        if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return WM_EHIP;
        flags[dev] = true;
    }
    return WM_OK;
}

int device_cus(int* ncu) {
    static std::atomic<int> cached[64];                          // 0: not asked yet (two threads may both ask: same answer)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return WM_EHIP;
    int n = cached[dev].load(std::memory_order_relaxed);
    if (n == 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return WM_EHIP;
        cached[dev].store(n, std::memory_order_relaxed);
    }
    *ncu = n;
    return WM_OK;
}

}  // namespace wm

using namespace wm;

extern "C" {

int wm_abi_version(void) { return 34; }

#ifndef WM_BUILD_ID
#define WM_BUILD_ID "unknown"
#endif
const char* wm_build_id(void) { return WM_BUILD_ID; }

const char* wm_strerror(int code) {
    switch (code) {
        case WM_OK: return "ok";
        case WM_EINVAL: return "invalid shape or size argument";
        case WM_ENULL: return "required pointer is NULL";
        case WM_EALIGN: return "pointer not aligned to its element size";
        case WM_EWORKSPACE: return "workspace too small";
        case WM_EUNSUPPORTED: return "argument combination not supported";
        case WM_EHIP: return "a HIP runtime call made on behalf of the launch failed";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
    }
}

int wm_zero_arena_register(void* base, size_t bytes) {
    if (!base) return WM_ENULL;
    if (bytes == 0) return WM_EINVAL;
    const uintptr_t b = reinterpret_cast<uintptr_t>(base);
    std::lock_guard<std::mutex> lk(g_zero_arenas.mu);
    for (const auto& r : g_zero_arenas.ranges)
        if (b < r.second && b + bytes > r.first) return WM_EINVAL;  // overlaps a registered range
    g_zero_arenas.ranges.emplace_back(b, b + bytes);
    g_zero_arenas.count.store((int)g_zero_arenas.ranges.size(), std::memory_order_release);
    return WM_OK;
}

int wm_zero_arena_unregister(void* base) {
    const uintptr_t b = reinterpret_cast<uintptr_t>(base);
    std::lock_guard<std::mutex> lk(g_zero_arenas.mu);
    for (size_t i = 0; i < g_zero_arenas.ranges.size(); ++i)
        if (g_zero_arenas.ranges[i].first == b) {
            g_zero_arenas.ranges.erase(g_zero_arenas.ranges.begin() + (long)i);
            g_zero_arenas.count.store((int)g_zero_arenas.ranges.size(), std::memory_order_release);
            return WM_OK;
        }
    return WM_EINVAL;
}

void wm_prof_enable(unsigned mask) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    g_prof.mask = mask;
    if (mask)
        for (auto& v : g_prof.rec) {
            for (auto& pr : v) { g_prof.pool.push_back(pr.first); g_prof.pool.push_back(pr.second); }
            v.clear();
        }
}

int wm_prof_collect(int* launches, double* total_ms) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    for (int k = 0; k < WM_PROF_NKERNELS; ++k) {
        double tot = 0.0;
        for (auto& pr : g_prof.rec[k]) {
            hipError_t e = hipEventSynchronize(pr.second);
            if (e != hipSuccess) return (int)e;
            float ms = 0.f;
            e = hipEventElapsedTime(&ms, pr.first, pr.second);
            if (e != hipSuccess) return (int)e;
            tot += ms;
        }
        launches[k] = (int)g_prof.rec[k].size();
        total_ms[k] = tot;
    }
    return WM_OK;
}

int wm_event_synchronize_relaxed(void* event) {
    if (!event) return WM_EINVAL;
    hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
    if (hipThreadExchangeStreamCaptureMode(&mode) != hipSuccess) return WM_EHIP;
    const hipError_t e = hipEventSynchronize(static_cast<hipEvent_t>(event));
    hipThreadExchangeStreamCaptureMode(&mode);
    return e == hipSuccess ? WM_OK : WM_EHIP;
}

}  // extern "C"
