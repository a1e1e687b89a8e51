// host_common.h - what the library's translation units (csrc/*.hip) share on the host side.  No kernels here: a kernel is
// defined (or instantiated) in exactly one unit.  Process-wide state is DEFINED in common.hip and declared here; everything
// that crosses units has hidden visibility, so the library's dynamic symbols stay the wm_* entry points and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <array>
#include <atomic>
#include <list>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/wavemamba_hip.h"

#define WM_HIDDEN __attribute__((visibility("hidden")))

namespace wm {

// ------------------------------------------------------------------------------------------------
// profiling hooks: HIP events on the launch stream around each kernel class
// ------------------------------------------------------------------------------------------------
struct Prof {
    std::mutex mu;
    unsigned mask = 0;                                          // bit k: record kernel class k
    std::vector<hipEvent_t> pool;                               // recycled events
    std::vector<std::pair<hipEvent_t, hipEvent_t>> rec[WM_PROF_NKERNELS];
    hipEvent_t get() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e; hipEventCreate(&e); return e;
    }
};
WM_HIDDEN extern Prof g_prof;                                   // one per process (common.hip): wm_prof_collect sees every unit's launches

struct ProfScope {
    int id; hipStream_t s; hipEvent_t e0 = nullptr, e1 = nullptr; bool active;
    ProfScope(int id_, hipStream_t s_) : id(id_), s(s_), active((g_prof.mask >> id_) & 1u) {
        if (!active) return;
        std::lock_guard<std::mutex> lk(g_prof.mu);
        e0 = g_prof.get(); e1 = g_prof.get();
        hipEventRecord(e0, s);
    }
    ~ProfScope() {
        if (!active) return;
        hipEventRecord(e1, s);
        std::lock_guard<std::mutex> lk(g_prof.mu);
        g_prof.rec[id].emplace_back(e0, e1);
    }
};

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static inline int launch_status() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? WM_OK : (int)e;
}

// Zeroing by a kernel (zero_fill_kernel, common.hip), never hipMemsetAsync.  bytes % 4 == 0 and a 4-byte aligned pointer.
WM_HIDDEN hipError_t zero_async(void* p, size_t bytes, hipStream_t st);
// zero_async unless the buffer lies inside a registered zero arena (wm_zero_arena_register, one registry per process)
WM_HIDDEN hipError_t zero_out(void* p, size_t bytes, hipStream_t st);
// two small gradient buffers: one launch when the caller allocated them back to back
WM_HIDDEN hipError_t zero_pair(float* a, size_t na, float* b, size_t nb, hipStream_t st);

// Deterministic forms (wm_*_det): the kernels store one partial per workgroup, part[j * K + k] for workgroup slot j < nblk and value
// k < K, and det_finish (det.hip) adds the nblk partials of every k in an order that depends on (nblk, K) alone and OVERWRITES the
// outputs.  Where value k goes:
//   kDetSplit   k < a -> o0[k], else o1[k - a] (o1 may be NULL)                                  (dweight | dbias, sums, a scalar)
//   kDetDw      k = 10 c + i: i < 9 -> o0[9 c + i], i == 9 -> o1[c] (o1 may be NULL)             (depth-wise dW | db)
//   kDetScan    k = a d + t (a = record length): t < b -> o0[b d + t], t == c -> o1[d], t == c + 1 -> o2[d] (o1, o2 may be NULL)
enum { kDetSplit = 0, kDetDw = 1, kDetScan = 2 };
struct DetOut { float *o0, *o1, *o2; int mode, a, b, c; };
WM_HIDDEN int det_finish(const float* part, long long nblk, long long K, const DetOut& out, hipStream_t st);

// > 64 KB of dynamic LDS is an opt-in per kernel function AND per device: one flag per (instantiation, device).
// `flags` is the caller's function-local static array; returns WM_OK or WM_EHIP.
WM_HIDDEN int lds_optin(const void* fn, int bytes, bool (&flags)[64]);
// compute units of the current device (asked once per device); returns WM_OK or WM_EHIP
WM_HIDDEN int device_cus(int* ncu);

// Launch geometry of the row-walking kernels (row_walk.hip.h): strips of `cols` output columns x bands of `rows` output rows, a walk
// per (batch, band, strip), `wpw` walks per workgroup; xcd_runs: the kernel deals its workgroups to the 8 XCDs in contiguous runs
// (row_walk), so the grid is rounded up to a multiple of 8.
struct RowWalkGeom { int nstrips, nbands, rows; long long nwalks, nblocks; };
static inline RowWalkGeom row_walk_geom(int B, int H, int W, int cols, int rows, int wpw, bool xcd_runs) {
    RowWalkGeom g;
    g.nstrips = (W + cols - 1) / cols; g.nbands = (H + rows - 1) / rows; g.rows = rows;
    g.nwalks = (long long)B * g.nbands * g.nstrips;
    g.nblocks = (g.nwalks + wpw - 1) / wpw;
    if (xcd_runs) g.nblocks = (g.nblocks + 7) / 8 * 8;
    return g;
}
// Rows per band of a kernel that RECOMPUTES its halo at two waves per SIMD: the chip holds 512 workgroups at a time and a launch
// lasts about rounds x (rows + 2 recomputed + one of prologue) - of lo, lo + step, .. <= hi the first with the smallest product.
static inline int row_walk_band_rows(int B, int H, int W, int cols, int wpw, int lo, int hi, int step) {
    int rows = lo;
    long long best = -1;
    for (int cand = lo; cand <= hi; cand += step) {
        const long long cost = ((row_walk_geom(B, H, W, cols, cand, wpw, false).nblocks + 511) / 512) * (cand + 3);
        if (best < 0 || cost < best) { best = cost; rows = cand; }
    }
    return rows;
}

}  // namespace wm

// Plane-dtype dispatch: runs CALL once with TP = float (plane_dtype == WM_F32) or TP = bf16_t (otherwise; callers have checked
// plane_dtype beforehand).  bf16_t comes with the kernel headers of the units that use this.
#define WM_PLANE_DISPATCH(plane_dtype, CALL)                          \
    do {                                                              \
        if ((plane_dtype) == WM_F32) { using TP = float; CALL; }      \
        else { using TP = bf16_t; CALL; }                             \
    } while (0)
