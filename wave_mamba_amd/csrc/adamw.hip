// adamw.hip - the table-driven AdamW step with the weights' moving average: launch code and C ABI (kernels: adamw.hip.h).  Two
// launches, nothing else on the stream: the update, then the counter's increment - no atomics, no memset node, so a call captured
// into a HIP graph replays as it ran.
#include "host_common.h"
#include "adamw.hip.h"

using namespace wm;

extern "C" {

int wm_adamw_step(const void* table, int64_t n_rows, const float* lr, float* step, const double* hyper, const float* found_inf,
                  const float* grad_scale, void* stream) {
    static_assert(sizeof(long long) == sizeof(int64_t), "the table's fields are read as long long");
    if (n_rows < 0) return WM_EINVAL;
    if (n_rows == 0) return WM_OK;
    if (!table || !hyper || !lr || !step) return WM_ENULL;
    if (n_rows > 0x7fffffffLL) return WM_EUNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(table) & 7u) return WM_EALIGN;
    if ((reinterpret_cast<uintptr_t>(lr) | reinterpret_cast<uintptr_t>(step) | reinterpret_cast<uintptr_t>(found_inf) |
         reinterpret_cast<uintptr_t>(grad_scale)) & 3u) return WM_EALIGN;
    const AdamwHyper h{hyper[0], hyper[1], hyper[2], hyper[3], hyper[4]};       // HOST memory, read here: launch scalars of the run
    if (!(h.beta1 >= 0.0 && h.beta1 < 1.0 && h.beta2 >= 0.0 && h.beta2 < 1.0 && h.eps >= 0.0 && h.weight_decay >= 0.0 &&
          h.ema_decay >= 0.0 && h.ema_decay < 1.0)) return WM_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(adamw_step_kernel, dim3((unsigned)n_rows), dim3(256), 0, st, reinterpret_cast<const long long*>(table), lr,
                       (const float*)step, h, found_inf, grad_scale);
    const int rc = launch_status();
    if (rc != WM_OK) return rc;
    hipLaunchKernelGGL(adamw_count_kernel, dim3(1), dim3(64), 0, st, step, found_inf);
    return launch_status();
}

}  // extern "C"
