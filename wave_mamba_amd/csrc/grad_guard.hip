// grad_guard.hip - the guarded optimizer step: launch code and C ABI of the gradient norm / non-finite flag / clipping divisor
// (kernels: grad_guard.hip.h).  Two launches, nothing else on the stream: the workspace and the record are overwritten, so a call
// captured into a HIP graph holds no memset node and no accumulator state.
#include "host_common.h"
#include "grad_guard.hip.h"

using namespace wm;

extern "C" {

size_t wm_grad_guard_workspace_bytes(int64_t n_rows) { return n_rows > 0 ? (size_t)n_rows * sizeof(GuardPart) : 0; }

int wm_grad_guard(const void* table, int64_t n_rows, float max_norm, float* record, int64_t* skipped, void* ws, size_t ws_bytes,
                  void* stream) {
    static_assert(sizeof(long long) == sizeof(int64_t), "the table's fields and the counter are read as long long");
    if (n_rows < 0) return WM_EINVAL;
    if (!record) return WM_ENULL;
    if (n_rows > 0) {
        if (!table || !ws) return WM_ENULL;
        if (ws_bytes < wm_grad_guard_workspace_bytes(n_rows)) return WM_EWORKSPACE;
        if (n_rows > 0x7fffffffLL) return WM_EUNSUPPORTED;
        if ((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(ws)) & 7u) return WM_EALIGN;
    }
    if ((reinterpret_cast<uintptr_t>(record) & 3u) || (reinterpret_cast<uintptr_t>(skipped) & 7u)) return WM_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    GuardPart* part = (GuardPart*)ws;
    if (n_rows > 0) {
        hipLaunchKernelGGL(grad_guard_partial_kernel, dim3((unsigned)n_rows), dim3(256), 0, st,
                           reinterpret_cast<const long long*>(table), part);
        const int rc = launch_status();
        if (rc != WM_OK) return rc;
    }
    hipLaunchKernelGGL(grad_guard_finish_kernel, dim3(1), dim3(256), 0, st, part, (long long)n_rows, max_norm, record,
                       reinterpret_cast<long long*>(skipped));
    return launch_status();
}

}  // extern "C"
