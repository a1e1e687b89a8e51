// det.hip - the deterministic training mode's shared pieces: the fixed-order finish of the wm_*_det entry points (every unit's
// _det launcher calls det_finish) and the C ABI of the channel gather.
#include "host_common.h"
#include "det.hip.h"

namespace wm {

int det_finish(const float* part, long long nblk, long long K, const DetOut& out, hipStream_t st) {
    if (K <= 0) return WM_OK;
    // lanes per value: small records get up to a wave per value (a scalar loss of 1024 partials is not one thread's chain of 1024
    // loads), wide ones (a 128 x 32 linear weight gradient) one coalesced thread per value; never more lanes than partials
    int S = 64;
    while (S > 1 && (K * S > 16384 || S > 2 * nblk)) S >>= 1;
    const long long threads = K * S;
    ProfScope ps(19, st);
    hipLaunchKernelGGL(det_finish_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, part, nblk, K, S, out);
    return launch_status();
}

static unsigned gather_blocks(long long HW, bool vec) {
    long long bx = ((vec ? HW / 4 : HW) + 1023) / 1024;          // ~4 accesses per thread
    return (unsigned)(bx < 1 ? 1 : (bx > 64 ? 64 : bx));
}

}  // namespace wm

using namespace wm;

extern "C" {

int wm_channel_gather_fwd(const float* x, const int* index, float* y, int B, int C, int M, int64_t HW, void* stream) {
    if (B < 0 || C < 0 || M < 0 || HW < 0) return WM_EINVAL;
    if (B == 0 || M == 0 || HW == 0) return WM_OK;
    if (C == 0) return WM_EINVAL;
    if (!x || !index || !y) return WM_ENULL;
    if (B > 65535 || M > 65535) return WM_EUNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(index)) & 3u) return WM_EALIGN;
    const bool vec = HW % 4 == 0 && aligned16(x) && aligned16(y);
    const dim3 grid(gather_blocks(HW, vec), (unsigned)M, (unsigned)B);
    if (vec) hipLaunchKernelGGL(channel_gather_fwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, index, y, C, M, (long long)HW);
    else hipLaunchKernelGGL(channel_gather_fwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, index, y, C, M, (long long)HW);
    return launch_status();
}

int wm_channel_gather_bwd(const float* gy, const int* index, float* gx, int B, int C, int M, int64_t HW, void* stream) {
    if (B < 0 || C < 0 || M < 0 || HW < 0) return WM_EINVAL;
    if (B == 0 || C == 0 || HW == 0) return WM_OK;
    if (!gx || (M > 0 && (!gy || !index))) return WM_ENULL;
    if (B > 65535 || C > 65535 || M > kGatherMaxM) return WM_EUNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(gx) | reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(index)) & 3u) return WM_EALIGN;
    const bool vec = HW % 4 == 0 && aligned16(gy) && aligned16(gx);
    const dim3 grid(gather_blocks(HW, vec), (unsigned)C, (unsigned)B);
    if (vec) hipLaunchKernelGGL(channel_gather_bwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, gy, index, gx, C, M, (long long)HW);
    else hipLaunchKernelGGL(channel_gather_bwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, gy, index, gx, C, M, (long long)HW);
    return launch_status();
}

}  // extern "C"
