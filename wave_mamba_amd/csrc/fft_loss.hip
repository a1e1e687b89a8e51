// fft_loss.hip - the FFT training loss (FFTLoss, basicsr/losses/losses.py:300-313): launch code and C ABI (kernels:
// fft_loss.hip.h).  Forward is three launches (rows, columns, finish), backward two (columns, rows); nothing else goes on the stream:
// no memset, no atomics, no allocation, no host read - the workspace and the record are the caller's and are overwritten, so the
// pair can be captured into a HIP graph.
#include "host_common.h"
#include "fft_loss.hip.h"

using namespace wm;

namespace {

// a launch holds fewer than 2^32 threads: 2^24 - 1 workgroups of 256
const long long FL_MAX_TILES = (1LL << 24) - 1;

int fl_log2(int n) {                                       // log2 of a power of two in [FL_MIN, FL_MAX], -1 otherwise
    if (n < FL_MIN || n > FL_MAX || (n & (n - 1))) return -1;
    int l = 0;
    while ((1 << l) < n) ++l;
    return l;
}

struct FlPlan {
    FlGeom g;
    long long row_tiles, col_tiles, bins;                  // bins = planes H K
    size_t part_bytes;                                     // the column tiles' slots, padded to 16 bytes
};

// WM_EINVAL for no planes, WM_EUNSUPPORTED for a size that has no kernel or a grid that does not fit
int fl_plan(int64_t planes, int H, int W, FlPlan& p) {
    if (planes < 1) return WM_EINVAL;
    const int lH = fl_log2(H), lW = fl_log2(W);
    if (lH < 0 || lW < 0) return WM_EUNSUPPORTED;
    if (planes > FL_MAX_TILES) return WM_EUNSUPPORTED;      // (keeps the products below in 64 bits)
    FlGeom& g = p.g;
    g.H = H; g.W = W; g.K = W / 2 + 1; g.lH = lH; g.lW = lW;
    g.npairs = (long long)planes * (H / 2);
    g.ncols = (long long)planes * g.K;
    const int nbr = FL_TILE / W, nbc = FL_TILE / H;
    p.row_tiles = (g.npairs + nbr - 1) / nbr;
    p.col_tiles = (g.ncols + nbc - 1) / nbc;
    if (p.row_tiles > FL_MAX_TILES || p.col_tiles > FL_MAX_TILES) return WM_EUNSUPPORTED;
    p.bins = (long long)planes * H * g.K;
    p.part_bytes = ((size_t)p.col_tiles * sizeof(double) + 15) & ~(size_t)15;
    return WM_OK;
}

}  // namespace

extern "C" {

int wm_fft_l1_supported(int H, int W) { return fl_log2(H) >= 0 && fl_log2(W) >= 0 ? 1 : 0; }

size_t wm_fft_l1_record_bytes(int64_t planes, int H, int W) {
    FlPlan p;
    return fl_plan(planes, H, W, p) == WM_OK ? (size_t)p.bins : 0;
}

size_t wm_fft_l1_workspace_bytes(int64_t planes, int H, int W) {
    FlPlan p;
    return fl_plan(planes, H, W, p) == WM_OK ? p.part_bytes + (size_t)p.bins * sizeof(FlC) : 0;
}

int wm_fft_l1_mean_fwd(const float* a, const float* b, float* out, void* record, void* workspace, size_t workspace_bytes,
                       int64_t planes, int H, int W, void* stream) {
    FlPlan p;
    const int rc = fl_plan(planes, H, W, p);
    if (rc) return rc;
    if (!a || !b || !out || !workspace) return WM_ENULL;
    if (!aligned16(a) || !aligned16(b) || !aligned16(workspace)) return WM_EALIGN;
    if (workspace_bytes < wm_fft_l1_workspace_bytes(planes, H, W)) return WM_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)workspace;
    FlC* mid = (FlC*)((char*)workspace + p.part_bytes);
    hipLaunchKernelGGL(fft_l1_rows_fwd_kernel, dim3((unsigned)p.row_tiles), dim3(FL_THREADS), 0, st, a, b, mid, p.g);
    int rc2 = launch_status();
    if (rc2) return rc2;
    hipLaunchKernelGGL(fft_l1_cols_fwd_kernel, dim3((unsigned)p.col_tiles), dim3(FL_THREADS), 0, st, (const FlC*)mid,
                       (unsigned char*)record, part, p.g);
    rc2 = launch_status();
    if (rc2) return rc2;
    hipLaunchKernelGGL(fft_l1_finish_kernel, dim3(1), dim3(FL_THREADS), 0, st, (const double*)part, p.col_tiles, 2.0 * (double)p.bins,
                       out);
    return launch_status();
}

int wm_fft_l1_mean_bwd(const void* record, const float* gout, float* ga, float* gb, void* workspace, size_t workspace_bytes,
                       int64_t planes, int H, int W, void* stream) {
    FlPlan p;
    const int rc = fl_plan(planes, H, W, p);
    if (rc) return rc;
    if (!record || !gout || !workspace || (!ga && !gb)) return WM_ENULL;
    if (!aligned16(ga) || !aligned16(gb) || !aligned16(workspace)) return WM_EALIGN;
    if (workspace_bytes < wm_fft_l1_workspace_bytes(planes, H, W)) return WM_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    FlC* mid = (FlC*)((char*)workspace + p.part_bytes);
    hipLaunchKernelGGL(fft_l1_cols_bwd_kernel, dim3((unsigned)p.col_tiles), dim3(FL_THREADS), 0, st, (const unsigned char*)record, mid,
                       p.g);
    const int rc2 = launch_status();
    if (rc2) return rc2;
    hipLaunchKernelGGL(fft_l1_rows_bwd_kernel, dim3((unsigned)p.row_tiles), dim3(FL_THREADS), 0, st, (const FlC*)mid, gout, ga, gb, p.g,
                       0.5 / (2.0 * (double)p.bins));
    return launch_status();
}

}  // extern "C"
