// scan_bwd.hip - C ABI over the selective scan and the fused SS2D core, backward, and the linear weight gradient.
#include "scan_common.h"
#include "selscan_bwd.hip.h"
#include "ss2d_core_bwd.hip.h"
#include "linear_wgrad.hip.h"

namespace wm {

struct BwdPlan {
    int NP, wpg, rows, nchunks, cpb, nblocks; long long chains;
    size_t blk_bytes, arr_bytes, s_bytes, seg_bytes, part_bytes, total;
    // workspace: [P | H | Pr | G] block summaries (blk_bytes each), per-chunk local states (arr_bytes), per-chunk dt sums
    // (s_bytes), carry scratch for two scans (seg_bytes), per-block parameter-gradient partials (part_bytes)
    size_t off_hl() const { return 4 * blk_bytes; }
    size_t off_s() const { return off_hl() + arr_bytes; }
    size_t off_seg() const { return off_s() + s_bytes; }
    size_t off_part() const { return off_seg() + seg_bytes; }
};
// chunks per block of the two backward kernels: enough single-wave blocks to fill the chip (the reduce kernel holds 9
// per compute unit = 2,304 at once).  The summaries the carry kernels walk are per BLOCK, so longer blocks also mean a
// shorter carry and fewer partial records.  BASELINE config 3 training step on one MI355X (tools/train_breakdown.py,
// gpurun_out r3z): at least 8192 blocks / at most 8 chunks each 101.2 ms, 4096 / 8 99.7, 2048 / 16 95.9, 1024 / 32 97.5.
#ifndef WM_BWD_CPB_MAX
#define WM_BWD_CPB_MAX 16
#endif
#ifndef WM_BWD_MIN_BLOCKS
#define WM_BWD_MIN_BLOCKS 2048
#endif
// blocks of the finish kernel per channel: a thread adds up at most ~4 records per batch item
static int bwd_finish_split(int nblocks, int npp) {
    const int stride = (256 / npp) * npp;
    const long long per = (long long)nblocks * npp;
    long long y = (per + 4LL * stride - 1) / (4LL * stride);
    return (int)(y < 1 ? 1 : (y > 64 ? 64 : y));
}
// The fused core's gradient kernel (core_bwd_chunk_kernel) is a workgroup of NP / 8 waves with 37,952 / 58,944 B of LDS and ~256
// registers per lane: FOUR (N <= 16) / TWO (N <= 32) workgroups are resident per compute unit, 1024 / 512 on the chip, and a
// workgroup pays a prologue (weights, carried states) of ~0.4 chunks before its first chunk.  Its block length is therefore chosen
// per shape: the chunks per block c in [1, 32] that minimise  ceil(workgroups(c) / resident) * (c + 0.4)  - whole dispatch rounds
// of resident workgroups - ties to the longer block (fewer summaries, shorter carry).  Round 5, BASELINE config 3 on one MI355X
// (profiles/r05/core_bwd_block_length_ab.txt): against "at least 2048 blocks, at most 16 chunks" (two rounds at every level)
// 3.93 -> 3.77 / 1.19 -> 1.04 / 0.514 -> 0.368 ms per call at levels 1 / 2 / 3, 59.0 -> 57.1 ms per training step; 512, 1536, 2048
// and 4096 blocks are all slower (1536: one and a half rounds, the worst).
static int bwd_fused_cpb(int nchunks, long long rows, int NP) {
    const long long resident = NP == 16 ? 1024 : 512;
    int best = 1;
    double best_cost = 1e300;
    for (int c = 1; c <= 32; ++c) {
        const long long wgs = (long long)((nchunks + c - 1) / c) * rows;
        const double cost = (double)((wgs + resident - 1) / resident) * (c + 0.4);
        if (cost <= best_cost) { best_cost = cost; best = c; }
    }
    return best;
}
static int bwd_plan(BwdPlan& pl, int batch, int dim, int L, int N, int G, int part_pad = kPartPad) {
    if (batch <= 0 || dim <= 0 || L <= 0 || N <= 0 || G <= 0) return WM_EINVAL;
    if (N > 32) return WM_EUNSUPPORTED;
    if (dim % G != 0) return WM_EINVAL;
    pl.NP = N <= 16 ? 16 : 32;
    pl.wpg = (dim / G + 63) / 64;
    const long long rows = (long long)batch * G * pl.wpg;
    if (rows > 65535) return WM_EUNSUPPORTED;
    pl.rows = (int)rows;
    pl.nchunks = (L + kBT - 1) / kBT;
    {
        const long long blocks1 = (long long)pl.nchunks * pl.rows;
        const int cpb = (int)(blocks1 / (long long)WM_BWD_MIN_BLOCKS);
        pl.cpb = cpb < 1 ? 1 : (cpb > WM_BWD_CPB_MAX ? WM_BWD_CPB_MAX : cpb);
        if (part_pad == kPartPadFused) pl.cpb = bwd_fused_cpb(pl.nchunks, rows, pl.NP);     // the fused core's gradient kernel
    }
    pl.nblocks = (pl.nchunks + pl.cpb - 1) / pl.cpb;
    pl.chains = (long long)batch * dim * pl.NP;
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    pl.blk_bytes = up((size_t)pl.nblocks * pl.chains * sizeof(float));
    pl.arr_bytes = up((size_t)pl.nchunks * pl.chains * sizeof(float));
    pl.s_bytes = up((size_t)pl.nchunks * batch * dim * sizeof(float));
    pl.seg_bytes = up((size_t)4 * carry_nsegs(pl.nblocks) * pl.chains * sizeof(float));
    pl.part_bytes = up((size_t)pl.nblocks * batch * dim * (pl.NP + part_pad) * sizeof(float));
    pl.total = pl.off_part() + pl.part_bytes;
    return WM_OK;
}

// forward and adjoint carry of one direction in ONE batch launch (same length, same depth)
static void bwd_launch_carry(const ScanBwdArgs& a, const BwdPlan& pl, float* seg, hipStream_t st) {
    CarryBatch cb{};
    const int nsegs = (int)carry_nsegs(pl.nblocks);
    const size_t one = (size_t)nsegs * pl.chains;
    cb.d[0] = CarryDir{a.wsP, a.wsH, seg, seg + one, pl.nblocks, nsegs};
    cb.d[1] = CarryDir{a.wsPr, a.wsG, seg + 2 * one, seg + 3 * one, pl.nblocks, nsegs};
    launch_carry_batch(cb, 2, pl.chains, st);
}
static void bwd_bind_workspace(ScanBwdArgs& a, const BwdPlan& pl, char* w, float*& seg) {
    a.wsP = (float*)w; a.wsH = (float*)(w + pl.blk_bytes); a.wsPr = (float*)(w + 2 * pl.blk_bytes);
    a.wsG = (float*)(w + 3 * pl.blk_bytes);
    a.wsHl = (float*)(w + pl.off_hl()); a.wsS = (float*)(w + pl.off_s());
    seg = (float*)(w + pl.off_seg());
    a.part = (float*)(w + pl.off_part());
    a.nchunks = pl.nchunks; a.cpb = pl.cpb; a.nblocks = pl.nblocks;
}

// det_ws: NULL, or (wm_selscan_bwd_det) the room for the finish kernel's records - dA / dD / dbias are then written by det_finish
template <int NP, bool VEC>
static int bwd_launch(const ScanBwdArgs& a0, const BwdPlan& pl, float* seg, float* dA, float* dD, float* dbias,
                      hipStream_t st, float* det_ws = nullptr) {
    ScanBwdArgs a = a0;
    const dim3 grid((unsigned)pl.nblocks, (unsigned)pl.rows), block(64);
    ProfScope ps(12, st);
    if (pl.nchunks > 1) {
        hipLaunchKernelGGL((selscan_bwd_reduce_kernel<NP, VEC>), grid, block, 0, st, a);
        if (pl.nblocks > 1) bwd_launch_carry(a, pl, seg, st);
    }
    hipLaunchKernelGGL((selscan_bwd_chunk_kernel<NP, VEC>), grid, block, 0, st, a);
    if (det_ws) {
        const int ysplit = bwd_finish_split(pl.nblocks, NP + kPartPad);
        hipLaunchKernelGGL(selscan_bwd_finish_kernel<true>, dim3((unsigned)a.dim, (unsigned)ysplit), dim3(256), 0, st,
                           (const float*)a.part, det_ws, (float*)nullptr, (float*)nullptr, a.batch, a.dim, a.N, NP + kPartPad,
                           pl.nblocks, NP);
        return det_finish(det_ws, ysplit, (long long)a.dim * (NP + kPartPad), DetOut{dA, dD, dbias, kDetScan, NP + kPartPad, a.N, NP}, st);
    }
    zero_async(dA, (size_t)a.dim * a.N * sizeof(float), st);
    if (dD) zero_async(dD, (size_t)a.dim * sizeof(float), st);
    if (dbias) zero_async(dbias, (size_t)a.dim * sizeof(float), st);
    const int ysplit = bwd_finish_split(pl.nblocks, NP + kPartPad);
    hipLaunchKernelGGL(selscan_bwd_finish_kernel<false>, dim3((unsigned)a.dim, (unsigned)ysplit), dim3(256), 0, st,
                       (const float*)a.part, dA, dD, dbias, a.batch, a.dim, a.N, NP + kPartPad, pl.nblocks, NP);
    return launch_status();
}

// ---- second generation (ss2d_core_bwd.hip.h) ---------------------------------------------------------------------------
struct CoreBwdPlan2 {
    BwdPlan scan; long long L; int NP, NWT, slices;
    size_t prep_bytes, wt_bytes, map_bytes, scan_bytes, wpart_bytes, wsum_bytes, total;
};
static int core_bwd_plan2(CoreBwdPlan2& pl, int B, int D, int H, int W, int N, int R) {
    if (B <= 0 || D <= 0 || H <= 0 || W <= 0 || N <= 0 || R <= 0) return WM_EINVAL;
    if (N > 32 || R > kRecPad || D > 64) return WM_EUNSUPPORTED;
    pl.L = (long long)H * W;
    if (pl.L > 0x7fffffffLL) return WM_EUNSUPPORTED;
    if (B > 65535) return WM_EUNSUPPORTED;
    int rc = bwd_plan(pl.scan, B, D, (int)pl.L, N, 1, kPartPadFused);
    if (rc) return rc;
    pl.NP = N <= 16 ? 16 : 32;
    pl.NWT = pl.NP == 16 ? BwdCfg<16>::NWT : BwdCfg<32>::NWT;
    const long long nb = (long long)B * pl.scan.nblocks;
    pl.slices = (int)(nb < 64 ? 1 : (nb / 32 > 64 ? 64 : nb / 32));           // >= 32 partials per slice, <= 64 slices
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    pl.prep_bytes = up((size_t)4 * (pl.NP == 16 ? CoreCfg<16>::PREP : CoreCfg<32>::PREP) * sizeof(float));
    pl.wt_bytes = up((size_t)4 * (pl.NP == 16 ? BwdCfg<16>::WT_U4 : BwdCfg<32>::WT_U4) * sizeof(uint4));
    pl.map_bytes = up((size_t)B * D * pl.L * sizeof(float));
    pl.scan_bytes = up(pl.scan.total);
    pl.wpart_bytes = up((size_t)nb * pl.NWT * 256 * sizeof(float));
    pl.wsum_bytes = up((size_t)4 * pl.slices * pl.NWT * 256 * sizeof(float));
    pl.total = pl.prep_bytes + pl.wt_bytes + 4 * pl.map_bytes + 4 * pl.scan_bytes + 4 * pl.wpart_bytes + pl.wsum_bytes;
    return WM_OK;
}

template <int NP>
static int core_bwd_v2(const CoreBwdPlan2& pl, const float* x, const float* x_proj_weight, const float* dt_projs_weight,
                       const float* dt_projs_bias, const float* A_logs, const float* Ds, const float* dy_row_fwd,
                       const float* dy_row_rev, const float* dy_col_fwd, const float* dy_col_rev, float* dx,
                       float* dx_proj_weight, float* ddt_projs_weight, float* ddt_projs_bias, float* dA_logs, float* dDs,
                       void* workspace, int B, int D, int H, int W, int N, int R, hipStream_t st) {
    using Cfg = BwdCfg<NP>;
    const long long L = pl.L;
    char* w = (char*)workspace;
    float* prep = (float*)w; w += pl.prep_bytes;
    uint4* wT = (uint4*)w; w += pl.wt_bytes;
    float* xT = (float*)w; w += pl.map_bytes;
    float* dyTa = (float*)w; w += pl.map_bytes;
    float* dyTb = (float*)w; w += pl.map_bytes;
    float* dxT = (float*)w; w += pl.map_bytes;
    char* scan_ws[4];
    for (int k = 0; k < 4; ++k) { scan_ws[k] = w; w += pl.scan_bytes; }
    float* wpart[4];
    for (int k = 0; k < 4; ++k) { wpart[k] = (float*)w; w += pl.wpart_bytes; }
    float* wsum = (float*)w;

    ProfScope ps(12, st);
    // parameters -> forward-style fragments / constants, and the transposed fragments of the dx product
    hipLaunchKernelGGL((ss2d_core_prep_kernel<NP>), dim3(4), dim3(256), 0, st, x_proj_weight, dt_projs_weight, dt_projs_bias,
                       A_logs, Ds, prep, D, N, R);
    hipLaunchKernelGGL((core_bwd_prep_kernel<NP>), dim3(4), dim3(256), 0, st, x_proj_weight, wT, D, N, R);
    {   // the column directions scan the transposed map
        const dim3 tg((unsigned)((W + 31) / 32), (unsigned)((H + 31) / 32), (unsigned)(B * D)), tb(32, 8);
        hipLaunchKernelGGL(transpose_planes_kernel, tg, tb, 0, st, x, xT, H, W, 0);
        hipLaunchKernelGGL(transpose_planes_kernel, tg, tb, 0, st, dy_col_fwd, dyTa, H, W, 0);
        if (dy_col_rev != dy_col_fwd) hipLaunchKernelGGL(transpose_planes_kernel, tg, tb, 0, st, dy_col_rev, dyTb, H, W, 0);
    }
    const float* dyT_rev = dy_col_rev != dy_col_fwd ? dyTb : dyTa;
    CoreBwdArgs a[4];
    float* seg[4];
    const int CP = R + 2 * N;
    for (int k = 0; k < 4; ++k) {
        const bool col = k & 1;
        CoreBwdArgs& q = a[k];
        q.x = col ? xT : x;
        q.dy = k == 0 ? dy_row_fwd : k == 2 ? dy_row_rev : k == 1 ? (const float*)dyTa : dyT_rev;
        q.dx = col ? dxT : dx;
        q.prep = prep + (size_t)k * CoreCfg<NP>::PREP;
        q.wT = wT + (size_t)k * Cfg::WT_U4;
        q.WxR = x_proj_weight + (size_t)k * CP * D;
        ScanBwdArgs t{};
        bwd_bind_workspace(t, pl.scan, scan_ws[k], seg[k]);
        q.wsP = t.wsP; q.wsH = t.wsH; q.wsPr = t.wsPr; q.wsG = t.wsG; q.wsHl = t.wsHl; q.wsS = t.wsS; q.part = t.part;
        q.wpart = wpart[k];
        q.batch = B; q.dim = D; q.L = (int)L; q.N = N; q.R = R;
        q.nchunks = pl.scan.nchunks; q.cpb = pl.scan.cpb; q.nblocks = pl.scan.nblocks;
        q.accumulate = k >= 2;                           // a layout's first direction writes dx, its second adds
    }
    const bool vec = (L % 4 == 0) && aligned16(x) && aligned16(dx) && aligned16(dy_row_fwd) && aligned16(dy_row_rev) &&
                     aligned16(xT) && aligned16(dyTa) && aligned16(dyTb) && aligned16(dxT);
    const dim3 grid((unsigned)pl.scan.nblocks, (unsigned)B);
    if (pl.scan.nchunks > 1) {
        const dim3 g4(grid.x, grid.y, 4);
        if (vec) hipLaunchKernelGGL((core_bwd_reduce_kernel<NP, true>), g4, dim3(64), 0, st, a[0], a[1], a[2], a[3]);
        else hipLaunchKernelGGL((core_bwd_reduce_kernel<NP, false>), g4, dim3(64), 0, st, a[0], a[1], a[2], a[3]);
        if (pl.scan.nblocks > 1) {                       // all eight carries (four forward, four adjoint) in one batch
            CarryBatch cb{};
            const int nsegs = (int)carry_nsegs(pl.scan.nblocks);
            const size_t one = (size_t)nsegs * pl.scan.chains;
            for (int k = 0; k < 4; ++k) {
                cb.d[2 * k] = CarryDir{a[k].wsP, a[k].wsH, seg[k], seg[k] + one, pl.scan.nblocks, nsegs};
                cb.d[2 * k + 1] = CarryDir{a[k].wsPr, a[k].wsG, seg[k] + 2 * one, seg[k] + 3 * one, pl.scan.nblocks, nsegs};
            }
            launch_carry_batch(cb, 8, pl.scan.chains, st);
        }
    }
    const int order[4] = {0, 2, 1, 3};
    static const int dirmask = [] { const char* e = getenv("WM_CORE_BWD_DIRMASK"); return e ? atoi(e) : 15; }();   // tools only
    for (int i = 0; i < 4; ++i) {
        const int k = order[i];
        if (!((dirmask >> k) & 1)) continue;
        const dim3 blk(64 * Cfg::NW);
        if (k < 2) { if (vec) hipLaunchKernelGGL((core_bwd_chunk_kernel<NP, true, false>), grid, blk, 0, st, a[k]);
                     else hipLaunchKernelGGL((core_bwd_chunk_kernel<NP, false, false>), grid, blk, 0, st, a[k]); }
        else       { if (vec) hipLaunchKernelGGL((core_bwd_chunk_kernel<NP, true, true>), grid, blk, 0, st, a[k]);
                     else hipLaunchKernelGGL((core_bwd_chunk_kernel<NP, false, true>), grid, blk, 0, st, a[k]); }
    }
    {
        const dim3 tg((unsigned)((H + 31) / 32), (unsigned)((W + 31) / 32), (unsigned)(B * D)), tb(32, 8);
        hipLaunchKernelGGL(transpose_planes_kernel, tg, tb, 0, st, (const float*)dxT, dx, W, H, 1);   // dx += (dx^T)^T
    }
    CoreBwdFinishArgs f;
    for (int k = 0; k < 4; ++k) { f.part[k] = a[k].part; f.wpart[k] = wpart[k]; }
    f.wsum = wsum; f.A_logs = A_logs; f.dA_logs = dA_logs; f.dDs = dDs; f.dbias = ddt_projs_bias; f.dWdt = ddt_projs_weight;
    f.dWx = dx_proj_weight; f.batch = B; f.dim = D; f.N = N; f.R = R; f.NP = NP; f.nblocks = pl.scan.nblocks; f.slices = pl.slices;
    hipLaunchKernelGGL(core_bwd_finish_kernel, dim3((unsigned)D, 1, 4), dim3(256), 0, st, f);
    hipLaunchKernelGGL(core_bwd_wsum_kernel, dim3((unsigned)Cfg::NWT, (unsigned)pl.slices, 4), dim3(256), 0, st, f, (int)Cfg::NWT);
    hipLaunchKernelGGL(core_bwd_wfin_kernel, dim3((unsigned)Cfg::NWT, 1, 4), dim3(256), 0, st, f, (int)Cfg::NWT);
    return launch_status();
}

// waves of a linear_wgrad launch (a multiple of kLwWaves) and the tokens each takes
static long long linear_wgrad_waves(long long T, long long& slice) {
    long long waves = (T + 511) / 512;                                  // >= 512 tokens per wave
    if (waves > 4096) waves = 4096;
    if (waves < 1) waves = 1;
    waves = ((waves + kLwWaves - 1) / kLwWaves) * kLwWaves;
    slice = (T + waves - 1) / waves;
    slice = ((slice + 3) / 4) * 4;
    return waves;
}
template <int OT, int IT, bool DET = false>
static void linear_wgrad_launch(const float* gy, const float* x, float* dW, long long T, hipStream_t st) {
    long long slice;
    const long long waves = linear_wgrad_waves(T, slice);
    hipLaunchKernelGGL((linear_wgrad_kernel<OT, IT, DET>), dim3((unsigned)(waves / kLwWaves)), dim3(64 * kLwWaves), 0,
                       st, gy, x, dW, T, slice);
}

}  // namespace wm

using namespace wm;

extern "C" {

size_t wm_selscan_bwd_workspace_bytes(int batch, int dim, int L, int N, int G) {
    BwdPlan pl;
    if (bwd_plan(pl, batch, dim, L, N, G) != WM_OK) return 0;
    return pl.total;
}

// the deterministic form's room behind the plan's own workspace: the finish kernel's records [ysplit][dim][NP + pad], then (wpg > 1)
// wpg slabs each of dB and dC
struct BwdDetPlan { size_t fin_bytes, slab_elems, total; int ysplit; };
static void bwd_det_plan(BwdDetPlan& dp, const BwdPlan& pl, int batch, int dim, int L, int N, int G) {
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    dp.ysplit = bwd_finish_split(pl.nblocks, pl.NP + kPartPad);
    dp.fin_bytes = up((size_t)dp.ysplit * dim * (pl.NP + kPartPad) * sizeof(float));
    dp.slab_elems = pl.wpg > 1 ? (size_t)batch * G * N * L : 0;
    dp.total = up(pl.total) + dp.fin_bytes + up(2 * (size_t)pl.wpg * dp.slab_elems * sizeof(float));
}

static int selscan_bwd_entry(const float* u, const float* delta, const float* A, const float* Bm, const float* Cm,
                             const float* D, const float* delta_bias, const float* dy, float* du, float* ddelta,
                             float* dA, float* dB, float* dC, float* dD, float* dbias, void* workspace,
                             size_t workspace_bytes, int batch, int dim, int L, int N, int G, int delta_softplus,
                             void* stream, bool det) {
    if (batch == 0 || dim == 0 || L == 0) {
        if (batch < 0 || dim < 0 || L < 0) return WM_EINVAL;
        // the deterministic form's caller hands it uninitialised outputs: an empty problem's parameter gradients are zero, not
        // whatever the memory held (the other gradients have no element then)
        if (det && dim > 0 && N > 0 && N <= 32) {
            hipStream_t st = (hipStream_t)stream;
            hipError_t e = dA ? zero_out(dA, (size_t)dim * N * sizeof(float), st) : hipSuccess;
            if (e == hipSuccess) e = zero_pair(dD, dD ? (size_t)dim : 0, dbias, dbias ? (size_t)dim : 0, st);
            if (e != hipSuccess) return (int)e;
        }
        return WM_OK;
    }
    BwdPlan pl;
    int rc = bwd_plan(pl, batch, dim, L, N, G);
    if (rc) return rc;
    if (!u || !delta || !A || !Bm || !Cm || !dy || !du || !ddelta || !dA || !dB || !dC) return WM_ENULL;
    if (!workspace) return WM_ENULL;
    BwdDetPlan dp{};
    if (det) bwd_det_plan(dp, pl, batch, dim, L, N, G);
    if (workspace_bytes < (det ? dp.total : pl.total)) return WM_EWORKSPACE;
    if (!aligned16(workspace)) return WM_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    ScanBwdArgs a;
    a.u = u; a.delta = delta; a.A = A; a.Bm = Bm; a.Cm = Cm; a.D = D; a.bias = delta_bias; a.dy = dy;
    a.du = du; a.ddelta = ddelta; a.dB = dB; a.dC = dC;
    float* seg = nullptr;
    bwd_bind_workspace(a, pl, (char*)workspace, seg);
    a.batch = batch; a.dim = dim; a.L = L; a.N = N; a.G = G; a.dpg = dim / G; a.wpg = pl.wpg;
    a.softplus = delta_softplus ? 1 : 0; a.atomic_bc = pl.wpg > 1 && !det ? 1 : 0;
    a.bc_slab = 0;
    float* fin = nullptr;
    float* slabs = nullptr;
    if (det) {
        fin = (float*)((char*)workspace + (pl.total + 255) / 256 * 256);
        slabs = (float*)((char*)fin + dp.fin_bytes);
        if (pl.wpg > 1) { a.dB = slabs; a.dC = slabs + (size_t)pl.wpg * dp.slab_elems; a.bc_slab = (long long)dp.slab_elems; }
    }
    if (a.atomic_bc) {
        const size_t nb = (size_t)batch * G * N * L * sizeof(float);
        hipError_t e = zero_async(dB, nb, st);
        if (e == hipSuccess) e = zero_async(dC, nb, st);
        if (e != hipSuccess) return (int)e;
    }
    const bool vec = (L % 4 == 0) && aligned16(u) && aligned16(delta) && aligned16(Bm) && aligned16(Cm) &&
                     aligned16(dy) && aligned16(du) && aligned16(ddelta) && aligned16(dB) && aligned16(dC);
    if (pl.NP == 16) rc = vec ? bwd_launch<16, true>(a, pl, seg, dA, dD, dbias, st, fin)
                              : bwd_launch<16, false>(a, pl, seg, dA, dD, dbias, st, fin);
    else rc = vec ? bwd_launch<32, true>(a, pl, seg, dA, dD, dbias, st, fin) : bwd_launch<32, false>(a, pl, seg, dA, dD, dbias, st, fin);
    if (rc || !det || pl.wpg <= 1) return rc;
    // dB, dC = the wpg slabs added in ascending channel-slice order
    const long long n = (long long)dp.slab_elems;
    const int sv = vec ? 1 : 0;                                   // (L % 4 == 0: n % 4 == 0 and every slab starts 16-byte aligned)
    long long blocks = ((sv ? n / 4 : n) + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(det_slab_sum_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)a.dB, dB, n, pl.wpg, sv);
    hipLaunchKernelGGL(det_slab_sum_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)a.dC, dC, n, pl.wpg, sv);
    return launch_status();
}

int wm_selscan_bwd(const float* u, const float* delta, const float* A, const float* Bm, const float* Cm,
                   const float* D, const float* delta_bias, const float* dy, float* du, float* ddelta,
                   float* dA, float* dB, float* dC, float* dD, float* dbias, void* workspace,
                   size_t workspace_bytes, int batch, int dim, int L, int N, int G, int delta_softplus,
                   void* stream) {
    return selscan_bwd_entry(u, delta, A, Bm, Cm, D, delta_bias, dy, du, ddelta, dA, dB, dC, dD, dbias, workspace, workspace_bytes,
                             batch, dim, L, N, G, delta_softplus, stream, false);
}

size_t wm_selscan_bwd_det_workspace_bytes(int batch, int dim, int L, int N, int G) {
    BwdPlan pl;
    if (bwd_plan(pl, batch, dim, L, N, G) != WM_OK) return 0;
    BwdDetPlan dp;
    bwd_det_plan(dp, pl, batch, dim, L, N, G);
    return dp.total;
}

int wm_selscan_bwd_det(const float* u, const float* delta, const float* A, const float* Bm, const float* Cm,
                       const float* D, const float* delta_bias, const float* dy, float* du, float* ddelta,
                       float* dA, float* dB, float* dC, float* dD, float* dbias, void* workspace,
                       size_t workspace_bytes, int batch, int dim, int L, int N, int G, int delta_softplus,
                       void* stream) {
    return selscan_bwd_entry(u, delta, A, Bm, Cm, D, delta_bias, dy, du, ddelta, dA, dB, dC, dD, dbias, workspace, workspace_bytes,
                             batch, dim, L, N, G, delta_softplus, stream, true);
}

size_t wm_ss2d_core_bwd_workspace_bytes(int B, int D, int H, int W, int N, int R) {
    CoreBwdPlan2 pl;
    if (core_bwd_plan2(pl, B, D, H, W, N, R) != WM_OK) return 0;
    return pl.total;
}

int wm_ss2d_core_bwd(const float* x, const float* x_proj_weight, const float* dt_projs_weight,
                     const float* dt_projs_bias, const float* A_logs, const float* Ds, const float* dy_row_fwd,
                     const float* dy_row_rev, const float* dy_col_fwd, const float* dy_col_rev, float* dx,
                     float* dx_proj_weight, float* ddt_projs_weight, float* ddt_projs_bias, float* dA_logs, float* dDs,
                     void* workspace, size_t workspace_bytes, int B, int D, int H, int W, int N, int R, void* stream) {
    if (B == 0 || D == 0 || H == 0 || W == 0) return (B < 0 || D < 0 || H < 0 || W < 0) ? WM_EINVAL : WM_OK;
    hipStream_t st = (hipStream_t)stream;
    const bool nul = !x || !x_proj_weight || !dt_projs_weight || !dt_projs_bias || !A_logs || !Ds || !dy_row_fwd || !dy_row_rev ||
                     !dy_col_fwd || !dy_col_rev || !dx || !dx_proj_weight || !ddt_projs_weight || !ddt_projs_bias || !dA_logs ||
                     !dDs || !workspace;
    CoreBwdPlan2 pl;
    int rc = core_bwd_plan2(pl, B, D, H, W, N, R);
    if (rc) return rc;
    if (nul) return WM_ENULL;
    if (workspace_bytes < pl.total) return WM_EWORKSPACE;
    if (!aligned16(workspace)) return WM_EALIGN;
    if (pl.NP == 16)
        return core_bwd_v2<16>(pl, x, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds, dy_row_fwd, dy_row_rev, dy_col_fwd,
                               dy_col_rev, dx, dx_proj_weight, ddt_projs_weight, ddt_projs_bias, dA_logs, dDs, workspace, B, D, H, W, N, R, st);
    return core_bwd_v2<32>(pl, x, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds, dy_row_fwd, dy_row_rev, dy_col_fwd,
                           dy_col_rev, dx, dx_proj_weight, ddt_projs_weight, ddt_projs_bias, dA_logs, dDs, workspace, B, D, H, W, N, R, st);
}

size_t wm_linear_wgrad_det_workspace_bytes(int64_t T, int O, int I) {
    if (T <= 0 || O <= 0 || I <= 0 || O % 16 != 0 || I % 16 != 0 || O * I > 8192) return 0;
    long long slice;
    return (size_t)(linear_wgrad_waves((long long)T, slice) / kLwWaves) * O * I * sizeof(float);
}

int wm_linear_wgrad_det(const float* gy, const float* x, float* dW, void* workspace, size_t workspace_bytes, int64_t T, int O, int I,
                        void* stream) {
    if (T < 0 || O <= 0 || I <= 0) return WM_EINVAL;
    if (!dW) return WM_ENULL;
    hipStream_t st = (hipStream_t)stream;
    if (T == 0) {
        const hipError_t e = zero_async(dW, (size_t)O * I * sizeof(float), st);
        return e == hipSuccess ? WM_OK : (int)e;
    }
    if (!gy || !x || !workspace) return WM_ENULL;
    if (O % 16 != 0 || I % 16 != 0 || O * I > 8192) return WM_EUNSUPPORTED;
    if (workspace_bytes < wm_linear_wgrad_det_workspace_bytes(T, O, I)) return WM_EWORKSPACE;
    if (!aligned16(workspace)) return WM_EALIGN;
    long long slice;
    const long long nblk = linear_wgrad_waves((long long)T, slice) / kLwWaves;
#define WM_LW(OT, IT) if (O == 16 * OT && I == 16 * IT) {                                                                    \
        linear_wgrad_launch<OT, IT, true>(gy, x, (float*)workspace, (long long)T, st);                                       \
        return det_finish((const float*)workspace, nblk, (long long)O * I, DetOut{dW, nullptr, nullptr, kDetSplit, O * I, 0, 0}, st); }
    WM_LW(8, 2) WM_LW(2, 4) WM_LW(4, 1) WM_LW(1, 2) WM_LW(2, 1) WM_LW(1, 1) WM_LW(4, 2) WM_LW(2, 2) WM_LW(1, 4)
#undef WM_LW
    return WM_EUNSUPPORTED;
}

int wm_linear_wgrad(const float* gy, const float* x, float* dW, int64_t T, int O, int I, void* stream) {
    if (T < 0 || O <= 0 || I <= 0) return WM_EINVAL;
    if (!dW) return WM_ENULL;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = zero_out(dW, (size_t)O * I * sizeof(float), st);
    if (e != hipSuccess) return (int)e;
    if (T == 0) return WM_OK;
    if (!gy || !x) return WM_ENULL;
    if (O % 16 != 0 || I % 16 != 0 || O * I > 8192) return WM_EUNSUPPORTED;
#define WM_LW(OT, IT) if (O == 16 * OT && I == 16 * IT) { linear_wgrad_launch<OT, IT>(gy, x, dW, (long long)T, st); return launch_status(); }
    WM_LW(8, 2) WM_LW(2, 4) WM_LW(4, 1) WM_LW(1, 2) WM_LW(2, 1) WM_LW(1, 1) WM_LW(4, 2) WM_LW(2, 2) WM_LW(1, 4)
#undef WM_LW
    return WM_EUNSUPPORTED;
}

#if WM_BWD_STAMP
int wm_debug_bwd_stamps(unsigned long long* out, int reset) {      // host buffer of 44 values
    int rc = (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(wm::g_bwd_stamps), sizeof(unsigned long long) * 44);
    if (rc == 0 && reset) {
        unsigned long long z[44] = {};
        rc = (int)hipMemcpyToSymbol(HIP_SYMBOL(wm::g_bwd_stamps), z, sizeof(z));
    }
    return rc;
}
#endif

}  // extern "C"
