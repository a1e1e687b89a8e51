// scan_fwd.hip - C ABI over the selective scan and the fused SS2D core, forward.
#include "scan_common.h"
#include "ss2d_core.hip.h"

namespace wm {

// ------------------------------------------------------------------------------------------------
// selective-scan host side
// ------------------------------------------------------------------------------------------------
struct ScanPlan { int NP, wpg, rows, chunk_len, nchunks; size_t ws_bytes; };

void launch_carry_batch(CarryBatch cb, int ndirs, long long nchains, hipStream_t st) {
    ProfScope ps(3, st);
    const dim3 cgrid((unsigned)((nchains + 15) / 16), 1, (unsigned)ndirs), cblock(1024);
    int maxchunks = 0;
    for (int i = 0; i < ndirs; ++i) maxchunks = cb.d[i].nchunks > maxchunks ? cb.d[i].nchunks : maxchunks;
    if (maxchunks <= 1024 || !cb.d[0].segP) {
        hipLaunchKernelGGL((selscan_carry_kernel<false>), cgrid, cblock, 0, st, cb, nchains);
        return;
    }
    int maxsegs = 0;
    for (int i = 0; i < ndirs; ++i) {
        cb.d[i].nsegs = (int)carry_nsegs(cb.d[i].nchunks);
        maxsegs = cb.d[i].nsegs > maxsegs ? cb.d[i].nsegs : maxsegs;
    }
    const dim3 grid((unsigned)((nchains + 63) / 64), (unsigned)((maxsegs + 3) / 4), (unsigned)ndirs), block(256);
    hipLaunchKernelGGL((selscan_carry_seg_kernel<false>), grid, block, 0, st, cb, nchains);
    hipLaunchKernelGGL((selscan_carry_kernel<true>), cgrid, cblock, 0, st, cb, nchains);
    hipLaunchKernelGGL((selscan_carry_seg_kernel<true>), grid, block, 0, st, cb, nchains);
}
static void launch_carry(float* wsP, float* wsH, float* seg, long long nchains, int nchunks, hipStream_t st) {
    CarryBatch cb{};
    const int nsegs = (int)carry_nsegs(nchunks);
    cb.d[0] = CarryDir{wsP, wsH, seg, seg ? seg + (size_t)nsegs * nchains : nullptr, nchunks, nsegs};
    launch_carry_batch(cb, 1, nchains, st);
}

static int scan_plan(ScanPlan& pl, int batch, int dim, int L, int N, int G) {
    if (batch <= 0 || dim <= 0 || L <= 0 || N <= 0 || G <= 0) return WM_EINVAL;
    if (N > 32) return WM_EUNSUPPORTED;
    if (dim % G != 0) return WM_EINVAL;
    const int dpg = dim / G;
    pl.NP = N <= 16 ? 16 : 32;
    pl.wpg = (dpg + 63) / 64;
    const long long rows = (long long)batch * G * pl.wpg;
    if (rows > 65535) return WM_EUNSUPPORTED;
    pl.rows = (int)rows;
    // enough chunks to keep every CU's wave slots busy for several rounds (256 CUs x ~12 resident
    // single-wave workgroups), but never shorter than 64 steps
#ifndef WM_TARGET_WAVES
#define WM_TARGET_WAVES (256LL * 12 * 4)
#endif
    const long long target_waves = WM_TARGET_WAVES;
    long long want = (target_waves + rows - 1) / rows;           // chunks wanted per wave-row
    long long cl = ((long long)L + want - 1) / want;
    cl = ((cl + kTile - 1) / kTile) * kTile;
    if (cl < 64) cl = 64;
    pl.chunk_len = (int)cl;
    pl.nchunks = (int)(((long long)L + cl - 1) / cl);
    pl.ws_bytes = pl.nchunks > 1 ? (size_t)2 * (pl.nchunks + carry_nsegs(pl.nchunks)) * batch * dim * pl.NP * sizeof(float) : 0;
    return WM_OK;
}

template <int NP, bool VEC>
static int scan_launch(const ScanArgs& a, const ScanPlan& pl, hipStream_t st) {
    const dim3 grid((unsigned)pl.nchunks, (unsigned)pl.rows), block(64);
    if (pl.nchunks > 1) {
        {
            ProfScope ps(2, st);
            hipLaunchKernelGGL((selscan_chunk_kernel<NP, 1, VEC>), grid, block, 0, st, a);
        }
        const long long nchains = (long long)a.batch * a.dim * NP;
        launch_carry(a.wsP, a.wsH, a.wsH + (size_t)pl.nchunks * nchains, nchains, pl.nchunks, st);
    }
    {
        ProfScope ps(4, st);
        hipLaunchKernelGGL((selscan_chunk_kernel<NP, 3, VEC>), grid, block, 0, st, a);
    }
    return launch_status();
}

// ------------------------------------------------------------------------------------------------
// SS2D core, second generation (ss2d_core.hip.h): reduce (4 directions) -> carry -> scan (4 directions)
// ------------------------------------------------------------------------------------------------
struct CorePlan {
    int NP, NW;
    int row_chunk, row_nchunks, row_wgs, row_cpw;
    int col_seg, col_nseg, col_tiles, col_wgs;
    long long col_nchunks, max_chunks;
    size_t half_bytes, ytmp_bytes, prep_bytes, total;   // one H (or stored-P) array of one direction; merged-mode y buffers;
                                                        // the prep kernel's output; everything
    size_t p_bytes;                                     // what one direction keeps for P: a sum_dt array [chunk][B * D]
                                                        // (half_bytes / NP), or half_bytes on the stored-P path
};

// 0: the reduce pass stores sum_dt and ss2d_core_carry_kernel forms P; 1: the reduce pass stores P, selscan_carry_kernel
// (wm_ss2d_core_carry_select; the same H_in bits either way: tests/test_core_carry.py)
static std::atomic<int> g_core_carry_select{0};

// Length of one core launch (in row-tile times) under the dispatch model of core_plan's comment, replaying
// ss2d_core_kernel's blockIdx -> (direction, slot) mapping.  Costs measured on MI355X (tools/bench_core.py with
// WM_CORE_DIRMASK, gpurun_out r3a): a 16-wave tile round takes the same 15.7 us (chunk-scan) / 13.4 us (chunk-reduce) in
// a column workgroup (68 tiles, one round of 240: 1.065 / 0.919 ms) as in a row workgroup (60 tiles: 0.942 / 0.790 ms),
// so kColTile = 1; a workgroup costs about one tile round on top of its tiles (UHD level 2: 240 workgroups of 34 tiles
// in one round 1.07 ms, 512 of 17 / 15 tiles in two rounds 1.12 ms; level 3: 234 of 9 tiles 0.319 ms, 222 with 10-tile
// row workgroups 0.340 ms) - launch, LDS fill, carried-in state, and above all the drain: a compute unit holds one
// workgroup, and the next one starts only when the slowest of its 16 waves has finished.
// Returns early (a value >= bound) once the launch is known to be no better than `bound`.
#ifndef WM_CORE_COST_COL
#define WM_CORE_COST_COL 1.0
#endif
#ifndef WM_CORE_COST_WG
#define WM_CORE_COST_WG 1.0
#endif
static double core_makespan(const CorePlan& pl, int B, int H, double bound) {
    const double kColTile = WM_CORE_COST_COL, kWgStart = WM_CORE_COST_WG, kCarry = 0.0005;
    const int slots = 32 * (16 / pl.NW);
    double freeat[8][64];
    for (int x = 0; x < 8; ++x) for (int i = 0; i < slots; ++i) freeat[x][i] = 0.0;
    const long long per_b = 2LL * pl.row_wgs + 2LL * pl.col_wgs;
    const long long total = (long long)B * per_b;
    // a row workgroup's waves share its row_cpw chunks: tile rounds = chunks x tiles per chunk / waves
    const int row_tiles = (pl.row_cpw * (pl.row_chunk / 16) + pl.NW - 1) / pl.NW;
    double span = 0.0;
    {   // lower bound: all work spread evenly
        double work = 0.0;
        for (int sg = 0; sg < pl.col_nseg; ++sg) {
            const int rows = (H - sg * pl.col_seg) < pl.col_seg ? (H - sg * pl.col_seg) : pl.col_seg;
            work += 2.0 * B * pl.col_tiles * (((rows + 15) / 16) * kColTile + kWgStart);
        }
        work += 2.0 * B * pl.row_wgs * (row_tiles + kWgStart);
        if (work / (8.0 * slots) >= bound) return work / (8.0 * slots);
    }
    for (long long i = 0; i < total; ++i) {
        const long long r = i % per_b;
        double cost;
        if (r < 2LL * pl.col_wgs) {
            const int idx = (int)(r >> 1);
            const int wg = (((idx >> 3) << 2) + (idx & 3)) * 2 + ((idx >> 2) & 1);
            if (wg >= pl.col_tiles * pl.col_nseg) continue;
            const int sg = wg / pl.col_tiles;
            const int rows = (H - sg * pl.col_seg) < pl.col_seg ? (H - sg * pl.col_seg) : pl.col_seg;
            cost = ((rows + 15) / 16) * kColTile + kWgStart;
        } else {
            const long long wg = (r - 2LL * pl.col_wgs) >> 1;
            long long c0 = wg * pl.row_cpw;                                   // first chunk of the workgroup
            if (c0 >= pl.row_nchunks) continue;
            cost = row_tiles + kWgStart;                                       // (the very last chunk may be shorter)
        }
        double* f = freeat[i & 7];
        int best = 0;
        for (int j = 1; j < slots; ++j) if (f[j] < f[best]) best = j;
        f[best] += cost;
        if (f[best] > span) { span = f[best]; if (span >= bound) return span; }
    }
    const long long chunks = pl.col_nchunks > pl.row_nchunks ? pl.col_nchunks : pl.row_nchunks;
    return span + kCarry * (double)chunks;
}

static int core_plan(CorePlan& pl, int B, int D, int H, int W, int N, int R, int merged, bool stored_p) {
    if (B <= 0 || D <= 0 || H <= 0 || W <= 0 || N <= 0 || R <= 0) return WM_EINVAL;
    if (N > 32 || R > 4 || D > 64) return WM_EUNSUPPORTED;
    const long long L = (long long)H * W;
    if (L * D > 0x7fffffffLL) return WM_EUNSUPPORTED;          // 32-bit element offsets inside one batch item
    pl.NP = N <= 16 ? 16 : 32;
    // (12-wave and 8-wave workgroups at N <= 16 were measured slower or equal at every UHD level:
    // profiles/r04/core_forward_experiments.txt, profiles/r06/core_forward_analysis.md item 8)
    pl.NW = pl.NP == 16 ? 16 : 8;
    const int NW = pl.NW;
    pl.col_tiles = (W + NW - 1) / NW;
    // Work split.  Column workgroups: one per (NW-column tile, segment of `col_seg` rows); row workgroups: NW waves with
    // one chunk of `row_chunk` steps each.  Workgroup i goes to XCD i % 8 and there to the first of 32 compute units
    // (x 2 workgroups at NW = 8) that frees up - so a launch is list scheduling in workgroup-id order, and its length
    // is decided by how the LAST workgroups fill the machine.  Round 2 gave the row workgroups the column workgroups'
    // length: 480 equal workgroups on 256 compute units at UHD level 1 = 2 rounds, the second 7/8 full, and halving or
    // quartering the row chunks changes nothing (480 k / 256 is never whole).  Now the plan is searched: every
    // (segments per column, tiles per row chunk) pair is replayed through that dispatch model with measured per-tile
    // costs (core_makespan) and the shortest launch wins, e.g. level 1: 240 column workgroups of 68 tiles + 272 row
    // workgroups of 60.  Plans are cached per shape (the search replays ~10^5 workgroups).
    const long long RT = ((L + 15) / 16 + NW - 1) / NW;             // row workgroup-tiles per direction
    // Row workgroups hand their chunks to their waves on demand (ss2d_core.hip.h), kRowSplit chunks per wave.  Measured
    // (gpurun_out r3h, UHD levels 1 / 2 / 3, ms per call): 1 chunk per wave 3.564 / 1.034 / 0.323, 2: 3.541 / 1.046 /
    // 0.339, 3: 3.498 / 1.081 / 0.344, 4: 3.584 / 1.062 / 0.366 - shorter chunks do even out the waves' lifetimes (566-918 us
    // instead of 370-857 at level 1) but the launch does not get shorter (the remaining waves of a SIMD were using the
    // issue slots of the finished ones) and the carry pays for the extra chunks: 1.
#ifndef WM_CORE_ROW_SPLIT
#define WM_CORE_ROW_SPLIT 1
#endif
    constexpr int kRowSplit = WM_CORE_ROW_SPLIT;
    struct Cand { int seg, nseg, row_chunk; };
    auto fill = [&](const Cand& c) {
        pl.col_seg = c.seg; pl.col_nseg = c.nseg;
        pl.col_nchunks = (long long)W * pl.col_nseg;
        pl.col_wgs = ((pl.col_tiles * pl.col_nseg + 7) / 8) * 8;
        pl.row_chunk = c.row_chunk;
        pl.row_nchunks = (int)((L + c.row_chunk - 1) / c.row_chunk);
        pl.row_cpw = NW * kRowSplit;
        pl.row_wgs = (pl.row_nchunks + pl.row_cpw - 1) / pl.row_cpw;
    };
    {
        // shape -> plan, most recently used first; the least recently used entry is evicted at kPlanCache entries (a
        // serving process meets an open-ended set of image sizes - three pyramid levels each; a cache that stopped
        // inserting when full re-ran the 5-18 ms search on every call for every later shape)
        constexpr size_t kPlanCache = 1024;
        static std::mutex mu;
        static std::list<std::pair<std::array<int, 6>, Cand>> lru;
        static std::map<std::array<int, 6>, std::list<std::pair<std::array<int, 6>, Cand>>::iterator> index;
        const std::array<int, 6> key = {B, D, H, W, pl.NP, NW};
        std::lock_guard<std::mutex> lk(mu);
        const Cand* hit = nullptr;
        {
            const auto it = index.find(key);
            if (it != index.end()) { lru.splice(lru.begin(), lru, it->second); hit = &lru.front().second; }
        }
        if (hit) fill(*hit);
        else {
            double best = 1e300; Cand bc{((H + 15) / 16) * 16, 1, 32};
            int last_seg = -1;
            for (int n = 1; n <= 64; ++n) {
                int sg = (H + n - 1) / n;
                sg = ((sg + 15) / 16) * 16;
                if (n > 1 && sg < 32) break;
                if (sg == last_seg) continue;
                last_seg = sg;
                const int nn = (H + sg - 1) / sg;
                int last_chunk = -1;
                for (long long ct = RT < 128 ? RT : 128; ct >= 2; --ct) {      // tile rounds per row workgroup
                    const long long m = (RT + ct - 1) / ct;                    // row workgroups per direction
                    long long c = (L + m * NW * kRowSplit - 1) / (m * NW * kRowSplit);
                    c = ((c + 15) / 16) * 16;
                    if (c < 32) c = 32;
                    if ((int)c == last_chunk) continue;
                    last_chunk = (int)c;
                    const Cand cand{sg, nn, (int)c};
                    fill(cand);
                    const double t = core_makespan(pl, B, H, best);
                    if (t < best * 0.995) { best = t; bc = cand; }
                }
            }
            fill(bc);
            lru.emplace_front(key, bc);
            index[key] = lru.begin();
            if (lru.size() > kPlanCache) { index.erase(lru.back().first); lru.pop_back(); }
        }
    }
    pl.max_chunks = pl.col_nchunks > pl.row_nchunks ? pl.col_nchunks : pl.row_nchunks;
    if ((long long)B * (2LL * pl.row_wgs + 2LL * pl.col_wgs) > 0x7fffffffLL) return WM_EUNSUPPORTED;
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    pl.half_bytes = up((size_t)pl.max_chunks * B * D * pl.NP * sizeof(float));
    pl.ytmp_bytes = merged ? up((size_t)B * D * L * sizeof(float)) : 0;
    pl.prep_bytes = up((size_t)4 * (pl.NP == 16 ? CoreCfg<16>::PREP : CoreCfg<32>::PREP) * sizeof(float));
    pl.p_bytes = stored_p ? pl.half_bytes : up((size_t)pl.max_chunks * B * D * sizeof(float));
    pl.total = 4 * (pl.half_bytes + pl.p_bytes) + 3 * pl.ytmp_bytes + pl.prep_bytes;
    return WM_OK;
}

template <int NP, int NW, bool RHI, typename TP, bool VEC>
static int core_launch(const CoreArgs& a, const CorePlan& pl, bool do_prep, hipStream_t st) {
    constexpr int lds = core_lds_bytes<NP, NW>();
    static bool configured1[64] = {}, configured3[64] = {};     // the reduce pass (phase 1) and the scan pass (phase 3)
    int rc = lds_optin((const void*)ss2d_core_kernel<NP, NW, 1, RHI, TP, VEC>, lds, configured1);
    if (!rc) rc = lds_optin((const void*)ss2d_core_kernel<NP, NW, 3, RHI, TP, VEC>, lds, configured3);
    if (rc) return rc;
    const dim3 grid((unsigned)(a.B * (2 * pl.row_wgs + 2 * pl.col_wgs))), block(64 * NW);
    const bool split = pl.row_nchunks > 1 || pl.col_nchunks > 1;
    if (do_prep) {   // parameters -> bf16 weight fragments, A * log2(e), per-channel constants (four small blocks)
        ProfScope ps(10, st);
        hipLaunchKernelGGL((ss2d_core_prep_kernel<NP, true>), dim3(4), dim3(256), 0, st, a.Wx, a.Wdt, a.dtb, a.A_logs, a.Ds,
                           const_cast<float*>(a.prep), a.D, a.N, a.R);
    }
    if (split) {
        {
            ProfScope ps(10, st);
            hipLaunchKernelGGL((ss2d_core_kernel<NP, NW, 1, RHI, TP, VEC>), grid, block, lds, st, a);
        }
        ProfScope ps(3, st);
        const int order[4] = {0, 2, 1, 3};
        const long long nchains = (long long)a.B * a.D * NP;
        if (a.sdt[0]) {
            CoreCarryBatch cb{};
            for (int i = 0; i < 4; ++i) {
                const int k = order[i];
                cb.d[i] = CoreCarryDir{a.sdt[k], a.wsH[k], a.prep + (size_t)k * CoreCfg<NP>::PREP + CoreCfg<NP>::P_A2,
                                       (k & 1) ? (int)pl.col_nchunks : pl.row_nchunks};
            }
            // summaries per segment of the longest direction -> how many a thread keeps in registers between fold and re-walk
            // (the kernel's KEEP; 36 x 5 registers is what two waves per SIMD leave); longer sequences stream them twice
            const int per = (int)((pl.max_chunks + kCarrySeg - 1) / kCarrySeg);
#define WM_CARRY_GO(KEEP)                                                                                                      \
    hipLaunchKernelGGL((ss2d_core_carry_kernel<NP, KEEP>), dim3((unsigned)((nchains + kCoreCarryChains - 1) / kCoreCarryChains), 1, 4), \
                       dim3(512), 0, st, cb, a.B * a.D, a.D)
            if (per <= 16) WM_CARRY_GO(16);
            else if (per <= 24) WM_CARRY_GO(24);
            else if (per <= 36) WM_CARRY_GO(36);
            else WM_CARRY_GO(0);
#undef WM_CARRY_GO
        } else {
            CarryBatch cb{};
            for (int i = 0; i < 4; ++i) {
                const int k = order[i];
                cb.d[i] = CarryDir{a.wsP[k], a.wsH[k], nullptr, nullptr, (k & 1) ? (int)pl.col_nchunks : pl.row_nchunks, 0};
            }
            hipLaunchKernelGGL((selscan_carry_kernel<false>), dim3((unsigned)((nchains + 15) / 16), 1, 4), dim3(1024), 0,
                               st, cb, nchains);
        }
    }
    {
        ProfScope ps(8, st);
        hipLaunchKernelGGL((ss2d_core_kernel<NP, NW, 3, RHI, TP, VEC>), grid, block, lds, st, a);
    }
    return launch_status();
}
}  // namespace wm

using namespace wm;

extern "C" {

size_t wm_selscan_fwd_workspace_bytes(int batch, int dim, int L, int N, int G) {
    ScanPlan pl;
    if (scan_plan(pl, batch, dim, L, N, G) != WM_OK) return 0;
    return pl.ws_bytes;
}

int wm_selscan_fwd(const float* u, const float* delta, const float* A, const float* Bm, const float* Cm,
                   const float* D, const float* z, const float* delta_bias, float* out,
                   float* last_state, void* workspace, size_t workspace_bytes, int batch, int dim, int L,
                   int N, int G, int delta_softplus, void* stream) {
    if (batch == 0 || dim == 0 || L == 0) return (batch < 0 || dim < 0 || L < 0) ? WM_EINVAL : WM_OK;
    ScanPlan pl;
    int rc = scan_plan(pl, batch, dim, L, N, G);
    if (rc) return rc;
    if (!u || !delta || !A || !Bm || !Cm || !out) return WM_ENULL;
    if (pl.ws_bytes > 0) {
        if (!workspace) return WM_ENULL;
        if (workspace_bytes < pl.ws_bytes) return WM_EWORKSPACE;
        if (!aligned16(workspace)) return WM_EALIGN;
    }
    ScanArgs a;
    a.u = u; a.delta = delta; a.A = A; a.Bm = Bm; a.Cm = Cm; a.D = D; a.z = z; a.bias = delta_bias;
    a.out = out; a.last_state = last_state;
    a.wsP = (float*)workspace;
    a.wsH = a.wsP ? a.wsP + (size_t)pl.nchunks * batch * dim * pl.NP : nullptr;
    a.batch = batch; a.dim = dim; a.L = L; a.N = N; a.G = G; a.dpg = dim / G; a.wpg = pl.wpg;
    a.chunk_len = pl.chunk_len; a.nchunks = pl.nchunks; a.softplus = delta_softplus ? 1 : 0;
    const bool vec = (L % 4 == 0) && aligned16(u) && aligned16(delta) && aligned16(Bm) && aligned16(Cm) &&
                     aligned16(out) && (!z || aligned16(z));
    hipStream_t st = (hipStream_t)stream;
    if (pl.NP == 16) return vec ? scan_launch<16, true>(a, pl, st) : scan_launch<16, false>(a, pl, st);
    return vec ? scan_launch<32, true>(a, pl, st) : scan_launch<32, false>(a, pl, st);
}

size_t wm_ss2d_core_fwd_workspace_bytes(int B, int D, int H, int W, int N, int R, int merged) {
    // (sized for fp32 planes; bf16 planes need less for the merged mode's temporaries)
    CorePlan pl;
    if (core_plan(pl, B, D, H, W, N, R, merged == 1, g_core_carry_select.load(std::memory_order_relaxed) == 1) != WM_OK) return 0;
    return pl.total;
}

size_t wm_ss2d_core_prep_bytes(int N) {
    if (N <= 0 || N > 32) return 0;
    return (size_t)4 * (N <= 16 ? CoreCfg<16>::PREP : CoreCfg<32>::PREP) * sizeof(float);
}

int wm_ss2d_core_prep(const float* x_proj_weight, const float* dt_projs_weight, const float* dt_projs_bias,
                      const float* A_logs, const float* Ds, void* prepared, int D, int N, int R, void* stream) {
    if (D <= 0 || N <= 0 || R <= 0) return WM_EINVAL;
    if (N > 32 || R > 4 || D > 64) return WM_EUNSUPPORTED;
    if (!x_proj_weight || !dt_projs_weight || !dt_projs_bias || !A_logs || !Ds || !prepared) return WM_ENULL;
    if (!aligned16(prepared)) return WM_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    if (N <= 16)
        hipLaunchKernelGGL((ss2d_core_prep_kernel<16, true>), dim3(4), dim3(256), 0, st, x_proj_weight, dt_projs_weight,
                           dt_projs_bias, A_logs, Ds, (float*)prepared, D, N, R);
    else
        hipLaunchKernelGGL((ss2d_core_prep_kernel<32, true>), dim3(4), dim3(256), 0, st, x_proj_weight, dt_projs_weight,
                           dt_projs_bias, A_logs, Ds, (float*)prepared, D, N, R);
    return launch_status();
}

int wm_ss2d_core_carry_select(int mode) {
    if (mode < 0 || mode > 1) return WM_EINVAL;
    g_core_carry_select.store(mode, std::memory_order_relaxed);
    return WM_OK;
}

int wm_ss2d_core_plan(int B, int D, int H, int W, int N, int R, int* out10) {
    if (!out10) return WM_ENULL;
    CorePlan pl;
    const int rc = core_plan(pl, B, D, H, W, N, R, 0, false);
    if (rc) return rc;
    out10[0] = pl.NW; out10[1] = pl.col_seg; out10[2] = pl.col_nseg; out10[3] = pl.col_tiles; out10[4] = pl.col_wgs;
    out10[5] = pl.row_chunk; out10[6] = pl.row_nchunks; out10[7] = pl.row_wgs;      // (row_wgs x 2 NW chunks, taken on demand)
    out10[8] = B * (2 * pl.row_wgs + 2 * pl.col_wgs);
    out10[9] = (int)(100.0 * core_makespan(pl, B, H, 1e300));
    return WM_OK;
}

int wm_ss2d_core_fwd(const void* x, const float* x_proj_weight, const float* dt_projs_weight,
                     const float* dt_projs_bias, const float* A_logs, const float* Ds, void* y_row_fwd,
                     void* y_row_rev, void* y_col_fwd, void* y_col_rev, int merged, void* workspace,
                     size_t workspace_bytes, const void* prepared, int B, int D, int H, int W, int N, int R, int plane_dtype,
                     void* stream) {
    if (B == 0 || D == 0 || H == 0 || W == 0) return (B < 0 || D < 0 || H < 0 || W < 0) ? WM_EINVAL : WM_OK;
    if (plane_dtype != WM_F32 && plane_dtype != WM_BF16) return WM_EUNSUPPORTED;
    CorePlan pl;
    const bool stored_p = g_core_carry_select.load(std::memory_order_relaxed) == 1;      // read once: sizes and launch agree
    int rc = core_plan(pl, B, D, H, W, N, R, merged == 1, stored_p);
    if (rc) return rc;
    if (!x || !x_proj_weight || !dt_projs_weight || !dt_projs_bias || !A_logs || !Ds || !y_row_fwd) return WM_ENULL;
    if (merged < 0 || merged > 1) return WM_EINVAL;       // (2 was round 4's two-plane mode: measured slower, deleted in round 5)
    if (merged == 0 && (!y_row_rev || !y_col_fwd || !y_col_rev)) return WM_ENULL;
    if (!workspace) return WM_ENULL;
    if (workspace_bytes < pl.total) return WM_EWORKSPACE;
    if (!aligned16(workspace)) return WM_EALIGN;
    // 16-byte tile accesses when the map width allows them (every size the network itself produces: it pads its input
    // to multiples of 8); otherwise the same kernels with element-wise tile accesses (fp32 planes only).
    const bool planes16 = aligned16(x) && aligned16(y_row_fwd) &&
                          (merged || (aligned16(y_row_rev) && aligned16(y_col_fwd) && aligned16(y_col_rev)));
    const bool vec = (W % 4 == 0) && planes16;
    if (!vec && plane_dtype != WM_F32) return (W % 4 == 0) ? WM_EALIGN : WM_EUNSUPPORTED;
    {
        auto mis4 = [](const void* q) { return q && ((uintptr_t)q & 3) != 0; };
        if (mis4(x) || mis4(y_row_fwd) || (!merged && (mis4(y_row_rev) || mis4(y_col_fwd) || mis4(y_col_rev)))) return WM_EALIGN;
    }
    hipStream_t st = (hipStream_t)stream;
    CoreArgs a;
    a.x = x; a.Wx = x_proj_weight; a.Wdt = dt_projs_weight; a.dtb = dt_projs_bias; a.A_logs = A_logs; a.Ds = Ds;
    char* w = (char*)workspace;
    for (int k = 0; k < 4; ++k) {        // [H x 4 | P or sum_dt x 4 | merged-mode y x 3 | prep]
        a.wsH[k] = (float*)(w + (size_t)k * pl.half_bytes);
        float* pk = (float*)(w + 4 * pl.half_bytes + (size_t)k * pl.p_bytes);
        a.wsP[k] = stored_p ? pk : nullptr;
        a.sdt[k] = stored_p ? nullptr : pk;
    }
    char* yt = w + 4 * (pl.half_bytes + pl.p_bytes);
    a.prep = prepared ? (const float*)prepared : (const float*)(yt + 3 * pl.ytmp_bytes);
    if (prepared && !aligned16(prepared)) return WM_EALIGN;
    // direction k: 0 row forward, 1 column forward, 2 row reversed, 3 column reversed (the reference's xs order, :451-452)
    a.y[0] = y_row_fwd;
    a.y[1] = merged ? (void*)yt : y_col_fwd;
    a.y[2] = merged ? (void*)(yt + pl.ytmp_bytes) : y_row_rev;
    a.y[3] = merged ? (void*)(yt + 2 * pl.ytmp_bytes) : y_col_rev;
    a.B = B; a.D = D; a.H = H; a.W = W; a.L = H * W; a.N = N; a.R = R;
    a.row_chunk = pl.row_chunk; a.row_nchunks = pl.row_nchunks; a.row_wgs = pl.row_wgs; a.row_cpw = pl.row_cpw;
    a.stamps = nullptr;
#if WM_CORE_STAMP
    {   // diagnostics build: WM_CORE_STAMPS=<device pointer, decimal> receives [workgroups][waves][8] cycle totals of the scan launch
        const char* e = getenv("WM_CORE_STAMPS");
        a.stamps = e ? (unsigned long long*)strtoull(e, nullptr, 10) : nullptr;
    }
#endif
    {   // WM_CORE_DIRMASK (tools only): run a subset of the four directions, e.g. 1 = row forward alone
        static const int mask = [] { const char* e = getenv("WM_CORE_DIRMASK"); return e ? atoi(e) : 15; }();
        a.dirmask = mask;
    }
    a.col_seg = pl.col_seg; a.col_nseg = pl.col_nseg; a.col_tiles = pl.col_tiles; a.col_wgs = pl.col_wgs;
#define WM_CORE_GO(TP, VEC)                                                                                                   \
    do {                                                                                                                      \
        const bool dp = prepared == nullptr;                                                                                  \
        if (pl.NP == 16) rc = R > 2 ? core_launch<16, 16, true, TP, VEC>(a, pl, dp, st) : core_launch<16, 16, false, TP, VEC>(a, pl, dp, st); \
        else rc = R > 2 ? core_launch<32, 8, true, TP, VEC>(a, pl, dp, st) : core_launch<32, 8, false, TP, VEC>(a, pl, dp, st); \
    } while (0)
    if (!vec) WM_CORE_GO(float, false);
    else if (plane_dtype == WM_F32) WM_CORE_GO(float, true);
    else WM_CORE_GO(bf16_t, true);
#undef WM_CORE_GO
    if (rc) return rc;
    if (merged) {
        const long long n = (long long)B * D * a.L, n4 = n / 4;
        ProfScope ps(8, st);
        if (!vec || (n & 3))
            hipLaunchKernelGGL((ss2d_sum4_kernel<float, false>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (float*)a.y[0],
                               (const float*)a.y[2], (const float*)a.y[1], (const float*)a.y[3], n);
        else if (plane_dtype == WM_F32)
            hipLaunchKernelGGL((ss2d_sum4_kernel<float, true>), dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, (float*)a.y[0],
                               (const float*)a.y[2], (const float*)a.y[1], (const float*)a.y[3], n4);
        else
            hipLaunchKernelGGL((ss2d_sum4_kernel<bf16_t, true>), dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, (bf16_t*)a.y[0],
                               (const bf16_t*)a.y[2], (const bf16_t*)a.y[1], (const bf16_t*)a.y[3], n4);
    }
    return launch_status();
}

}  // extern "C"
