// emulate_patch_batch.cpp - paired_patches_kernel (csrc/patch_batch.hip.h) run on the HOST under AddressSanitizer / UBSan, against
// the definition written out directly.  The kernel header is compiled for the CPU through tools/hip_host_shim (256 std::threads and
// a barrier per workgroup, workgroups one after another); every image sits in a heap block of exactly 3 h w bytes, so a read
// outside an image is an ASan report.  Cases: P = 40 / 33 / 32 / 64, images larger and smaller than the patch (down to 1 x 1), all
// eight modes, both channel orders, crops at the extremes and random, table rows with top / left / mode OUT of range (the kernel
// clamps), and a row that names no image (zeros).  Prints the number of elements compared and of differences; exit status 1 on any.
// No GPU, a few minutes (thread creation dominates).
//
//   cd tools && g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I hip_host_shim emulate_patch_batch.cpp -o emulate_patch_batch \
//       -lpthread && ./emulate_patch_batch
#include <array>
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <thread>
#include <vector>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
thread_local Idx threadIdx;
Idx blockIdx;
static pthread_barrier_t bar;
void __syncthreads() { pthread_barrier_wait(&bar); }
#include "../wave_mamba_amd/csrc/patch_batch.hip.h"
using namespace wm;

static long long refl(long long y, long long n) { long long m = y % (2 * n); return m < n ? m : 2 * n - 1 - m; }
static void reference(const uint8_t* img, long long h, long long w, long long top, long long left, int mode, int P, int swap, float* out) {
    for (int i = 0; i < P; ++i) for (int j = 0; j < P; ++j) {
        int r, c;
        switch (mode) {
            case 0: r = i; c = j; break; case 1: r = P-1-i; c = j; break; case 2: r = j; c = P-1-i; break; case 3: r = j; c = i; break;
            case 4: r = P-1-i; c = P-1-j; break; case 5: r = i; c = P-1-j; break; case 6: r = P-1-j; c = i; break; default: r = P-1-j; c = P-1-i;
        }
        long long sy = refl(top + r, h), sx = refl(left + c, w);
        for (int ch = 0; ch < 3; ++ch) out[((long long)ch * P + i) * P + j] = (float)img[(sy * w + sx) * 3 + (swap ? 2 - ch : ch)] / 255.0f;
    }
}
static void launch(const long long* table, float* lq, float* gt, int B, int P, int swap) {
    int tiles = (P + 31) / 32;
    for (int blk = 0; blk < tiles * tiles * 2 * B; ++blk) {
        blockIdx.x = blk;
        std::vector<std::thread> th;
        for (int t = 0; t < 256; ++t) th.emplace_back([=] { threadIdx.x = t; paired_patches_kernel(table, lq, gt, P, tiles, swap); });
        for (auto& x : th) x.join();
    }
}
int main() {
    pthread_barrier_init(&bar, nullptr, 256);
    std::mt19937 rng(1);
    struct Case { int P; std::vector<std::pair<int,int>> shapes; };
    std::vector<Case> cases = {{40, {{97,131},{64,200},{41,43}}}, {33, {{33,33},{50,35}}}, {32, {{32,32},{20,50},{50,20},{20,20},{7,9},{1,1}}}, {64,{{70,65},{64,64}}}};
    long long bad = 0, total = 0;
    for (auto& cs : cases) for (int swap = 0; swap < 2; ++swap) for (int rep = 0; rep < 3; ++rep) {
        int P = cs.P;
        std::vector<long long> table; std::vector<uint8_t*> imgs; std::vector<std::array<long long,6>> rows;
        for (auto& sh : cs.shapes) for (int mode = 0; mode < 8; ++mode) {
            long long h = sh.first, w = sh.second, n = 3 * h * w;
            int misalign = rng() % 4;
            uint8_t* a = (uint8_t*)malloc(n), *b = (uint8_t*)malloc(n);  // exact size: ASan sees any read outside
            for (long long k = 0; k < n; ++k) { a[k] = rng(); b[k] = rng(); }
            (void)misalign;
            long long H = std::max<long long>(h, P), W = std::max<long long>(w, P);
            long long top = rep == 0 ? 0 : rep == 1 ? H - P : rng() % (H - P + 1), left = rep == 0 ? W - P : rep == 1 ? 0 : rng() % (W - P + 1);
            long long ttop = top, tleft = left; int tmode = mode;
            if (rep == 2 && mode % 3 == 0) { ttop = top == H - P ? H + 1000 : -5; tleft = left == 0 ? -7 : (left == W - P ? W + 3 : left); tmode = mode + 8; if (ttop < 0) top = 0; if (tleft < 0) left = 0; }
            long long row[8] = {(long long)(uintptr_t)a, (long long)(uintptr_t)b, h, w, ttop, tleft, tmode, 0};
            table.insert(table.end(), row, row + 8);
            imgs.push_back(a); imgs.push_back(b);
            rows.push_back({h, w, top, left, mode, 0});
        }
        int B = rows.size();
        std::vector<float> lq((size_t)B * 3 * P * P, -1.f), gt((size_t)B * 3 * P * P, -1.f), want((size_t)3 * P * P);
        launch(table.data(), lq.data(), gt.data(), B, P, swap);
        for (int b = 0; b < B; ++b) for (int which = 0; which < 2; ++which) {
            reference(imgs[2 * b + which], rows[b][0], rows[b][1], rows[b][2], rows[b][3], (int)rows[b][4], P, swap, want.data());
            const float* got = (which ? gt : lq).data() + (size_t)b * 3 * P * P;
            for (size_t k = 0; k < want.size(); ++k) { ++total; if (memcmp(&got[k], &want[k], 4)) { if (bad < 5) printf("P %d b %d which %d k %zu got %g want %g (h %lld w %lld top %lld left %lld mode %lld)\n", P, b, which, k, got[k], want[k], rows[b][0], rows[b][1], rows[b][2], rows[b][3], rows[b][4]); ++bad; } }
        }
        for (auto p : imgs) free(p);
    }
    // empty rows: zeros
    { long long row[8] = {0, 0, 5, 5, 0, 0, 0, 0}; std::vector<float> lq(3 * 40 * 40, -1.f), gt(3 * 40 * 40, -1.f); launch(row, lq.data(), gt.data(), 1, 40, 1);
      for (float v : lq) if (v != 0.f) ++bad; for (float v : gt) if (v != 0.f) ++bad; }
    printf("%lld elements compared, %lld differ\n", total, bad);
    return bad != 0;
}
