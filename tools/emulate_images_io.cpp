// emulate_images_io.cpp - images_pre_kernel and images_post_kernel (csrc/images_io.hip.h) run on the HOST under AddressSanitizer /
// UBSan, against the definition written out directly (the index table of data_augmentation, scattered, not inverted).  The kernel
// header is compiled for the CPU through tools/hip_host_shim, as tools/emulate_patch_batch.cpp does; every image and every fp32
// tensor sits in a heap block of exactly its size, so an access outside one is an ASan report.  Cases: shapes 1 x 1, 5 x 7,
// 33 x 65 and 65 x 33 at window 32 (pads of 31, the largest legal) and 45 x 70 at window 8 (crosses the 32 x 32 tile both ways
// with a remainder), all eight modes, both channel orders, k = 1 and the two-tensor k = 8 ensemble, fp32 values below 0, above 1
// and on exact halves of a level; table rows the kernels must refuse (a padding that reaches the image's size, an image that does
// not fit, a source index outside its tensor, a source too small, k = 9): zeros / untouched.  Prints the number of elements
// compared and of differences; exit status 1 on any.  No GPU, about two minutes (thread creation dominates).
//
//   cd tools && g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I hip_host_shim emulate_images_io.cpp -o emulate_images_io \
//       -lpthread && ./emulate_images_io
#include <cmath>
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
#include "../wave_mamba_amd/csrc/images_io.hip.h"
using namespace wm;

static long long bad = 0, total = 0;
static const int KEEP[4] = {0, 1, 4, 5}, TURN[4] = {2, 3, 6, 7};

// out[i, j] = A[r, c] of an (h, w) image A
static void source_of(int mode, int h, int w, int i, int j, int& r, int& c) {
    switch (mode) {
        case 0: r = i; c = j; break;             case 1: r = h - 1 - i; c = j; break;
        case 2: r = j; c = w - 1 - i; break;     case 3: r = j; c = i; break;
        case 4: r = h - 1 - i; c = w - 1 - j; break; case 5: r = i; c = w - 1 - j; break;
        case 6: r = h - 1 - j; c = i; break;     default: r = h - 1 - j; c = w - 1 - i;
    }
}
static bool turns(int mode) { return mode == 2 || mode == 3 || mode == 6 || mode == 7; }
static int padded(int n, int window) { return n + (window - n % window) % window; }
static int refl(int y, int n) { return y < n ? y : 2 * (n - 1) - y; }

template <typename F>
static void run_blocks(int gx, int gy, int gz, F kernel) {
    for (int z = 0; z < gz; ++z) for (int y = 0; y < gy; ++y) for (int x = 0; x < gx; ++x) {
        blockIdx.x = x; blockIdx.y = y; blockIdx.z = z;
        std::vector<std::thread> th;
        for (int t = 0; t < 256; ++t) th.emplace_back([=] { threadIdx.x = t; kernel(); });
        for (auto& a : th) a.join();
    }
}
static void launch_pre(const long long* table, float* out, int N, int Hp, int Wp, int swap) {
    run_blocks((Wp + 31) / 32, (Hp + 31) / 32, N, [=] { images_pre_kernel(table, out, Hp, Wp, swap); });
}
static void launch_post(const long long* table, IoSource s0, IoSource s1, int rows, int hmax, int wmax, int swap) {
    run_blocks((wmax + 31) / 32, (hmax + 31) / 32, rows, [=] { images_post_kernel(table, s0, s1, swap); });
}
static void differ(const char* what, long long k) { if (bad++ < 8) printf("%s: element %lld differs\n", what, k); }

static float* exact_floats(size_t n) { return (float*)malloc(n * sizeof(float)); }

// the pre kernel: every mode of an (h, w) image in one launch per padded shape
static void check_pre(int h, int w, int window, int swap, std::mt19937& rng) {
    uint8_t* img = (uint8_t*)malloc((size_t)3 * h * w);                  // exact size: ASan sees any read outside
    for (long long k = 0; k < 3LL * h * w; ++k) img[k] = rng();
    for (const int* modes : {KEEP, TURN}) {
        const int ht = turns(modes[0]) ? w : h, wt = turns(modes[0]) ? h : w, Hp = padded(ht, window), Wp = padded(wt, window);
        std::vector<long long> table;
        for (int n = 0; n < 4; ++n) { long long row[4] = {(long long)(uintptr_t)img, h, w, modes[n] + 8 * (n & 1)}; table.insert(table.end(), row, row + 4); }
        const size_t count = (size_t)4 * 3 * Hp * Wp;
        float* out = exact_floats(count);
        for (size_t k = 0; k < count; ++k) out[k] = -1.f;
        launch_pre(table.data(), out, 4, Hp, Wp, swap);
        for (int n = 0; n < 4; ++n) for (int ch = 0; ch < 3; ++ch) for (int i = 0; i < Hp; ++i) for (int j = 0; j < Wp; ++j) {
            int r, c;
            source_of(modes[n], h, w, refl(i, ht), refl(j, wt), r, c);
            const float want = (float)img[((long long)r * w + c) * 3 + (swap ? 2 - ch : ch)] / 255.0f;
            const long long k = (((long long)n * 3 + ch) * Hp + i) * Wp + j;
            ++total;
            if (memcmp(&out[k], &want, 4)) differ("pre", k);
        }
        free(out);
    }
    free(img);
}

// the post kernel: k = 1 rows of every mode, and the k = 8 ensemble over two tensors, for `copies` destinations of (h, w)
static void check_post(int h, int w, int window, int swap, int copies, std::mt19937& rng) {
    const int Hp0 = padded(h, window), Wp0 = padded(w, window), Hp1 = padded(w, window), Wp1 = padded(h, window);
    const int N0 = 4 * copies, N1 = 4 * copies;
    const size_t n0 = (size_t)N0 * 3 * Hp0 * Wp0, n1 = (size_t)N1 * 3 * Hp1 * Wp1;
    float* t0 = exact_floats(n0), *t1 = exact_floats(n1);
    auto fill = [&](float* p, size_t n) {
        for (size_t k = 0; k < n; ++k) {
            const unsigned u = rng();
            switch (u % 8) {
                case 0: p[k] = ((u >> 8) % 255 + 0.5f) / 255.0f; break;                 // a half level (after * 255: to even)
                case 1: p[k] = -0.25f * ((u >> 8) % 5); break;
                case 2: p[k] = 1.0f + 0.25f * ((u >> 8) % 5); break;
                default: p[k] = ((u >> 8) % 100000) / 100000.0f - 0.1f * (u % 3 == 0);
            }
        }
    };
    fill(t0, n0); fill(t1, n1);
    const IoSource s0{t0, N0, Hp0, Wp0}, s1{t1, N1, Hp1, Wp1};
    std::vector<std::vector<long long>> rows;                                       // per destination: the source words
    for (int b = 0; b < copies; ++b) {
        std::vector<long long> all(8);
        for (int at = 0; at < 4; ++at) {
            all[KEEP[at]] = KEEP[at] | 0 << 8 | (long long)(4 * b + at) << 16;
            all[TURN[at]] = TURN[at] | 1 << 8 | (long long)(4 * b + at) << 16;
        }
        rows.push_back(all);
        for (int m = 0; m < 8; ++m) rows.push_back({all[m]});
    }
    std::vector<uint8_t*> dst;
    std::vector<long long> table;
    for (auto& words : rows) {
        uint8_t* d = (uint8_t*)malloc((size_t)3 * h * w);
        memset(d, 0xAB, (size_t)3 * h * w);
        dst.push_back(d);
        long long row[IO_POST_WORDS] = {(long long)(uintptr_t)d, h, w, (long long)words.size()};
        for (size_t s = 0; s < words.size(); ++s) row[4 + s] = words[s];
        table.insert(table.end(), row, row + IO_POST_WORDS);
    }
    launch_post(table.data(), s0, s1, (int)rows.size(), h, w, swap);
    std::vector<float> sum((size_t)3 * h * w), y((size_t)3 * h * w);
    for (size_t rix = 0; rix < rows.size(); ++rix) {
        bool first = true;
        for (long long word : rows[rix]) {
            const int mode = word & 7, which = (word >> 8) & 1; const long long index = word >> 16;
            const IoSource& src = which ? s1 : s0;
            const int ht = turns(mode) ? w : h, wt = turns(mode) ? h : w;
            for (int ch = 0; ch < 3; ++ch) for (int i = 0; i < ht; ++i) for (int j = 0; j < wt; ++j) {
                int r, c;
                source_of(mode, h, w, i, j, r, c);                                  // the network saw A[r, c] at (i, j): it goes back to (r, c)
                y[((size_t)ch * h + r) * w + c] = src.base[((index * 3 + ch) * src.Hp + i) * src.Wp + j];
            }
            for (size_t k = 0; k < sum.size(); ++k) sum[k] = first ? y[k] : sum[k] + y[k];
            first = false;
        }
        const float inv = 1.0f / (float)rows[rix].size();
        for (int r = 0; r < h; ++r) for (int c = 0; c < w; ++c) for (int ch = 0; ch < 3; ++ch) {
            volatile float mean = sum[((size_t)ch * h + r) * w + c] * inv;
            const float v = fminf(fmaxf(mean, 0.0f), 1.0f);
            const uint8_t want = (uint8_t)rintf(v * 255.0f);
            ++total;
            if (dst[rix][((size_t)r * w + c) * 3 + (swap ? 2 - ch : ch)] != want) differ("post", ((long long)r * w + c) * 3 + ch);
        }
    }
    for (auto d : dst) free(d);
    free(t0); free(t1);
}

// rows the kernels must refuse
static void check_refusals() {
    uint8_t* img = (uint8_t*)malloc(3 * 3 * 40);
    memset(img, 7, 3 * 3 * 40);
    // 3 rows padded to 8 (pad 5 >= 3); an image larger than the launch's shape; no image; a turned image that does not fit
    long long pre[4][4] = {{(long long)(uintptr_t)img, 3, 40, 0}, {(long long)(uintptr_t)img, 20, 6, 0}, {0, 8, 40, 0}, {(long long)(uintptr_t)img, 3, 40, 2}};
    float* out = exact_floats((size_t)4 * 3 * 8 * 40);
    for (size_t k = 0; k < (size_t)4 * 3 * 8 * 40; ++k) out[k] = -1.f;
    launch_pre(&pre[0][0], out, 4, 8, 40, 1);
    for (size_t k = 0; k < (size_t)4 * 3 * 8 * 40; ++k) { ++total; if (out[k] != 0.f) differ("refused pre row", (long long)k); }
    free(out);
    float* t0 = exact_floats((size_t)2 * 3 * 8 * 40);
    for (size_t k = 0; k < (size_t)2 * 3 * 8 * 40; ++k) t0[k] = 0.5f;
    uint8_t* d = (uint8_t*)malloc(3 * 8 * 40);
    memset(d, 0xAB, 3 * 8 * 40);
    const long long D = (long long)(uintptr_t)d;
    // index outside the tensor; a second tensor that is not there; a destination larger than the source; a turned source that does
    // not fit; k = 9; k = 0; no destination
    long long post[7][IO_POST_WORDS] = {{D, 8, 40, 1, 0 | 2LL << 16}, {D, 8, 40, 1, 0 | 1 << 8}, {D, 9, 40, 1, 0}, {D, 8, 40, 1, 2},
                                        {D, 8, 40, 9, 0, 0, 0, 0, 0, 0, 0, 0}, {D, 8, 40, 0}, {0, 8, 40, 1, 0}};
    launch_post(&post[0][0], IoSource{t0, 2, 8, 40}, IoSource{nullptr, 0, 0, 0}, 7, 9, 40, 1);
    for (int k = 0; k < 3 * 8 * 40; ++k) { ++total; if (d[k] != 0xAB) differ("refused post row", k); }
    free(d); free(t0); free(img);
}

int main() {
    pthread_barrier_init(&bar, nullptr, 256);
    std::mt19937 rng(1);
    const int cases[5][3] = {{1, 1, 1}, {5, 7, 1}, {33, 65, 32}, {65, 33, 32}, {45, 70, 8}};
    for (auto& cs : cases) for (int swap = 0; swap < 2; ++swap) {
        check_pre(cs[0], cs[1], cs[2], swap, rng);
        check_post(cs[0], cs[1], cs[2], swap, cs[0] == 5 ? 2 : 1, rng);
    }
    check_refusals();
    printf("%lld elements compared, %lld differ\n", total, bad);
    return bad != 0;
}
