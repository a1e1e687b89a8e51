// emulate_fft_loss.hip - the kernels of csrc/fft_loss.hip.h run on the HOST under AddressSanitizer / UBSan against a float64 DFT.
// The tile code of that header is __host__ __device__ functions of (tile, thread); a kernel calls them between barriers, this
// program calls them thread after thread, phase by phase, on heap buffers of exactly the sizes the library asks its caller for:
// an index outside the tile, the workspace, the record or an image is a sanitizer report.  It also holds the compile-time twiddle
// table to libm's and checks value, gradient and gb = -ga for every transform length, ragged tiles and several planes.  No GPU.
//
//   cd tools && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined emulate_fft_loss.hip \
//       -o emulate_fft_loss && ./emulate_fft_loss
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <complex>
#include "../wave_mamba_amd/csrc/fft_loss.hip.h"
using namespace wm;
typedef std::complex<double> cd;

static FlTable T;

template <bool INV> void host_fft(FlC* buf, int lN) {
    const int N = 1 << lN;
    int Ns = 1;
    if (lN & 1) {
        std::vector<FlC> v(FL_THREADS * (FL_TILE / 2 / FL_THREADS) * 2);
        typedef FlC V2[FL_TILE / 2 / FL_THREADS][2];
        for (int t = 0; t < FL_THREADS; ++t) fl_stage_load<2, INV>(buf, T.w, t, lN, 1, *(V2*)&v[t * (FL_TILE / 2 / FL_THREADS) * 2]);
        for (int t = 0; t < FL_THREADS; ++t) fl_stage_store<2>(buf, t, lN, 1, *(V2*)&v[t * (FL_TILE / 2 / FL_THREADS) * 2]);
        Ns = 2;
    }
    for (; Ns < N; Ns *= 4) {
        std::vector<FlC> v(FL_THREADS * (FL_TILE / 4 / FL_THREADS) * 4);
        typedef FlC V4[FL_TILE / 4 / FL_THREADS][4];
        for (int t = 0; t < FL_THREADS; ++t) fl_stage_load<4, INV>(buf, T.w, t, lN, Ns, *(V4*)&v[t * (FL_TILE / 4 / FL_THREADS) * 4]);
        for (int t = 0; t < FL_THREADS; ++t) fl_stage_store<4>(buf, t, lN, Ns, *(V4*)&v[t * (FL_TILE / 4 / FL_THREADS) * 4]);
    }
}

static int lg(int n) { int l = 0; while ((1 << l) < n) ++l; return l; }

int run(int planes, int H, int W) {
    FlGeom g; g.H = H; g.W = W; g.K = W / 2 + 1; g.lH = lg(H); g.lW = lg(W);
    g.npairs = (long long)planes * H / 2; g.ncols = (long long)planes * g.K;
    const int nbr = FL_TILE / W, nbc = FL_TILE / H;
    const long long rt = (g.npairs + nbr - 1) / nbr, ct = (g.ncols + nbc - 1) / nbc, bins = (long long)planes * H * g.K;
    const long long n = (long long)planes * H * W;
    // exact-size heap buffers: the address sanitizer sees any index past the end
    std::vector<float> a(n), b(n), ga(n), gb(n);
    for (long long i = 0; i < n; ++i) { a[i] = (float)(rand() / (double)RAND_MAX); b[i] = a[i] + 0.05f * ((float)(rand() / (double)RAND_MAX) - 0.5f); }
    std::vector<FlC> mid(bins), mid2(bins);
    std::vector<unsigned char> rec(bins);
    std::vector<FlC> buf(FL_LDS);
    double sum = 0;
    for (long long t = 0; t < rt; ++t) {
        for (int tid = 0; tid < FL_THREADS; ++tid) fl_rows_load_diff(a.data(), b.data(), g, t, tid, buf.data());
        host_fft<false>(buf.data(), g.lW);
        for (int tid = 0; tid < FL_THREADS; ++tid) fl_rows_store_spectra(buf.data(), g, t, tid, mid.data());
    }
    for (long long t = 0; t < ct; ++t) {
        for (int tid = 0; tid < FL_THREADS; ++tid) fl_cols_load(mid.data(), g, t, tid, buf.data());
        host_fft<false>(buf.data(), g.lH);
        for (int tid = 0; tid < FL_THREADS; ++tid) sum += fl_cols_sum_signs(buf.data(), g, t, tid, rec.data());
    }
    const double M = 2.0 * bins, val = sum / M;
    for (long long t = 0; t < ct; ++t) {
        for (int tid = 0; tid < FL_THREADS; ++tid) fl_cols_load_signs(rec.data(), g, t, tid, buf.data());
        host_fft<true>(buf.data(), g.lH);
        for (int tid = 0; tid < FL_THREADS; ++tid) fl_cols_store(buf.data(), g, t, tid, mid2.data());
    }
    for (long long t = 0; t < rt; ++t) {
        for (int tid = 0; tid < FL_THREADS; ++tid) fl_rows_load_hermitian(mid2.data(), g, t, tid, buf.data());
        host_fft<true>(buf.data(), g.lW);
        for (int tid = 0; tid < FL_THREADS; ++tid) fl_rows_store_grad(buf.data(), g, t, tid, 1.0 * (0.5 / M), ga.data(), gb.data());
    }
    // truth in double: the separable DFT written out
    double vref = 0, gerr = 0, gmax = 0, minmargin = 1e30, ymax = 0;
    const double PI = 3.14159265358979323846;
    std::vector<cd> wH(H), wW(W);
    for (int i = 0; i < H; ++i) wH[i] = std::polar(1.0, -2 * PI * i / H);
    for (int i = 0; i < W; ++i) wW[i] = std::polar(1.0, -2 * PI * i / W);
    std::vector<double> gtruth(n);
    for (int p = 0; p < planes; ++p) {
        std::vector<cd> R((size_t)H * g.K), Y((size_t)H * g.K), S((size_t)H * g.K), Tm((size_t)H * g.K);
        for (int y = 0; y < H; ++y) for (int k = 0; k < g.K; ++k) {
            cd s = 0; for (int x = 0; x < W; ++x) s += (double)(a[(p * (long long)H + y) * W + x] - b[(p * (long long)H + y) * W + x]) * wW[(k * x) % W];
            R[y * g.K + k] = s; }
        for (int k1 = 0; k1 < H; ++k1) for (int k = 0; k < g.K; ++k) {
            cd s = 0; for (int y = 0; y < H; ++y) s += R[y * g.K + k] * wH[(k1 * y) % H];
            Y[k1 * g.K + k] = s; vref += fabs(s.real()) + fabs(s.imag());
            const bool self = (k1 == 0 || k1 == H / 2) && (k == 0 || k == W / 2);
            ymax = std::max(ymax, std::abs(s));
            minmargin = std::min(minmargin, fabs(s.real())); if (!self) minmargin = std::min(minmargin, fabs(s.imag()));
            auto sg = [](double v) { return (double)((v > 0) - (v < 0)); };
            S[k1 * g.K + k] = cd(sg(s.real()), self ? 0.0 : sg(s.imag())); }
        for (int y = 0; y < H; ++y) for (int k = 0; k < g.K; ++k) {
            cd s = 0; for (int k1 = 0; k1 < H; ++k1) s += S[k1 * g.K + k] * std::conj(wH[(k1 * y) % H]);
            Tm[y * g.K + k] = s; }
        for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
            cd s = 0; for (int k = 0; k < g.K; ++k) s += Tm[y * g.K + k] * std::conj(wW[(k * x) % W]);
            gtruth[(p * (long long)H + y) * W + x] = s.real() / M; }
    }
    vref /= M;
    for (long long i = 0; i < n; ++i) {
        gerr = std::max(gerr, fabs(ga[i] - gtruth[i])); gmax = std::max(gmax, fabs(gtruth[i]));
        if (gb[i] != -ga[i]) { printf("gb != -ga at %lld\n", i); return 1; }
    }
    printf("%d x %d x %d: value %.9g truth %.9g rel %.2e | grad max err / max %.2e | margin %.2e\n", planes, H, W, val, vref,
           fabs(val - vref) / vref, gerr / gmax, minmargin / ymax);
    return !(fabs(val - vref) / vref < 1e-5 && gerr / gmax < 1e-5);      // fp32 transforms: 2e-7 measured; a wrong index is O(1)
}

int main() {
    int bad = 0;
    for (int j = 0; j < FL_TW; ++j) {
        const double ang = 2 * 3.14159265358979323846 * j / FL_TW;
        // (libm's sine of its rounded pi is 1.2e-16, the table's is 0: an absolute floor of 2e-16)
        if (fabs(T.w[j].x - cos(ang)) > 2e-16 + 6e-8 * fabs(cos(ang)) || fabs(T.w[j].y + sin(ang)) > 2e-16 + 6e-8 * fabs(sin(ang))) ++bad;
    }
    printf("twiddles beyond half an ulp of libm's: %d\n", bad);
    int rc = bad != 0;
    rc |= run(3, 16, 16);
    rc |= run(1, 16, 32);
    rc |= run(1, 32, 16);
    rc |= run(2, 64, 128);
    rc |= run(1, 128, 64);
    rc |= run(1, 256, 16);
    rc |= run(1, 16, 1024);
    rc |= run(1, 1024, 16);
    rc |= run(5, 16, 16);
    printf(rc ? "FAILED\n" : "ok\n");
    return rc;
}
