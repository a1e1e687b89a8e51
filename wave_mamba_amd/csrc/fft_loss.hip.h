// fft_loss.hip.h - the FFT training loss (FFTLoss: the L1 mean between the stacked real / imaginary parts of rfft2(pred) and
// rfft2(target)) and its input gradients, for gfx950.
//
// Reference: basicsr/losses/losses.py:300-313 (FFTLoss, loss_weight 0.1 by train_wavemamba_uhdll.yml:102-104 `fft_opt`).
// rfft2 is linear, so the two spectra are never made: d = a - b is taken in fp32 FIRST and transformed once,
//   Y[k1, k2] = sum d[n1, n2] exp(-2 pi i (k1 n1 / H + k2 n2 / W)),  k2 < K = W / 2 + 1
//   out = sum(|Re Y| + |Im Y|) / M,  M = planes H K 2
//   ga[n1, n2] = gout / M * Re sum_{k1, k2 < K} s[k1, k2] exp(+2 pi i (k1 n1 / H + k2 n2 / W)),  s = sign(Re Y) + i sign(Im Y)
// (the half spectrum only: what autograd gives for the reference's composition), gb = -ga.  H and W: powers of two in [16, 1024].
//
// Every kernel works on a tile of FL_TILE = 4096 complex values in LDS: NB = 4096 / N sequences of length N, sequence b's element e
// at fl_at(e NB + b) - the sequences interleaved, so that the lanes of a wave walk across sequences first and a butterfly's four
// operands of all lanes lie in contiguous runs, whatever the stage's stride.  fl_at puts 4 unused values after every 16: the first
// stages write 16 lanes' values (ds_write_b64 services 16 lanes per cycle over 32 banks) at strides of 4 NB or 16 NB values, which
// without the gaps fall on one bank group for NB = 4 and 8 (H or W = 1024, 512).
// The transform is Stockham's (natural order in, natural order out, no bit reversal) in place: each thread holds its butterflies'
// operands in registers across a barrier (4 radix-4 butterflies per thread and stage; when log2 N is odd the first stage is radix 2).
// Twiddles: exp(-2 pi i j / 1024) from a table evaluated in double AT COMPILE TIME and rounded once (fl_cos / fl_sin below: a Taylor
// series on [0, pi / 4] and the octant symmetries); a stage reads entry r k 1024 / (Ns R) - no device sine or cosine anywhere.
//
// Forward, rows:     a tile holds NB pairs of rows, z = d[row 2p] + i d[row 2p + 1] (16-byte loads of a and b), one complex
//                    transform of length W, X0[k] = (Z[k] + conj Z[W - k]) / 2, X1[k] = (Z[k] - conj Z[W - k]) / 2i, k < K, to a
//                    workspace of planes H K complex values.
// Forward, columns:  a tile holds NB adjacent columns of that workspace (columns of all planes numbered through: plane K + k2), the
//                    transform of length H, |Re| + |Im| summed in double into the workgroup's slot, and for a gradient one byte per
//                    bin into the record: (sign Re + 1) | (sign Im + 1) << 2, the imaginary sign of the four self-conjugate bins
//                    (k1 in {0, H / 2}, k2 in {0, W / 2}) stored as 0: its derivative is zero and its value is rounding noise.
// Finish:            the slots added in a fixed order, out OVERWRITTEN: no atomics, nothing zeroed, two calls are bit-identical.
// Backward, columns: the signs of NB columns, the inverse transform of length H, to the workspace (the record stays as it was).
// Backward, rows:    Re(inverse transform of T) = inverse transform of T's Hermitian part: for a pair of rows with half spectra A, B
//                    U[k] = A[k] + i B[k], U[W - k] = conj A[k] + i conj B[k] (0 < k < W / 2), U[0] = 2 Re A[0] + 2 i Re B[0], the same
//                    at W / 2; one inverse transform of length W gives row 2p in the real and row 2p + 1 in the imaginary part, times
//                    gout / 2M (the product formed in double and rounded once).
#pragma once
#include <hip/hip_runtime.h>

#define FL_HD __host__ __device__ inline

namespace wm {

constexpr int FL_TILE = 4096, FL_THREADS = 256, FL_TW = 1024, FL_MIN = 16, FL_MAX = 1024;
constexpr int FL_LDS = FL_TILE + FL_TILE / 4;                  // with fl_at's gaps
static_assert(FL_TILE / FL_MAX >= 4 && FL_THREADS % (FL_TILE / FL_MAX) == 0 && FL_TILE / FL_MIN <= FL_THREADS,
              "a thread's items all belong to one sequence: b = tid mod NB");

struct alignas(8) FlC { float x, y; };

constexpr double fl_sin(double x) {                             // 0 <= x <= pi / 4: the series to x^25 (2e-22 there)
    double x2 = x * x, r = 1.0;
    for (int n = 25; n >= 3; n -= 2) r = 1.0 - x2 / (double)((n - 1) * n) * r;
    return x * r;
}
constexpr double fl_cos(double x) {
    double x2 = x * x, r = 1.0;
    for (int n = 24; n >= 2; n -= 2) r = 1.0 - x2 / (double)((n - 1) * n) * r;
    return r;
}

// w[j] = exp(-2 pi i j / FL_TW), each part the double value rounded once to float
struct FlTable {
    FlC w[FL_TW];
    constexpr FlTable() : w{} {
        for (int j = 0; j < FL_TW; ++j) {
            const int quad = j / (FL_TW / 4), r = j % (FL_TW / 4);
            const bool swap = r > FL_TW / 8;
            const double ang = 3.14159265358979323846 * (double)(swap ? FL_TW / 4 - r : r) / (double)(FL_TW / 2);
            const double c0 = swap ? fl_sin(ang) : fl_cos(ang), s0 = swap ? fl_cos(ang) : fl_sin(ang);
            const double c = quad == 0 ? c0 : quad == 1 ? -s0 : quad == 2 ? -c0 : s0;
            const double s = quad == 0 ? s0 : quad == 1 ? c0 : quad == 2 ? -s0 : -c0;
            w[j].x = (float)c;
            w[j].y = (float)-s;
        }
    }
};

struct FlGeom {
    int H, W, K, lH, lW;           // K = W / 2 + 1; lH = log2 H, lW = log2 W
    long long npairs, ncols;       // planes H / 2 pairs of rows; planes K columns
};

FL_HD int fl_at(int a) { return a + ((a >> 4) << 2); }

FL_HD FlC fl_mul(FlC a, FlC w) { return FlC{a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x}; }

// One Stockham stage of radix R on the tile, first half: the R operands of this thread's butterflies (item i = tid + it 256:
// sequence b = i mod NB, butterfly j = i / NB) read from buf, twiddled and combined into v.  Ns = the product of the radices before.
template <int R, bool INV>
FL_HD void fl_stage_load(const FlC* buf, const FlC* tw, int tid, int lN, int Ns, FlC (&v)[FL_TILE / R / FL_THREADS][R]) {
    constexpr int IT = FL_TILE / R / FL_THREADS;
    static_assert((R == 2 || R == 4) && FL_TILE == 1 << 12, "radix 2 or 4; log2 NB = 12 - lN");
    const int lNB = 12 - lN, NB = 1 << lNB, q = (1 << lN) / R, tstep = FL_TW / (Ns * R);
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int i = tid + it * FL_THREADS, b = i & (NB - 1), j = i >> lNB, k = j & (Ns - 1);
        FlC x[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            x[r] = buf[fl_at((j + r * q) * NB + b)];
            if (r > 0 && Ns > 1) {
                FlC w = tw[r * k * tstep];
                if (INV) w.y = -w.y;
                x[r] = fl_mul(x[r], w);
            }
        }
        if (R == 2) {
            v[it][0] = FlC{x[0].x + x[1].x, x[0].y + x[1].y};
            v[it][1] = FlC{x[0].x - x[1].x, x[0].y - x[1].y};
        } else {
            const FlC t0{x[0].x + x[2].x, x[0].y + x[2].y}, t1{x[0].x - x[2].x, x[0].y - x[2].y};
            const FlC t2{x[1].x + x[3].x, x[1].y + x[3].y}, t3{x[1].x - x[3].x, x[1].y - x[3].y};
            v[it][0] = FlC{t0.x + t2.x, t0.y + t2.y};
            v[it][2] = FlC{t0.x - t2.x, t0.y - t2.y};
            const FlC lo{t1.x + t3.y, t1.y - t3.x}, hi{t1.x - t3.y, t1.y + t3.x};       // t1 - i t3, t1 + i t3
            v[it][1] = INV ? hi : lo;
            v[it][R - 1] = INV ? lo : hi;
        }
    }
}

// second half, after a barrier: output r of butterfly j goes to element (j - k) R + k + r Ns
template <int R>
FL_HD void fl_stage_store(FlC* buf, int tid, int lN, int Ns, const FlC (&v)[FL_TILE / R / FL_THREADS][R]) {
    constexpr int IT = FL_TILE / R / FL_THREADS;
    const int lNB = 12 - lN, NB = 1 << lNB;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int i = tid + it * FL_THREADS, b = i & (NB - 1), j = i >> lNB, k = j & (Ns - 1);
        const int e0 = (j - k) * R + k;
#pragma unroll
        for (int r = 0; r < R; ++r) buf[fl_at((e0 + r * Ns) * NB + b)] = v[it][r];
    }
}

// ---- tile <-> memory, one item loop per phase (each FL_HD: the host statement of a kernel runs the same code thread by thread) --

// rows, forward: z = (a - b)[row 2p] + i (a - b)[row 2p + 1]; item = (pair b, group of 4 columns)
FL_HD void fl_rows_load_diff(const float* a, const float* b, const FlGeom& g, long long tile, int tid, FlC* buf) {
    const int lNB = 12 - g.lW, NB = 1 << lNB, sb = tid & (NB - 1);
    const long long p = tile * NB + sb;
    const bool live = p < g.npairs;
    const long long row = 2 * p * g.W;
    for (int i = tid; i < FL_TILE / 4; i += FL_THREADS) {
        const int e = 4 * (i >> lNB);
        float4 d0 = make_float4(0.f, 0.f, 0.f, 0.f), d1 = d0;
        if (live) {
            const float4 a0 = *reinterpret_cast<const float4*>(a + row + e), b0 = *reinterpret_cast<const float4*>(b + row + e);
            const float4 a1 = *reinterpret_cast<const float4*>(a + row + g.W + e), b1 = *reinterpret_cast<const float4*>(b + row + g.W + e);
            d0 = make_float4(a0.x - b0.x, a0.y - b0.y, a0.z - b0.z, a0.w - b0.w);
            d1 = make_float4(a1.x - b1.x, a1.y - b1.y, a1.z - b1.z, a1.w - b1.w);
        }
        buf[fl_at((e + 0) * NB + sb)] = FlC{d0.x, d1.x};
        buf[fl_at((e + 1) * NB + sb)] = FlC{d0.y, d1.y};
        buf[fl_at((e + 2) * NB + sb)] = FlC{d0.z, d1.z};
        buf[fl_at((e + 3) * NB + sb)] = FlC{d0.w, d1.w};
    }
}

// the (pair, k) items of a row tile, k < K: 8 adjacent k of one pair in adjacent lanes (64-byte runs in memory, one run in LDS)
struct FlRowItem { int b, k; bool live; };
FL_HD int fl_row_items(const FlGeom& g) { return (FL_TILE / g.W) * 8 * (g.K / 8 + 1); }
FL_HD FlRowItem fl_row_item(const FlGeom& g, int i) {
    const int lNB = 12 - g.lW, NB = 1 << lNB;
    FlRowItem it;
    it.b = (i >> 3) & (NB - 1);
    it.k = ((i >> (3 + lNB)) << 3) | (i & 7);
    it.live = it.k < g.K;
    return it;
}

// rows, forward: the two rows' half spectra out of the packed transform
FL_HD void fl_rows_store_spectra(const FlC* buf, const FlGeom& g, long long tile, int tid, FlC* mid) {
    const int NB = FL_TILE / g.W, n = fl_row_items(g);
    for (int i = tid; i < n; i += FL_THREADS) {
        const FlRowItem it = fl_row_item(g, i);
        const long long p = tile * NB + it.b;
        if (!it.live || p >= g.npairs) continue;
        const FlC z = buf[fl_at(it.k * NB + it.b)], m = buf[fl_at(((g.W - it.k) & (g.W - 1)) * NB + it.b)];
        mid[2 * p * g.K + it.k] = FlC{0.5f * (z.x + m.x), 0.5f * (z.y - m.y)};
        mid[(2 * p + 1) * g.K + it.k] = FlC{0.5f * (z.y + m.y), -0.5f * (z.x - m.x)};
    }
}

// rows, backward: the packed Hermitian parts of the two rows' half spectra (see the header)
FL_HD void fl_rows_load_hermitian(const FlC* mid, const FlGeom& g, long long tile, int tid, FlC* buf) {
    const int NB = FL_TILE / g.W, n = fl_row_items(g);
    for (int i = tid; i < n; i += FL_THREADS) {
        const FlRowItem it = fl_row_item(g, i);
        if (!it.live) continue;
        const long long p = tile * NB + it.b;
        FlC A{0.f, 0.f}, B{0.f, 0.f};
        if (p < g.npairs) {
            A = mid[2 * p * g.K + it.k];
            B = mid[(2 * p + 1) * g.K + it.k];
        }
        if (it.k == 0 || it.k == g.W / 2) {
            buf[fl_at(it.k * NB + it.b)] = FlC{2.0f * A.x, 2.0f * B.x};
        } else {
            buf[fl_at(it.k * NB + it.b)] = FlC{A.x - B.y, A.y + B.x};
            buf[fl_at((g.W - it.k) * NB + it.b)] = FlC{A.x + B.y, B.x - A.y};
        }
    }
}

// rows, backward: ga (and gb = -ga) = scale * the transform's real part (row 2p) and imaginary part (row 2p + 1)
FL_HD void fl_rows_store_grad(const FlC* buf, const FlGeom& g, long long tile, int tid, double scale, float* ga, float* gb) {
    const int lNB = 12 - g.lW, NB = 1 << lNB, sb = tid & (NB - 1);
    const long long p = tile * NB + sb;
    if (p >= g.npairs) return;
    const long long row = 2 * p * g.W;
    for (int i = tid; i < FL_TILE / 4; i += FL_THREADS) {
        const int e = 4 * (i >> lNB);
        FlC u[4];
        for (int c = 0; c < 4; ++c) u[c] = buf[fl_at((e + c) * NB + sb)];
        const float4 r0 = make_float4((float)(scale * (double)u[0].x), (float)(scale * (double)u[1].x), (float)(scale * (double)u[2].x),
                                      (float)(scale * (double)u[3].x));
        const float4 r1 = make_float4((float)(scale * (double)u[0].y), (float)(scale * (double)u[1].y), (float)(scale * (double)u[2].y),
                                      (float)(scale * (double)u[3].y));
        if (ga != nullptr) {
            *reinterpret_cast<float4*>(ga + row + e) = r0;
            *reinterpret_cast<float4*>(ga + row + g.W + e) = r1;
        }
        if (gb != nullptr) {
            *reinterpret_cast<float4*>(gb + row + e) = make_float4(-r0.x, -r0.y, -r0.z, -r0.w);
            *reinterpret_cast<float4*>(gb + row + g.W + e) = make_float4(-r1.x, -r1.y, -r1.z, -r1.w);
        }
    }
}

// a column tile's sequence of this thread: column c = tile NB + (tid mod NB) of planes K, at mid / record offset `at` + e K
struct FlCol { bool live; int k2; long long at; };
FL_HD FlCol fl_col(const FlGeom& g, long long tile, int tid) {
    const int NB = FL_TILE / g.H;
    const long long c = tile * NB + (tid & (NB - 1));
    FlCol o;
    o.live = c < g.ncols;
    const long long plane = c / g.K;
    o.k2 = (int)(c - plane * g.K);
    o.at = plane * g.H * g.K + o.k2;
    return o;
}

FL_HD void fl_cols_load(const FlC* mid, const FlGeom& g, long long tile, int tid, FlC* buf) {
    const int lNB = 12 - g.lH, NB = 1 << lNB;
    const FlCol c = fl_col(g, tile, tid);
    for (int i = tid; i < FL_TILE; i += FL_THREADS) {
        const int e = i >> lNB;
        buf[fl_at(e * NB + (tid & (NB - 1)))] = c.live ? mid[c.at + (long long)e * g.K] : FlC{0.f, 0.f};
    }
}

FL_HD void fl_cols_store(const FlC* buf, const FlGeom& g, long long tile, int tid, FlC* mid) {
    const int lNB = 12 - g.lH, NB = 1 << lNB;
    const FlCol c = fl_col(g, tile, tid);
    if (!c.live) return;
    for (int i = tid; i < FL_TILE; i += FL_THREADS) {
        const int e = i >> lNB;
        mid[c.at + (long long)e * g.K] = buf[fl_at(e * NB + (tid & (NB - 1)))];
    }
}

FL_HD float fl_sign(float v) { return (float)((v > 0.0f) - (v < 0.0f)); }

// columns, forward: this thread's share of sum(|Re| + |Im|), and the sign bytes where a record is kept
FL_HD double fl_cols_sum_signs(const FlC* buf, const FlGeom& g, long long tile, int tid, unsigned char* rec) {
    const int lNB = 12 - g.lH, NB = 1 << lNB;
    const FlCol c = fl_col(g, tile, tid);
    double s = 0.0;
    if (!c.live) return s;
    const bool edge = c.k2 == 0 || c.k2 == g.W / 2;
    for (int i = tid; i < FL_TILE; i += FL_THREADS) {
        const int e = i >> lNB;
        const FlC y = buf[fl_at(e * NB + (tid & (NB - 1)))];
        s += (double)(fabsf(y.x) + fabsf(y.y));
        if (rec != nullptr) {
            const int sr = (y.x > 0.0f) - (y.x < 0.0f);
            const int si = (edge && (e == 0 || e == g.H / 2)) ? 0 : (y.y > 0.0f) - (y.y < 0.0f);
            rec[c.at + (long long)e * g.K] = (unsigned char)((sr + 1) | ((si + 1) << 2));
        }
    }
    return s;
}

FL_HD void fl_cols_load_signs(const unsigned char* rec, const FlGeom& g, long long tile, int tid, FlC* buf) {
    const int lNB = 12 - g.lH, NB = 1 << lNB;
    const FlCol c = fl_col(g, tile, tid);
    for (int i = tid; i < FL_TILE; i += FL_THREADS) {
        const int e = i >> lNB;
        FlC s{0.f, 0.f};
        if (c.live) {
            const int code = rec[c.at + (long long)e * g.K];
            s = FlC{(float)((code & 3) - 1), (float)(((code >> 2) & 3) - 1)};
        }
        buf[fl_at(e * NB + (tid & (NB - 1)))] = s;
    }
}

#if defined(__HIPCC__)
static __device__ const FlTable FL_TWIDDLES{};

// The tile's NB transforms of length 2^lN, in place.  Barriers: the caller's writes to buf are fenced here; the result is fenced on return.
template <bool INV>
__device__ inline void fl_fft(FlC* buf, const FlC* tw, int lN) {
    const int tid = threadIdx.x, N = 1 << lN;
    __syncthreads();
    int Ns = 1;
    if (lN & 1) {
        FlC v[FL_TILE / 2 / FL_THREADS][2];
        fl_stage_load<2, INV>(buf, tw, tid, lN, 1, v);
        __syncthreads();
        fl_stage_store<2>(buf, tid, lN, 1, v);
        __syncthreads();
        Ns = 2;
    }
    for (; Ns < N; Ns *= 4) {
        FlC v[FL_TILE / 4 / FL_THREADS][4];
        fl_stage_load<4, INV>(buf, tw, tid, lN, Ns, v);
        __syncthreads();
        fl_stage_store<4>(buf, tid, lN, Ns, v);
        __syncthreads();
    }
}

__device__ inline void fl_table_to_lds(FlC* tw) {
    for (int i = threadIdx.x; i < FL_TW; i += FL_THREADS) tw[i] = FL_TWIDDLES.w[i];
}

// grid (row tiles), block 256
__global__ __launch_bounds__(FL_THREADS) void fft_l1_rows_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                      FlC* __restrict__ mid, FlGeom g) {
    __shared__ FlC buf[FL_LDS], tw[FL_TW];
    fl_table_to_lds(tw);
    fl_rows_load_diff(a, b, g, blockIdx.x, threadIdx.x, buf);
    fl_fft<false>(buf, tw, g.lW);
    fl_rows_store_spectra(buf, g, blockIdx.x, threadIdx.x, mid);
}

// grid (column tiles), block 256.  part[blockIdx.x] = the tile's sum of |Re Y| + |Im Y|; rec: the sign bytes, or nullptr
__global__ __launch_bounds__(FL_THREADS) void fft_l1_cols_fwd_kernel(const FlC* __restrict__ mid, unsigned char* __restrict__ rec,
                                                                      double* __restrict__ part, FlGeom g) {
    __shared__ FlC buf[FL_LDS], tw[FL_TW];
    __shared__ double red[FL_THREADS / 64];
    fl_table_to_lds(tw);
    fl_cols_load(mid, g, blockIdx.x, threadIdx.x, buf);
    fl_fft<false>(buf, tw, g.lH);
    double s = fl_cols_sum_signs(buf, g, blockIdx.x, threadIdx.x, rec);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// grid (1), block 256: out[0] = float(the slots added in a fixed order / m)
__global__ __launch_bounds__(FL_THREADS) void fft_l1_finish_kernel(const double* __restrict__ part, long long nparts, double m,
                                                                    float* __restrict__ out) {
    __shared__ double rs[FL_THREADS];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (long long i = tid; i < nparts; i += FL_THREADS) s += part[i];
    rs[tid] = s;
    __syncthreads();
    for (int w = FL_THREADS / 2; w >= 1; w >>= 1) {
        if (tid < w) rs[tid] += rs[tid + w];
        __syncthreads();
    }
    if (tid == 0) out[0] = (float)(rs[0] / m);
}

// grid (column tiles), block 256
__global__ __launch_bounds__(FL_THREADS) void fft_l1_cols_bwd_kernel(const unsigned char* __restrict__ rec, FlC* __restrict__ mid,
                                                                      FlGeom g) {
    __shared__ FlC buf[FL_LDS], tw[FL_TW];
    fl_table_to_lds(tw);
    fl_cols_load_signs(rec, g, blockIdx.x, threadIdx.x, buf);
    fl_fft<true>(buf, tw, g.lH);
    fl_cols_store(buf, g, blockIdx.x, threadIdx.x, mid);
}

// grid (row tiles), block 256.  half_inv_m = 1 / 2M
__global__ __launch_bounds__(FL_THREADS) void fft_l1_rows_bwd_kernel(const FlC* __restrict__ mid, const float* __restrict__ gout,
                                                                      float* __restrict__ ga, float* __restrict__ gb, FlGeom g,
                                                                      double half_inv_m) {
    __shared__ FlC buf[FL_LDS], tw[FL_TW];
    fl_table_to_lds(tw);
    fl_rows_load_hermitian(mid, g, blockIdx.x, threadIdx.x, buf);
    fl_fft<true>(buf, tw, g.lW);
    fl_rows_store_grad(buf, g, blockIdx.x, threadIdx.x, (double)gout[0] * half_inv_m, ga, gb);
}
#endif  // __HIPCC__

}  // namespace wm
