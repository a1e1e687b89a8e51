// images_io.hip.h - the caller's I/O step around the network (imageio.hip.h) for N images per launch, driven by DEVICE tables: a dihedral
// mode per image on the way in, the inverse mode and a group average on the way out.  Three uses, one pair of kernels:
//
//   batches         N images of one shape, mode 0, one source per destination
//   self-ensemble   the eight flips / rotations of one image (data_augmentation, transforms.py:223-268) as two batches of four - modes
//                   0, 1, 4, 5 keep the shape, modes 2, 3, 6, 7 transpose it - and the mean of the eight results turned back
//   graphs          the tables and every buffer they name are allocated before a capture; the launches hold no pointer that moves
//
// With A the (h, w) image and out the transformed one, out[i, j] = A[r, c] (the table of patch_batch.hip.h, for a non-square A):
//
//   mode   0       1          2          3       4              5          6          7
//   r      i       h-1-i      j          j       h-1-i          i          h-1-j      h-1-j
//   c      j       j          w-1-i      i       w-1-j          w-1-j      i          w-1-i
//
// out is (h, w) for modes 0, 1, 4, 5 and (w, h) for the others.  The inverse of a mode is a mode (2 <-> 6, the rest their own), but the
// kernels never need it by name: both directions index with the one table above.
//
// pre:  out[n] (3, Hp, Wp) = reflect_pad(chw(mode(A)) / 255) - the padding FOLLOWS the transform (check_image_size(aug(img)):
//       bottom / right of the transformed image), so a padded index is first reflected into the transformed shape, then turned.
//       One workgroup forms one 32 x 32 tile of one output image.  The transformed indices a tile needs are a contiguous interval on
//       each axis (a reflected interval is one, and so is an interval that straddles the edge), so the tile is a rectangle of at most
//       32 x 32 pixels of A: it is staged in LDS as bytes, every row read from memory as one run of consecutive bytes by consecutive
//       lanes whatever the mode; the turn, the mirrors and the reflection happen in the LDS read, and every fp32 plane row leaves as
//       32 consecutive floats.  LDS rows are 100 bytes = 25 dwords apart: odd, so the 32 lanes of a transposing read (one staged row
//       each) fall on 32 distinct banks.
//
// post: dst (h, w, 3) uint8 = hwc(rint(clamp(mean, 0, 1) * 255)), mean = (((y_0 + y_1) + y_2) + ...) * (1 / k) in fp32, y_s = source s
//       cropped to its transformed shape and turned back.  One workgroup forms one 32 x 32 tile of one destination.  A shape-keeping
//       source is read straight from memory (rows of consecutive floats, forwards or backwards); a transposing source goes through a
//       32 x 33 fp32 LDS tile per plane - rows of consecutive floats in, columns out, 33 being odd.  The sum runs in the table's order.
//       With k = 1 and mode 0 this is image_post_kernel's arithmetic: 1 / 1 is exact.
//
// The host cannot check a device table at launch time (ops.images_io_table checks what it writes): a row that names no image, an
// image that does not fit the launch's (Hp, Wp), a padding that reaches the image's size, a source index outside its tensor or a
// source too small for the destination is written as zeros (pre) or left unwritten (post) - it never indexes out of range.  The
// pointers themselves are the caller's responsibility.  No atomics, nothing zeroed first: both launches capture into a graph.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wm {

constexpr int IO_TILE = 32;
constexpr int IO_PITCH = 100;                                       // bytes per staged row: 96 of pixels, rounded up to an odd dword count
constexpr int IO_PRE_WORDS = 4;                                     // int64 per pre row: {image, h, w, mode}
constexpr int IO_MAX_SOURCES = 8;
constexpr int IO_POST_WORDS = 4 + IO_MAX_SOURCES;                   // int64 per post row: {image, h, w, k, k x source word}
// a source word: mode | which tensor << 8 | image index << 16

struct IoMode {
    bool turn, flip_r, flip_c;
};
__device__ __forceinline__ IoMode io_mode(int mode) {
    IoMode m;
    m.turn = (mode >> 1) & 1;                                        // modes 2, 3, 6, 7: r comes from j, c from i
    m.flip_r = m.turn ? mode >= 6 : (mode == 1 || mode == 4);
    m.flip_c = m.turn ? (mode == 2 || mode == 7) : (mode == 4 || mode == 5);
    return m;
}

// one fp32 source tensor of the post kernel: (N, 3, Hp, Wp), contiguous
struct IoSource {
    const float* base;
    int N, Hp, Wp;
};

// F.pad(..., 'reflect') at the far end of an axis of n elements (pad < n)
__device__ __forceinline__ int io_reflect(int y, int n) { return y < n ? y : 2 * (n - 1) - y; }

// the interval [lo, lo + count) of io_reflect(y, n) over y in [y0, y0 + len)
__device__ __forceinline__ void io_reflect_range(int y0, int len, int n, int& lo, int& count) {
    const int a = io_reflect(y0, n), b = io_reflect(y0 + len - 1, n);
    const int hi = (y0 <= n - 1 && n - 1 <= y0 + len - 1) ? n - 1 : max(a, b);
    lo = min(a, b);
    count = hi - lo + 1;
}

// grid (ceil(Wp / 32), ceil(Hp / 32), N), block (256)
__global__ __launch_bounds__(256) void images_pre_kernel(const long long* __restrict__ table, float* __restrict__ out, int Hp, int Wp,
                                                         int swap_rb) {
    __shared__ uint32_t s_words[IO_TILE * IO_PITCH / 4];
    uint8_t* const tile8 = reinterpret_cast<uint8_t*>(s_words);

    const int t = threadIdx.x, n = blockIdx.z;
    const int i0 = blockIdx.y * IO_TILE, j0 = blockIdx.x * IO_TILE;
    const int th = min(IO_TILE, Hp - i0), tw = min(IO_TILE, Wp - j0);

    const long long* row = table + (long long)n * IO_PRE_WORDS;
    const uint8_t* img = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(row[0]));
    const long long h64 = row[1], w64 = row[2];
    const IoMode m = io_mode((int)(row[3] & 7));
    const long long ht64 = m.turn ? w64 : h64, wt64 = m.turn ? h64 : w64;            // the transformed shape
    const bool empty = img == nullptr || h64 < 1 || w64 < 1 || ht64 > Hp || wt64 > Wp || Hp - ht64 >= ht64 || Wp - wt64 >= wt64;
    const int h = empty ? 1 : (int)h64, w = empty ? 1 : (int)w64;
    const int ht = m.turn ? w : h, wt = m.turn ? h : w;

    // the rectangle [r0, r0 + nr) x [c0, c0 + nc) of A that this tile shows
    int ta, nth, tb, ntw;
    io_reflect_range(i0, th, ht, ta, nth);
    io_reflect_range(j0, tw, wt, tb, ntw);
    const int pa = m.turn ? tb : ta, nr = m.turn ? ntw : nth;
    const int ca = m.turn ? ta : tb, nc = m.turn ? nth : ntw;
    const int r0 = m.flip_r ? h - pa - nr : pa, c0 = m.flip_c ? w - ca - nc : ca;

    if (!empty) {
        const int len = 3 * nc;
        for (int item = t; item < nr * (3 * IO_TILE); item += 256) {
            const int rr = item / (3 * IO_TILE), k = item % (3 * IO_TILE);
            if (k < len) tile8[rr * IO_PITCH + k] = img[((long long)(r0 + rr) * w + c0) * 3 + k];
        }
    }
    __syncthreads();

    const long long plane = (long long)Hp * Wp;
    float* const o = out + (long long)n * 3 * plane;
    const int lj = t & 31;
    for (int li = t >> 5; li < th; li += 8) {
        if (lj >= tw) continue;
        float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
        if (!empty) {
            const int ti = io_reflect(i0 + li, ht), tj = io_reflect(j0 + lj, wt);
            const int pr = m.turn ? tj : ti, pc = m.turn ? ti : tj;
            const int rr = (m.flip_r ? h - 1 - pr : pr) - r0, cc = (m.flip_c ? w - 1 - pc : pc) - c0;
            const uint8_t* p = tile8 + rr * IO_PITCH + 3 * cc;
            v0 = (float)p[0] / 255.0f; v1 = (float)p[1] / 255.0f; v2 = (float)p[2] / 255.0f;
        }
        const long long at = (long long)(i0 + li) * Wp + j0 + lj;
        o[at] = swap_rb ? v2 : v0;
        o[plane + at] = v1;
        o[2 * plane + at] = swap_rb ? v0 : v2;
    }
}

// grid (ceil(w_max / 32), ceil(h_max / 32), rows), block (256)
__global__ __launch_bounds__(256) void images_post_kernel(const long long* __restrict__ table, IoSource s0, IoSource s1, int swap_rb) {
    __shared__ float s_tile[3][IO_TILE][IO_TILE + 1];

    const int t = threadIdx.x;
    const long long* row = table + (long long)blockIdx.z * IO_POST_WORDS;
    uint8_t* const dst = reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(row[0]));
    const long long h64 = row[1], w64 = row[2], k64 = row[3];
    if (dst == nullptr || h64 < 1 || w64 < 1 || h64 > 0x7fffffffLL || w64 > 0x7fffffffLL || k64 < 1 || k64 > IO_MAX_SOURCES) return;
    const int h = (int)h64, w = (int)w64, k = (int)k64;
    const int r0 = blockIdx.y * IO_TILE, c0 = blockIdx.x * IO_TILE;
    if (r0 >= h || c0 >= w) return;                                  // a launch is sized by its largest destination
    const int th = min(IO_TILE, h - r0), tw = min(IO_TILE, w - c0);

    // every source must hold the destination's transformed shape (the same in all threads: the workgroup leaves as one)
    for (int s = 0; s < k; ++s) {
        const long long word = row[4 + s], index = word >> 16;
        const IoSource src = ((word >> 8) & 1) ? s1 : s0;
        const bool turn = (word >> 1) & 1;
        if (src.base == nullptr || index < 0 || index >= src.N || (turn ? w : h) > src.Hp || (turn ? h : w) > src.Wp) return;
    }

    const int lc = t & 31, lr = t >> 5;                              // this thread's pixels: (r0 + lr + 8 q, c0 + lc), q = 0 .. 3
    const bool col_ok = lc < tw;
    float acc[4][3];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q][0] = acc[q][1] = acc[q][2] = 0.0f;

    for (int s = 0; s < k; ++s) {
        const long long word = row[4 + s];
        const IoSource src = ((word >> 8) & 1) ? s1 : s0;
        const IoMode m = io_mode((int)(word & 7));
        const long long plane = (long long)src.Hp * src.Wp;
        const float* const base = src.base + (word >> 16) * 3 * plane;
        if (!m.turn) {
            // dst[r, c] = y[i, j] with i = r or h-1-r, j = c or w-1-c
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int li = lr + 8 * q;
                if (li < th && col_ok) {
                    const int r = r0 + li, c = c0 + lc;
                    const long long at = (long long)(m.flip_r ? h - 1 - r : r) * src.Wp + (m.flip_c ? w - 1 - c : c);
                    acc[q][0] += base[at]; acc[q][1] += base[plane + at]; acc[q][2] += base[2 * plane + at];
                }
            }
        } else {
            // dst[r, c] = y[i, j] with i = c or w-1-c, j = r or h-1-r: the tile of y has tw rows [ia, ia + tw) and th columns [ja, ja + th)
            const int ia = m.flip_c ? w - c0 - tw : c0, ja = m.flip_r ? h - r0 - th : r0;
            __syncthreads();                                         // the previous source's tile has been read
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int li = lr + 8 * q;
                if (li < tw && lc < th) {
                    const long long at = (long long)(ia + li) * src.Wp + ja + lc;
                    s_tile[0][li][lc] = base[at]; s_tile[1][li][lc] = base[plane + at]; s_tile[2][li][lc] = base[2 * plane + at];
                }
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int li = lr + 8 * q;
                if (li < th && col_ok) {
                    const int r = r0 + li, c = c0 + lc;
                    const int i = (m.flip_c ? w - 1 - c : c) - ia, j = (m.flip_r ? h - 1 - r : r) - ja;
                    acc[q][0] += s_tile[0][i][j]; acc[q][1] += s_tile[1][i][j]; acc[q][2] += s_tile[2][i][j];
                }
            }
        }
    }

    const float inv_k = 1.0f / (float)k;
    auto quantise = [inv_k](float v) -> uint8_t {
        v = fminf(fmaxf(v * inv_k, 0.0f), 1.0f);
        return (uint8_t)rintf(v * 255.0f);                           // numpy round: half to even
    };
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int li = lr + 8 * q;
        if (li < th && col_ok) {
            const uint8_t q0 = quantise(acc[q][0]), q1 = quantise(acc[q][1]), q2 = quantise(acc[q][2]);
            uint8_t* p = dst + ((long long)(r0 + li) * w + c0 + lc) * 3;
            p[0] = swap_rb ? q2 : q0; p[1] = q1; p[2] = swap_rb ? q0 : q2;
        }
    }
}

}  // namespace wm
