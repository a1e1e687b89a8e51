// patch_batch.hip.h - the train phase of the reference's PairedImageDataset.__getitem__ after the decode, plus the default
// collate, as ONE kernel for a whole batch (basicsr/data/paired_image_dataset.py:80-131 at scale 1):
//
//   padding            (img_util.py:150-166)     bottom / right to at least P with cv2.BORDER_REFLECT, the edge-INCLUDING reflection
//                                                ...cba|abcdefgh|hgf... (numpy 'symmetric'; not the F.pad 'reflect' of image_pre_kernel)
//   paired_random_crop (transforms.py:24-83)     the same P x P window (top, left) of both images
//   data_augmentation  (transforms.py:223-268)   one of the eight flips / rotations, the same for both
//   img2tensor         (img_util.py:9-38)        BGR -> RGB, HWC -> CHW, float32;  / 255
//
// Every sample is described by a row of a DEVICE table (PbRow below), so the launch can sit in a captured graph and see new
// crops on every replay.  Nothing after the division rounds: the outputs are defined bit for bit.
//
// One workgroup forms one 32 x 32 tile of one output image (all three planes).  With A the cropped patch, out[i, j] = A[r, c]:
//
//   mode   0       1          2          3       4              5          6          7
//   r      i       P-1-i      j          j       P-1-i          i          P-1-j      P-1-j
//   c      j       j          P-1-i      i       P-1-j          P-1-j      i          P-1-i
//
// so an output tile is a source tile of A read forwards or backwards along each axis, transposed for modes 2, 3, 6, 7.  The source
// tile goes through LDS as bytes: its rows are read from memory as runs of consecutive bytes whatever the mode, the turn and the
// mirroring happen in the LDS read, and every fp32 plane row leaves as 32 consecutive floats.
//
// Alignment: a source row starts at byte 3 (sy w + sx) of an image whose pitch 3 w is rarely a multiple of 4.  A row is staged in
// LDS at the offset (address & 3), so an ALIGNED dword of memory is an aligned dword of LDS: the dwords that lie wholly inside the
// row's run are loaded as dwords (aligned by construction, inside the image because the run is), the up to 3 bytes before and
// after them byte by byte, and so is every byte of a tile whose columns are reflected (the run is then not consecutive).
//
// LDS: PB_TILE rows of PB_PITCH = 100 bytes (96 of pixels + 3 of offset, rounded to a dword).  25 dwords is odd, so the 32 lanes
// of a transposing read (one source row each, same column) fall on 32 distinct banks; a straight read has neighbouring lanes
// 3 bytes apart, i.e. on the same or the next dword.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wm {

constexpr int PB_TILE = 32;
constexpr int PB_SLOTS = (3 * PB_TILE + 3 + 3) / 4;                 // dwords per staged row: 25
constexpr int PB_PITCH = 4 * PB_SLOTS;
constexpr int PB_FIELDS = 8;                                        // int64 fields per table row

// one sample of the table, as the kernel reads it
struct PbRow {
    const uint8_t* img;
    long long h, w, top, left;
    int mode;
};

// source index of padded index y on an axis of n elements, cv2.BORDER_REFLECT: period 2 n (P may exceed 2 n)
__device__ __forceinline__ long long pb_reflect(long long y, long long n) {
    if (y < n) return y;
    const long long m = y % (2 * n);
    return m < n ? m : 2 * n - 1 - m;
}

// grid (tiles_x * tiles_y * 2 * B): tile fastest, then lq / gt, then the sample; block (256)
__global__ __launch_bounds__(256) void paired_patches_kernel(const long long* __restrict__ table, float* __restrict__ lq,
                                                             float* __restrict__ gt, int P, int tiles, int swap_rb) {
    __shared__ uint32_t s_tile[PB_TILE * PB_SLOTS];
    __shared__ unsigned long long s_row[PB_TILE];                    // address of the aligned dword that holds a row's first byte
    __shared__ int s_off[PB_TILE];                                   // that byte's offset in it (0 for a reflected-column tile)
    uint8_t* const tile8 = reinterpret_cast<uint8_t*>(s_tile);

    const int t = threadIdx.x;
    const int tile = blockIdx.x % (tiles * tiles), rest = blockIdx.x / (tiles * tiles);
    const int which = rest & 1, b = rest >> 1;
    const int i0 = (tile / tiles) * PB_TILE, j0 = (tile % tiles) * PB_TILE;
    const int th = min(PB_TILE, P - i0), tw = min(PB_TILE, P - j0);
    float* const out = (which ? gt : lq) + (long long)b * 3 * P * P;

    // the row of the table, made safe: whatever it says, the reads below stay inside [img, img + 3 h w)
    const long long* row = table + (long long)b * PB_FIELDS;
    PbRow s;
    s.img = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(row[which]));
    s.h = row[2]; s.w = row[3];
    // names no image (or one whose byte offsets would not fit 64 bits): the sample is written as zeros
    const bool empty = s.h < 1 || s.w < 1 || s.h > (1LL << 30) || s.w > (1LL << 30) || s.img == nullptr;
    if (empty) s.h = s.w = 1;
    const long long H = s.h > P ? s.h : P, W = s.w > P ? s.w : P;
    s.top = min(max(row[4], 0LL), H - P);
    s.left = min(max(row[5], 0LL), W - P);
    s.mode = (int)(row[6] & 7);

    const bool turn = (s.mode >> 1) & 1;                             // modes 2, 3, 6, 7: r comes from j, c from i
    const bool flip_r = turn ? s.mode >= 6 : (s.mode == 1 || s.mode == 4);
    const bool flip_c = turn ? (s.mode == 2 || s.mode == 7) : (s.mode == 4 || s.mode == 5);
    // the source tile [r0, r0 + nr) x [c0, c0 + nc) of the patch
    const int ra = turn ? j0 : i0, nr = turn ? tw : th;
    const int ca = turn ? i0 : j0, nc = turn ? th : tw;
    const int r0 = flip_r ? P - ra - nr : ra, c0 = flip_c ? P - ca - nc : ca;
    const bool straight = s.left + c0 + nc <= s.w;                   // the tile's columns are consecutive pixels of the image

    if (!empty) {
        if (t < nr) {
            const long long sy = pb_reflect(s.top + r0 + t, s.h);
            const unsigned long long a = reinterpret_cast<uintptr_t>(s.img) + 3ull * (unsigned long long)(sy * s.w + (straight ? s.left + c0 : 0));
            s_row[t] = straight ? (a & ~3ull) : a;                   // reflected columns: the row's first byte, indexed per pixel below
            s_off[t] = straight ? (int)(a & 3ull) : 0;
        }
        __syncthreads();
        const int len = 3 * nc;
        for (int item = t; item < nr * PB_SLOTS; item += 256) {
            const int rr = item / PB_SLOTS, slot = item % PB_SLOTS;
            const int off = s_off[rr];
            const int lo = max(4 * slot, off), hi = min(4 * slot + 4, off + len);      // the row's bytes inside this dword
            if (lo >= hi) continue;
            if (straight) {
                const uint8_t* base = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(s_row[rr]));
                if (hi - lo == 4)
                    s_tile[rr * PB_SLOTS + slot] = *reinterpret_cast<const uint32_t*>(base + 4 * slot);
                else
                    for (int k = lo; k < hi; ++k) tile8[rr * PB_PITCH + k] = base[k];
            } else {
                const uint8_t* base = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(s_row[rr]));
                for (int k = lo; k < hi; ++k) {
                    const long long sx = pb_reflect(s.left + c0 + k / 3, s.w);
                    tile8[rr * PB_PITCH + k] = base[3 * sx + k % 3];
                }
            }
        }
        __syncthreads();
    }

    const long long plane = (long long)P * P;
    const int lj = t & 31;
    for (int li = t >> 5; li < th; li += 8) {
        if (lj >= tw) continue;
        float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
        if (!empty) {
            const int i = i0 + li, j = j0 + lj;
            const int pr = turn ? j : i, pc = turn ? i : j;
            const int rr = (flip_r ? P - 1 - pr : pr) - r0, cc = (flip_c ? P - 1 - pc : pc) - c0;
            const uint8_t* p = tile8 + rr * PB_PITCH + s_off[rr] + 3 * cc;
            v0 = (float)p[0] / 255.0f; v1 = (float)p[1] / 255.0f; v2 = (float)p[2] / 255.0f;
        }
        const long long o = (long long)(i0 + li) * P + j0 + lj;
        out[o] = swap_rb ? v2 : v0;
        out[plane + o] = v1;
        out[2 * plane + o] = swap_rb ? v0 : v2;
    }
}

}  // namespace wm
