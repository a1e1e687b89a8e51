// hip_runtime.h for tools/emulate_patch_batch.cpp and tools/emulate_images_io.cpp ONLY: just enough of the HIP kernel language to compile a kernel header for the
// host - one std::thread per GPU thread, __syncthreads() a barrier over the workgroup, __shared__ a static (one workgroup at a time).
#pragma once
#include <stdint.h>
#include <algorithm>
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
#define __shared__ static
struct Idx { int x, y, z; };
extern thread_local Idx threadIdx;
extern Idx blockIdx;
void __syncthreads();
static inline int min(int a, int b) { return a < b ? a : b; }
static inline int max(int a, int b) { return a > b ? a : b; }
static inline long long min(long long a, long long b) { return a < b ? a : b; }
static inline long long max(long long a, long long b) { return a > b ? a : b; }
