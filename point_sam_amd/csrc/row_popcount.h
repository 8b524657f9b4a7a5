// The popcount of a row of packed bits and the block sum under it: the area pass of scene_expand.h's and scene_interp.hip's packed masks, and the
// reductions of regions.hip's row kernels.  row_popcount_kernel is a template so that it can live in a header; a translation unit that launches it
// gets its own instance.
#pragma once
#include "voxel_cell.h"      // u64

// The sum of c over a block of THREADS threads, valid in thread 0; s_cnt [THREADS / WAVE] shared words.  One __syncthreads(): shared words the
// caller wrote before the call are visible after it.
template <int THREADS>
__device__ __forceinline__ int block_sum(int c, int* s_cnt) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    int s = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < THREADS / WAVE; ++w) s += s_cnt[w];
    return s;
}

// The set bits of row[0 .. W), valid in thread 0.  The index type is the caller's W's.
template <int THREADS, typename Index>
__device__ __forceinline__ int row_popcount(const u64* __restrict__ row, Index W, int* s_cnt) {
    int c = 0;
    for (Index w = threadIdx.x; w < W; w += THREADS) c += __popcll(row[w]);
    return block_sum<THREADS>(c, s_cnt);
}

// area[k] = the set bits of row k: one block per row, a pass of its own over the finished rows
template <int THREADS>
__global__ __launch_bounds__(THREADS) void row_popcount_kernel(const u64* __restrict__ bits, int64_t W, int* __restrict__ area) {
    __shared__ int s_cnt[THREADS / WAVE];
    const int s = row_popcount<THREADS>(bits + (int64_t)blockIdx.x * W, W, s_cnt);
    if (threadIdx.x == 0) area[blockIdx.x] = s;
}
