// From a working cloud back to the scan, shared by scene.hip and crops.hip: rows of 32-bit words and rows of packed bits are gathered through
// inv [M], the position of each scan point's representative in the working cloud.  An index outside [0, Nw) -- a crop's -1 for a point off its
// ball; psam_voxel_downsample produces none -- takes the fill word, or a zero bit.  The kernels are templates so that they can live in a header:
// each translation unit that includes this launches its own instance.
#pragma once
#include "row_popcount.h"

constexpr int EXPAND_THREADS = 256;

// ------------------------------------------------------------------------------------------------ expand rows
// One thread per scan point: inv[i] is read once, then one gathered word (or the fill) and one coalesced store per row.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void expand_rows_kernel(const unsigned* __restrict__ src, int64_t src_ld, const int64_t* __restrict__ inv, int R, int Nw,
                                                              int M, unsigned fill, unsigned* __restrict__ dst, int64_t dst_ld) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= M) return;
    const int64_t j = inv[i];
    const bool ok = (u64)j < (u64)Nw;
    int r = 0;
    for (; r + 4 <= R; r += 4) {
        unsigned v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = ok ? src[(int64_t)(r + u) * src_ld + j] : fill;
#pragma unroll
        for (int u = 0; u < 4; ++u) dst[(int64_t)(r + u) * dst_ld + i] = v[u];
    }
    for (; r < R; ++r) dst[(int64_t)r * dst_ld + i] = ok ? src[(int64_t)r * src_ld + j] : fill;
}

static inline int32_t expand_rows_launch(const void* src, int64_t src_ld, const int64_t* inv, int R, int Nw, int M, unsigned fill, void* dst, int64_t dst_ld,
                                         hipStream_t stream, const char* what) {
    hipLaunchKernelGGL(expand_rows_kernel<EXPAND_THREADS>, dim3((unsigned)psam_cdiv(M, EXPAND_THREADS)), dim3(EXPAND_THREADS), 0, stream, (const unsigned*)src,
                       src_ld, inv, R, Nw, M, fill, (unsigned*)dst, dst_ld);
    return psam_launch_status(what);
}

// ------------------------------------------------------------------------------------------------ expand bits
// A wave owns 64 consecutive scan points per output word and BITS_WORDS consecutive words: every lane loads its BITS_WORDS indices once, then for
// every row the ballot of the tested bit IS the output word, and lanes 0 .. BITS_WORDS - 1 store the wave's words of the row as one contiguous
// 64-byte segment.  The working row is read as 32-bit halves (little endian: bit j of the row is bit j % 32 of half j / 32): a working cloud's row is a
// few KiB and stays in cache.  Points past M and indices outside [0, Nw) give a zero bit.  Most of a scan lies off a crop's ball: a wave whose 512
// points all have no source (SKIP_EMPTY: a wave-uniform test on inv) stores zero words for every row and gathers nothing.  A scene has no such wave
// and was measured 0.3 % slower with the test than without (profiles/scene/README.md), so its instance leaves it out.
constexpr int BITS_WORDS = 8;
constexpr int BITS_BLOCK_WORDS = BITS_WORDS * EXPAND_THREADS / WAVE;

template <int THREADS, bool SKIP_EMPTY>
__global__ __launch_bounds__(THREADS) void expand_bits_kernel(const unsigned* __restrict__ bits_w, int64_t Ww, const int64_t* __restrict__ inv, int K, int Nw,
                                                              int M, u64* __restrict__ bits_f, int64_t Wf) {
    const int lane = threadIdx.x & 63;
    const int64_t w0 = ((int64_t)blockIdx.x * (THREADS / WAVE) + (threadIdx.x >> 6)) * BITS_WORDS;
    if (w0 >= Wf) return;                                          // wave-uniform
    int j[BITS_WORDS];
    bool any = false;
#pragma unroll
    for (int u = 0; u < BITS_WORDS; ++u) {
        const int64_t i = (w0 + u) * 64 + lane;
        const int64_t v = i < M ? inv[i] : -1;
        j[u] = (u64)v < (u64)Nw ? (int)v : -1;
        any |= j[u] >= 0;
    }
    const bool store = lane < BITS_WORDS && w0 + lane < Wf;
    if (SKIP_EMPTY && __ballot(any) == 0) {                                      // wave-uniform: nothing to gather
        if (store)
            for (int k = 0; k < K; ++k) bits_f[(int64_t)k * Wf + w0 + lane] = 0;
        return;
    }
    for (int k = 0; k < K; ++k) {
        const unsigned* __restrict__ row = bits_w + (int64_t)k * Ww * 2;
        unsigned half[BITS_WORDS];
#pragma unroll
        for (int u = 0; u < BITS_WORDS; ++u) half[u] = j[u] >= 0 ? row[j[u] >> 5] : 0u;
        u64 mine = 0;
#pragma unroll
        for (int u = 0; u < BITS_WORDS; ++u) {
            const u64 m = __ballot(j[u] >= 0 && ((half[u] >> (j[u] & 31)) & 1u));
            mine = lane == u ? m : mine;
        }
        if (store) bits_f[(int64_t)k * Wf + w0 + lane] = mine;
    }
}

// the expanded rows, then (area_f given) their popcounts
template <bool SKIP_EMPTY>
static inline int32_t expand_bits_launch(const uint64_t* bits_w, const int64_t* inv, int K, int Nw, int M, uint64_t* bits_f, int32_t* area_f, hipStream_t stream,
                                         const char* what, const char* what_area) {
    const int64_t Ww = psam_cdiv(Nw, 64), Wf = psam_cdiv(M, 64);
    hipLaunchKernelGGL((expand_bits_kernel<EXPAND_THREADS, SKIP_EMPTY>), dim3((unsigned)psam_cdiv(Wf, BITS_BLOCK_WORDS)), dim3(EXPAND_THREADS), 0, stream,
                       (const unsigned*)bits_w, Ww, inv, K, Nw, M, (u64*)bits_f, Wf);
    const int32_t st = psam_launch_status(what);
    if (st != PSAM_OK || !area_f) return st;
    hipLaunchKernelGGL(row_popcount_kernel<EXPAND_THREADS>, dim3((unsigned)K), dim3(EXPAND_THREADS), 0, stream, (const u64*)bits_f, Wf, area_f);
    return psam_launch_status(what_area);
}
