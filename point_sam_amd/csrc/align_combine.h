// The second kernel of the two ICP steps (align.hip: point to point, align_plane.hip: point to plane): the order in which the waves' partial sums are
// added is one decision and lives here once.  Both first kernels hold query 64 w + lane in lane `lane` of wave w and store one row of SUMS fp64
// partials per wave (the xor butterfly of wave_sum_f64); this kernel adds the rows.
#pragma once
#include "common.h"

constexpr int ALIGN_SEGMENTS = 32;                                 // ALIGN_SEGMENTS x 32 threads, column c of segment s at thread 32 s + c
constexpr int ALIGN_COLUMNS = 32;

static inline int64_t align_waves(int64_t M) { return psam_cdiv(M, WAVE); }

// One workgroup.  Thread 32 s + c adds column c of the waves [s per, (s + 1) per) in wave order; then thread c adds the segments in segment order.
template <int SUMS>
__global__ __launch_bounds__(ALIGN_SEGMENTS * ALIGN_COLUMNS) void align_combine_kernel(const double* __restrict__ part, int waves, int per,
                                                                                       double* __restrict__ sums) {
    static_assert(SUMS <= ALIGN_COLUMNS, "one thread per column");
    __shared__ double seg[ALIGN_SEGMENTS][ALIGN_COLUMNS];
    const int c = threadIdx.x % ALIGN_COLUMNS, s = threadIdx.x / ALIGN_COLUMNS;
    double acc = 0.0;
    if (c < SUMS) {
        const int hi = min((s + 1) * per, waves);
        for (int w = s * per; w < hi; ++w) acc = acc + part[(int64_t)w * SUMS + c];
    }
    seg[s][c] = acc;
    __syncthreads();
    if (s == 0 && c < SUMS) {
        double total = 0.0;
        for (int t = 0; t < ALIGN_SEGMENTS; ++t) total = total + seg[t][c];
        sums[c] = total;
    }
}
