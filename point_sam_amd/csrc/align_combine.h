// What the two ICP steps share (align.hip: point to point, align_plane.hip: point to plane): the wave's row of partial sums, the order in which
// the second kernel adds the rows, and the host entry are one decision each and live here once.  Both first kernels hold query 64 w + lane in lane
// `lane` of wave w and store one row of SUMS fp64 partials per wave (the xor butterfly of wave_sum_f64); the second kernel adds the rows.
// NOT here: the pair of a query (the bits test, the load, the pose, the cell, the (q, j) minimum), which both kernels write out.  As one helper it
// computes the same bits, but both kernels then compile to another block layout and measured 2.5 - 4 % slower on an MI355X where the chain walk
// dominates (profiles/align/README.md), in every form tried (a struct, reference parameters).  Change the two copies together.
#pragma once
#include "common.h"
#include "rigid_pose.h"
#include "transfer_index.h"

#include <cstdio>

constexpr int ALIGN_THREADS = 256;
constexpr int ALIGN_SEGMENTS = 32;                                 // ALIGN_SEGMENTS x 32 threads, column c of segment s at thread 32 s + c
constexpr int ALIGN_COLUMNS = 32;

static inline int64_t align_waves(int64_t M) { return psam_cdiv(M, WAVE); }

template <int SUMS>
static inline size_t align_workspace_bytes(int32_t M) {
    if (M <= 0 || M > VOXEL_MAX_POINTS) return 0;
    return (size_t)align_waves(M) * SUMS * sizeof(double);
}

// The row of a wave, out = part + wave * SUMS.  A wave in which no lane has a cell stores SUMS exact zeros and is done (true): the kernel returns
// and skips its terms and the butterfly.
template <int SUMS>
__device__ __forceinline__ bool align_zero_row(bool cell, double* __restrict__ out, int lane) {
    if (__ballot(cell) != 0) return false;
    if (lane < SUMS) out[lane] = 0.0;                              // wave-uniform: nothing to add
    return true;
}

// The lanes' words s[SUMS] added over the wave by the xor butterfly; lane 0 stores the row.
template <int SUMS>
__device__ __forceinline__ void align_store_row(double (&s)[SUMS], double* __restrict__ out, int lane) {
#pragma unroll
    for (int c = 0; c < SUMS; ++c) s[c] = wave_sum_f64(s[c]);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < SUMS; ++c) out[c] = s[c];
    }
}

// The second kernel.  One workgroup.  Thread 32 s + c adds column c of the waves [s per, (s + 1) per) in wave order; then thread c adds the segments
// in segment order.
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

static inline int32_t align_launch_status(const char* entry, const char* what) {
    char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s", entry, what);
    return psam_launch_status(msg);
}

// The host entry of a step: the checks, the pair kernel (with or without a pose) and the combine kernel.  `extra`: the per-source arrays the pair
// kernel takes after the index (the normals), each required and 4-byte aligned like src; ws_small is the entry's text for a workspace below its own workspace query.
template <int SUMS, class Kernel, class... Extra>
static inline int32_t align_step_entry(const TransferEntry& e, const char* ws_small, Kernel posed, Kernel unposed, const float* src, int32_t N,
                                       const void* index_ws, size_t index_ws_bytes, const float* origin, float inv_h, float r2, const float* qry, int32_t M,
                                       const uint64_t* qry_bits, const float* pose, int32_t* nearest, double* sums, void* ws, size_t ws_bytes,
                                       hipStream_t stream, Extra... extra) {
    const bool aligned = (((uintptr_t)sums | (uintptr_t)ws | (uintptr_t)qry_bits) & 7) == 0 && (((uintptr_t)nearest | ... | (uintptr_t)extra) & 3) == 0;
    int32_t st = transfer_check_query(e, src, N, index_ws, index_ws_bytes, origin, inv_h, r2, qry, M, (sums && ws) && (... && extra), aligned);
    if (st != PSAM_OK) return st;
    RigidPose P = {};
    if (pose && !pose_load(pose, P)) return transfer_refuse(PSAM_EINVAL, e.name, "pose must be finite");
    if (ws_bytes < align_workspace_bytes<SUMS>(M)) return transfer_refuse(PSAM_EWORKSPACE, e.name, ws_small);
    const TransferIndexView ix = transfer_view(src, N, index_ws);
    double* part = (double*)ws;
    hipLaunchKernelGGL(pose ? posed : unposed, dim3((unsigned)psam_cdiv(M, ALIGN_THREADS)), dim3(ALIGN_THREADS), 0, stream, ix, extra..., origin[0],
                       origin[1], origin[2], inv_h, r2, qry, (int)M, (const u64*)qry_bits, P, (int*)nearest, part);
    st = align_launch_status(e.name, "launch failed");
    if (st != PSAM_OK) return st;
    const int waves = (int)align_waves(M);
    hipLaunchKernelGGL(align_combine_kernel<SUMS>, dim3(1), dim3(ALIGN_SEGMENTS * ALIGN_COLUMNS), 0, stream, (const double*)part, waves,
                       (int)psam_cdiv(waves, ALIGN_SEGMENTS), sums);
    return align_launch_status(e.name, "combine launch failed");
}
