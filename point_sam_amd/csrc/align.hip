// The pose between two clouds (point_sam_amd/align.py): one ICP step on the cell index of transfer.hip.
//   psam_align_step   per query the nearest indexed source within r2 of pose(query), and the twenty fp64 sums over those pairs from which the host
//                     solves for the rigid motion (align.solve_rigid) -- fused: no per-point intermediate leaves the kernel unless `nearest` is asked for
//
// Definition.  The posed coordinate p and the candidates of a query are psam_transfer_plan's, bit for bit: pose_apply (rigid_pose.h), transfer_cell
// and transfer_candidates (transfer_index.h) -- the indexed sources of the 27 cells around cell(p) with q = (dx dx + dy dy) + dz dz <= r2 in fp32,
// NaN false.  The 27-cell set IS the definition; no cell is pruned by a geometric bound (the fp32 rounding of the cell can put a source in reach one
// cell further than geometry suggests).  r2 is the caller's: below the index's own r * r the search simply accepts fewer of the same candidates.  The
// pair of a query is the candidate lowest in (q, j), so neither the order inside a chain nor the schedule enters any output.
//
// Sums.  x = the query as given (NOT posed), s = its pair, both converted to fp64; over the paired queries: the count, sum q, sum x, sum s,
// sum x_a s_b, sum |x|^2, sum |s|^2, and the count of participating queries that have a cell.  Every term is exact (a converted fp32 value, or the
// product of two: 48 significant bits; |x|^2 is added as its three exact products, x first), only the additions round.  Nothing is accumulated
// across waves in flight, so there are no atomics, and:
//
//   the order of every fp64 addition is a function of M and the constants of align_combine.h alone -- per lane: query 64 w + lane of wave w, its
//   terms in the order written, starting from 0; per wave: the xor butterfly 32, 16, 8, 4, 2, 1 (wave_sum_f64: all lanes agree); per call: the second kernel
//   adds the waves' partials of a segment of ALIGN_SEGMENT(M) consecutive waves in wave order, then the segments in segment order -- neither the
//   bits, the pose, the data nor the schedule enters it.  The same inputs give the same twenty words from run to run.
//
// A wave without a participating query that has a cell stores twenty exact zeros and skips the butterfly.
// Every fp32 operation is rounded on its own (-ffp-contract=off).  Caller-owned workspace; no allocation, no host synchronisation.
// The wave's row (the all-zero row, the butterfly, lane 0's store), the second kernel and the host entry are align_combine.h's, shared with
// align_plane.hip.  The pair of a query is written out in both kernels: moved into a shared helper it ran slower (align_combine.h).
#include "common.h"
#include "rigid_pose.h"
#include "transfer_index.h"
#include "align_combine.h"

constexpr int ALIGN_SUMS = PSAM_ALIGN_SUMS;

// One thread per query; the wave's partial sums go to part[wave, 20].
template <bool POSE>
__global__ __launch_bounds__(ALIGN_THREADS) void align_pair_kernel(TransferIndexView ix, float ox, float oy, float oz, float inv_h, float r2,
                                                                  const float* __restrict__ qry, int M, const u64* __restrict__ bits, RigidPose P,
                                                                  int* __restrict__ nearest, double* __restrict__ part) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * ALIGN_THREADS + threadIdx.x;
    if ((i & ~(WAVE - 1)) >= M) return;                            // wave-uniform: the block's waves past the last query
    bool takes_part = i < M;
    if (takes_part && bits) takes_part = (bits[i >> 6] >> (i & 63)) & 1ull;
    float x = 0.0f, y = 0.0f, z = 0.0f, bq = 0.0f;
    int bj = -1;
    bool cell = false;
    if (takes_part) {
        x = qry[(int64_t)i * 3 + 0]; y = qry[(int64_t)i * 3 + 1]; z = qry[(int64_t)i * 3 + 2];
        float px = x, py = y, pz = z;
        if (POSE) pose_apply(P, x, y, z, px, py, pz);              // query frame -> source frame
        u64 cx, cy, cz;
        cell = transfer_cell(px, py, pz, ox, oy, oz, inv_h, cx, cy, cz);
        if (cell) {
            transfer_candidates(ix, px, py, pz, cx, cy, cz, r2, [&](float q, int j) {
                if (bj < 0 || q < bq || (q == bq && j < bj)) { bq = q; bj = j; }
            });
        }
    }
    if (nearest && i < M) nearest[i] = bj;
    double* __restrict__ out = part + (int64_t)(i >> 6) * ALIGN_SUMS;
    const int lane = threadIdx.x & 63;
    if (align_zero_row<ALIGN_SUMS>(cell, out, lane)) return;
    double s[ALIGN_SUMS];
#pragma unroll
    for (int c = 0; c < ALIGN_SUMS; ++c) s[c] = 0.0;
    if (bj >= 0) {
        const float* __restrict__ sp = ix.src + (int64_t)bj * 3;
        const double xd[3] = {(double)x, (double)y, (double)z}, sd[3] = {(double)sp[0], (double)sp[1], (double)sp[2]};
        s[0] = 1.0;
        s[1] = (double)bq;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            s[2 + a] = xd[a];
            s[5 + a] = sd[a];
#pragma unroll
            for (int b = 0; b < 3; ++b) s[8 + a * 3 + b] = xd[a] * sd[b];
            s[17] = s[17] + xd[a] * xd[a];
            s[18] = s[18] + sd[a] * sd[a];
        }
    }
    s[19] = cell ? 1.0 : 0.0;
    align_store_row<ALIGN_SUMS>(s, out, lane);
}

PSAM_API size_t psam_align_workspace_bytes(int32_t M) { return align_workspace_bytes<ALIGN_SUMS>(M); }

PSAM_API int32_t psam_align_step(const float* src, int32_t N, const void* index_ws, size_t index_ws_bytes, const float* origin, float inv_h, float r2,
                                 const float* qry, int32_t M, const uint64_t* qry_bits, const float* pose, int32_t* nearest, double* sums, void* ws,
                                 size_t ws_bytes, hipStream_t stream) {
    static const char* const aligned = "index_ws must be 16-byte aligned, sums, ws and qry_bits 8-byte aligned, src, qry and nearest 4-byte aligned";
    static const TransferEntry entry = {"psam_align_step", "index workspace", aligned, aligned};
    return align_step_entry<ALIGN_SUMS>(entry, "workspace too small (psam_align_workspace_bytes)", align_pair_kernel<true>, align_pair_kernel<false>, src, N,
                                        index_ws, index_ws_bytes, origin, inv_h, r2, qry, M, qry_bits, pose, nearest, sums, ws, ws_bytes, stream);
}
