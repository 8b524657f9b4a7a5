// The pose between two clouds, point to plane (point_sam_amd/align.py: solve_plane): one ICP step on the cell index of transfer.hip, with a normal
// per source.
//   psam_plane_step   per query the nearest indexed source within r2 of pose(query) -- psam_align_step's pair, bit for bit: pose_apply (rigid_pose.h),
//                     transfer_cell and transfer_candidates (transfer_index.h), the candidate lowest in (q, j) -- and the
//                     thirty-two fp64 sums over the USED pairs from which the host solves the 6 x 6 normal equations of the linearised point-to-plane
//                     residual -- fused: no per-point intermediate leaves the kernel unless `nearest` is asked for
//
// Used pairs.  A pair is used when its source's normal n has nn = (n_x n_x + n_y n_y) + n_z n_z (fp32) finite and > 0: the (0, 0, 0) that
// psam_normals_voxel writes below min_points drops out, and so does a normal with a NaN or an infinity, which never reaches a sum.  Normals are taken
// as given (not normalised); every term is even in n, so their sign does not matter.
//
// Terms.  p = the POSED coordinate (pose_apply's fp32 words; the query itself without a pose), s = the pair, n its normal, all converted to fp64;
// every fp64 operation rounded on its own:
//     d = p - s per component      r = (d_x n_x + d_y n_y) + d_z n_z      c = p x n: c_x = p_y n_z - p_z n_y and cyclic      J = (c_x, c_y, c_z, n_x, n_y, n_z)
// Sums: [0] the used pairs, [1] sum q (the pair's fp32 q) over them, [2] sum r r, [3..8] sum J_a r, [9..29] sum J_a J_b for a <= b (row-major upper
// triangle), [30] the paired queries whose pair was not used, [31] the participating queries that have a cell.  Nothing is accumulated across waves
// in flight, so there are no atomics, and, as in align.hip:
//
//   the order of every fp64 addition is a function of M and the constants of align_combine.h alone -- per lane: query 64 w + lane of wave w holds ONE
//   term per word (nothing is added inside a lane); per wave: the xor butterfly 32, 16, 8, 4, 2, 1 (wave_sum_f64: all lanes agree); per call: the
//   second kernel (align_combine.h: align.hip's) adds the waves' partials of a segment of ceil(ceil(M / 64) / 32) consecutive waves in wave order,
//   then the segments in segment order -- neither the bits, the pose, the data nor the schedule enters it.  The same inputs give the same
//   thirty-two words from run to run.
//
// A wave without a participating query that has a cell stores thirty-two exact zeros and skips the butterfly.
// Every fp32 operation is rounded on its own (-ffp-contract=off).  Caller-owned workspace; no allocation, no host synchronisation.
// The wave's row (the all-zero row, the butterfly, lane 0's store), the second kernel and the host entry are align_combine.h's, shared with
// align.hip.  The pair of a query is written out in both kernels: moved into a shared helper it ran slower (align_combine.h).
#include "common.h"
#include "rigid_pose.h"
#include "transfer_index.h"
#include "align_combine.h"

#include <cmath>

constexpr int PLANE_SUMS = PSAM_PLANE_SUMS;
static_assert(PLANE_SUMS == 2 + 1 + 6 + 21 + 2, "count, q, r r, J r, the upper triangle of J J^T, unused, with a cell");

// One thread per query; the wave's partial sums go to part[wave, 32].
template <bool POSE>
__global__ __launch_bounds__(ALIGN_THREADS) void plane_pair_kernel(TransferIndexView ix, const float* __restrict__ nrm, float ox, float oy, float oz,
                                                                  float inv_h, float r2, const float* __restrict__ qry, int M,
                                                                  const u64* __restrict__ bits, RigidPose P, int* __restrict__ nearest,
                                                                  double* __restrict__ part) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * ALIGN_THREADS + threadIdx.x;
    if ((i & ~(WAVE - 1)) >= M) return;                            // wave-uniform: the block's waves past the last query
    bool takes_part = i < M;
    if (takes_part && bits) takes_part = (bits[i >> 6] >> (i & 63)) & 1ull;
    float px = 0.0f, py = 0.0f, pz = 0.0f, bq = 0.0f;
    int bj = -1;
    bool cell = false;
    if (takes_part) {
        const float x = qry[(int64_t)i * 3 + 0], y = qry[(int64_t)i * 3 + 1], z = qry[(int64_t)i * 3 + 2];
        px = x; py = y; pz = z;
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
    double* __restrict__ out = part + (int64_t)(i >> 6) * PLANE_SUMS;
    const int lane = threadIdx.x & 63;
    if (align_zero_row<PLANE_SUMS>(cell, out, lane)) return;
    double s[PLANE_SUMS];
#pragma unroll
    for (int c = 0; c < PLANE_SUMS; ++c) s[c] = 0.0;
    if (bj >= 0) {                                                 // bj < N: an index of the chains (transfer_candidates)
        const float* __restrict__ np = nrm + (int64_t)bj * 3;
        const float nx = np[0], ny = np[1], nz = np[2];
        const float nn = (nx * nx + ny * ny) + nz * nz;
        if (nn > 0.0f && nn < INFINITY) {                          // NaN compares false
            const float* __restrict__ sp = ix.src + (int64_t)bj * 3;
            const double p[3] = {(double)px, (double)py, (double)pz}, n[3] = {(double)nx, (double)ny, (double)nz};
            const double d[3] = {p[0] - (double)sp[0], p[1] - (double)sp[1], p[2] - (double)sp[2]};
            const double r = (d[0] * n[0] + d[1] * n[1]) + d[2] * n[2];
            const double J[6] = {p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0], n[0], n[1], n[2]};
            s[0] = 1.0;
            s[1] = (double)bq;
            s[2] = r * r;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                s[3 + a] = J[a] * r;
#pragma unroll
                for (int b = a; b < 6; ++b) s[9 + a * 6 - a * (a - 1) / 2 + (b - a)] = J[a] * J[b];      // row a of the triangle starts after 6 + 5 + ...
            }
        } else {
            s[30] = 1.0;
        }
    }
    s[31] = cell ? 1.0 : 0.0;
    align_store_row<PLANE_SUMS>(s, out, lane);
}

PSAM_API size_t psam_plane_workspace_bytes(int32_t M) { return align_workspace_bytes<PLANE_SUMS>(M); }

PSAM_API int32_t psam_plane_step(const float* src, const float* src_normals, int32_t N, const void* index_ws, size_t index_ws_bytes, const float* origin,
                                 float inv_h, float r2, const float* qry, int32_t M, const uint64_t* qry_bits, const float* pose, int32_t* nearest,
                                 double* sums, void* ws, size_t ws_bytes, hipStream_t stream) {
    static const char* const aligned =
        "index_ws must be 16-byte aligned, sums, ws and qry_bits 8-byte aligned, src, src_normals, qry and nearest 4-byte aligned";
    static const TransferEntry entry = {"psam_plane_step", "index workspace", aligned, aligned};
    return align_step_entry<PLANE_SUMS>(entry, "workspace too small (psam_plane_workspace_bytes)", plane_pair_kernel<true>, plane_pair_kernel<false>, src, N,
                                        index_ws, index_ws_bytes, origin, inv_h, r2, qry, M, qry_bits, pose, nearest, sums, ws, ws_bytes, stream, src_normals);
}
