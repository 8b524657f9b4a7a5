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
#include "common.h"
#include "rigid_pose.h"
#include "transfer_index.h"
#include "align_combine.h"

#include <cmath>

constexpr int PLANE_THREADS = 256;
constexpr int PLANE_SUMS = PSAM_PLANE_SUMS;
static_assert(PLANE_SUMS == 2 + 1 + 6 + 21 + 2, "count, q, r r, J r, the upper triangle of J J^T, unused, with a cell");

// One thread per query; the wave's partial sums go to part[wave, 32].
template <bool POSE>
__global__ __launch_bounds__(PLANE_THREADS) void plane_pair_kernel(TransferIndexView ix, const float* __restrict__ nrm, float ox, float oy, float oz,
                                                                  float inv_h, float r2, const float* __restrict__ qry, int M,
                                                                  const u64* __restrict__ bits, RigidPose P, int* __restrict__ nearest,
                                                                  double* __restrict__ part) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * PLANE_THREADS + threadIdx.x;
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
    if (__ballot(cell) == 0) {                                     // wave-uniform: nothing to add
        if (lane < PLANE_SUMS) out[lane] = 0.0;
        return;
    }
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
#pragma unroll
    for (int c = 0; c < PLANE_SUMS; ++c) s[c] = wave_sum_f64(s[c]);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < PLANE_SUMS; ++c) out[c] = s[c];
    }
}

PSAM_API size_t psam_plane_workspace_bytes(int32_t M) {
    if (M <= 0 || M > VOXEL_MAX_POINTS) return 0;
    return (size_t)align_waves(M) * PLANE_SUMS * sizeof(double);
}

PSAM_API int32_t psam_plane_step(const float* src, const float* src_normals, int32_t N, const void* index_ws, size_t index_ws_bytes, const float* origin,
                                 float inv_h, float r2, const float* qry, int32_t M, const uint64_t* qry_bits, const float* pose, int32_t* nearest,
                                 double* sums, void* ws, size_t ws_bytes, hipStream_t stream) {
    PSAM_REQUIRE(src && src_normals && index_ws && origin && qry && sums && ws, PSAM_EINVAL, "psam_plane_step: null pointer");
    PSAM_REQUIRE(N > 0 && N <= VOXEL_MAX_POINTS, PSAM_EINVAL, "psam_plane_step: need 0 < N <= 2^28");
    PSAM_REQUIRE(M > 0 && M <= VOXEL_MAX_POINTS, PSAM_EINVAL, "psam_plane_step: need 0 < M <= 2^28");
    PSAM_REQUIRE(std::isfinite(inv_h) && inv_h > 0.0f, PSAM_EINVAL, "psam_plane_step: inv_h must be finite and positive");
    PSAM_REQUIRE(std::isfinite(r2) && r2 > 0.0f, PSAM_EINVAL, "psam_plane_step: r2 must be finite and positive");
    PSAM_REQUIRE(transfer_finite3(origin), PSAM_EINVAL, "psam_plane_step: origin must be finite");
    RigidPose P = {};
    PSAM_REQUIRE(!pose || pose_load(pose, P), PSAM_EINVAL, "psam_plane_step: pose must be finite");
    PSAM_REQUIRE((((uintptr_t)sums | (uintptr_t)ws | (uintptr_t)qry_bits) & 7) == 0 && ((uintptr_t)index_ws & 15) == 0 &&
                     (((uintptr_t)src | (uintptr_t)src_normals | (uintptr_t)qry | (uintptr_t)nearest) & 3) == 0,
                 PSAM_EALIGN,
                 "psam_plane_step: index_ws must be 16-byte aligned, sums, ws and qry_bits 8-byte aligned, src, src_normals, qry and nearest 4-byte aligned");
    PSAM_REQUIRE(index_ws_bytes >= transfer_layout(nullptr, N).bytes, PSAM_EWORKSPACE,
                 "psam_plane_step: index workspace too small (psam_transfer_index_workspace_bytes)");
    PSAM_REQUIRE(ws_bytes >= psam_plane_workspace_bytes(M), PSAM_EWORKSPACE, "psam_plane_step: workspace too small (psam_plane_workspace_bytes)");
    const TransferIndexView ix = transfer_view(src, N, index_ws);
    const dim3 grid((unsigned)psam_cdiv(M, PLANE_THREADS)), block(PLANE_THREADS);
    double* part = (double*)ws;
    if (pose) {
        hipLaunchKernelGGL(plane_pair_kernel<true>, grid, block, 0, stream, ix, src_normals, origin[0], origin[1], origin[2], inv_h, r2, qry, (int)M,
                           (const u64*)qry_bits, P, (int*)nearest, part);
    } else {
        hipLaunchKernelGGL(plane_pair_kernel<false>, grid, block, 0, stream, ix, src_normals, origin[0], origin[1], origin[2], inv_h, r2, qry, (int)M,
                           (const u64*)qry_bits, P, (int*)nearest, part);
    }
    const int32_t st = psam_launch_status("psam_plane_step: launch failed");
    if (st != PSAM_OK) return st;
    const int waves = (int)align_waves(M);
    hipLaunchKernelGGL(align_combine_kernel<PLANE_SUMS>, dim3(1), dim3(ALIGN_SEGMENTS * ALIGN_COLUMNS), 0, stream, (const double*)part, waves,
                       (int)psam_cdiv(waves, ALIGN_SEGMENTS), sums);
    return psam_launch_status("psam_plane_step: combine launch failed");
}
