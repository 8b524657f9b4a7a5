// Scan map tracking (point_sam_amd/scanmap.py: ScanMap.track_step, ScanMap.track): one ICP step of a scan against the map itself.
//   psam_track_step   per query the nearest map voxel (its mean position) within r2 of pose(query), found by probing the map's own voxel table, and
//                     align.hip's twenty fp64 sums over those pairs -- no cloud is read out of the map and no index is built
//   psam_scanmap_plane_step   the same pair, bit for bit, and align_plane.hip's thirty-two fp64 sums over the USED pairs: point to plane, with one normal
//                     per voxel id (psam_scanmap_normals' output fits; taken as given).  One kernel text, the template parameter PLANE
//
// Definition (include/pointsam_hip.h, "scan map tracking"; tests/track_reference.py states it again in numpy).  The posed coordinate p and the cell
// of a query are psam_map_locate's, bit for bit: pose_apply (rigid_pose.h) and map_point (map_block.h).  The candidates are the map voxels in the
// (2 reach + 1)^3 cells around cell(p) whose id is below V, whose count is at least min_count, whose bit in `skip` is clear and whose mean s (map_mean:
// psam_map_cloud's bits) has q = (dx dx + dy dy) + dz dz <= r2 in fp32, d = p - s, NaN false.  The cube IS the definition; no cell is pruned by a
// geometric bound, for align.hip's reason: a voxel's mean lies in its cell only up to the fp32 rounding of the cell.  The pair of a query is the
// candidate lowest in (q, id), so neither the order of the cube nor the schedule enters any output.
//
// Sums, and the order of every fp64 addition: align.hip's, through align_combine.h (the wave's row, the butterfly, the second kernel).  No atomics;
// the same inputs give the same twenty words from run to run.  The map block is only read.  PLANE: used pairs, terms and words are align_plane.hip's,
// word for word -- a pair is used iff its normal has nn (fp32) finite and > 0; p is the POSED fp32 words, s the pair's fp32 mean, both and n
// converted to fp64 -- through the same three pieces of align_combine.h at thirty-two words.
//
// Form.  The kernel is a walk of dependent loads: key -> id -> row, per neighbour cell, and a scan of 10^5 points is two waves per SIMD, so other
// waves do not hide them.  The cube is therefore taken TRACK_BATCH cells at a time, and each stage of the walk is issued for the whole batch
// before the next stage consumes it: the first probe of every cell, then (rarely, one cell at a time) the rest of a probe chain, then the ids,
// then the rows.  A cell that is off the grid or holds no voxel reads slot 0 / row 0 instead, in bounds and unused, so that every load of a stage is
// unconditional and they are in flight together.  Every array below is indexed by unrolled constants: nothing goes to scratch.
#include "map_block.h"
#include "align_combine.h"

#include <cmath>

constexpr int TRACK_SUMS = PSAM_ALIGN_SUMS;
constexpr int PLANE_SUMS = PSAM_PLANE_SUMS;
constexpr int TRACK_MAX_REACH = PSAM_TRACK_MAX_REACH;
constexpr int TRACK_BATCH = 9;                                     // reach 1: three batches of one 3 x 3 plane each

// One thread per query; the wave's partial sums go to part[wave, SUMS].  PLANE: nrm [V, 3] and align_plane.hip's thirty-two sums; otherwise nrm is
// not read and the sums are align.hip's twenty.  The pair search is one text for both; the point-to-point instances compile to the instructions they
// had before PLANE existed.
template <bool POSE, bool PLANE>
__global__ __launch_bounds__(ALIGN_THREADS) void track_pair_kernel(const int* __restrict__ header, const u64* __restrict__ keys, const int* __restrict__ id,
                                                                  int cv, const u64* __restrict__ rows, int V, const u64* __restrict__ skip, int min_count,
                                                                  int reach, float r2, const float* __restrict__ qry, int M, const u64* __restrict__ bits,
                                                                  RigidPose P, int* __restrict__ nearest, double* __restrict__ part,
                                                                  const float* __restrict__ nrm) {
#pragma clang fp contract(off)
    constexpr int SUMS = PLANE ? PLANE_SUMS : TRACK_SUMS;
    const int i = blockIdx.x * ALIGN_THREADS + threadIdx.x;
    if ((i & ~(WAVE - 1)) >= M) return;                            // wave-uniform: the block's waves past the last query
    bool takes_part = i < M;
    if (takes_part && bits) takes_part = (bits[i >> 6] >> (i & 63)) & 1ull;
    float x = 0.0f, y = 0.0f, z = 0.0f, bq = 0.0f, bs[3] = {0.0f, 0.0f, 0.0f};
    int bv = -1;
    bool cell = false;
    if (takes_part) {
        x = qry[(int64_t)i * 3 + 0]; y = qry[(int64_t)i * 3 + 1]; z = qry[(int64_t)i * 3 + 2];
        float px = x, py = y, pz = z;
        if (POSE) pose_apply(P, x, y, z, px, py, pz);              // scan frame -> map frame
        if constexpr (PLANE) { x = px; y = py; z = pz; }           // the plane terms take the posed words; the point-to-point sums the query as given
        u64 fixed[3], own;
        cell = map_point<POSE>(qry, i, P, map_inv_h(header), fixed, own);      // poses the point again: the same arithmetic, the same bits as p
        if (cell) {
            const int c0 = (int)(own & ((1ull << VOXEL_AXIS_BITS) - 1ull)), c1 = (int)((own >> VOXEL_AXIS_BITS) & ((1ull << VOXEL_AXIS_BITS) - 1ull)),
                      c2 = (int)(own >> (2 * VOXEL_AXIS_BITS));
            const int n = 2 * reach + 1, cells = n * n * n;
            const unsigned mask = (unsigned)cv - 1u;
            int d0 = -reach, d1 = -reach, d2 = -reach;             // the offset of the next cell of the cube, axis 0 fastest
            for (int base = 0; base < cells; base += TRACK_BATCH) {
                u64 key[TRACK_BATCH], cur[TRACK_BATCH];
                unsigned pos[TRACK_BATCH];
                int slot[TRACK_BATCH], v[TRACK_BATCH];
#pragma unroll
                for (int k = 0; k < TRACK_BATCH; ++k) {            // stage 1: the first probe of every cell of the batch
                    const int a0 = c0 + d0, a1 = c1 + d1, a2 = c2 + d2;
                    const bool on_grid = base + k < cells && ((unsigned)a0 | (unsigned)a1 | (unsigned)a2) < (1u << VOXEL_AXIS_BITS);
                    key[k] = on_grid ? voxel_key((u64)a0, (u64)a1, (u64)a2) : VOXEL_EMPTY;
                    pos[k] = on_grid ? (unsigned)voxel_hash(key[k]) & mask : 0u;
                    cur[k] = keys[pos[k]];
                    if (++d0 > reach) { d0 = -reach; if (++d1 > reach) { d1 = -reach; ++d2; } }
                }
#pragma unroll
                for (int k = 0; k < TRACK_BATCH; ++k)              // stage 2: the rest of a chain; a cell off the grid has no slot
                    slot[k] = key[k] == VOXEL_EMPTY ? -1 : map_find_rest(keys, cv, key[k], pos[k], cur[k]);
#pragma unroll
                for (int k = 0; k < TRACK_BATCH; ++k) v[k] = id[slot[k] >= 0 ? slot[k] : 0];      // stage 3
                ulonglong2 lo[TRACK_BATCH], hi[TRACK_BATCH];
                u64 word[TRACK_BATCH];
#pragma unroll
                for (int k = 0; k < TRACK_BATCH; ++k) {            // stage 4: count and the three sums of the position; the voxel's word of `skip`
                    if (!(slot[k] >= 0 && v[k] >= 0 && v[k] < V)) v[k] = -1;
                    const int at = v[k] >= 0 ? v[k] : 0;
                    const ulonglong2* __restrict__ row = (const ulonglong2*)(rows + (int64_t)at * MAP_ROW);
                    lo[k] = row[0];
                    hi[k] = row[1];
                    word[k] = skip ? skip[at >> 6] : 0ull;
                }
#pragma unroll
                for (int k = 0; k < TRACK_BATCH; ++k) {
                    if (v[k] < 0 || lo[k].x < (u64)min_count || ((word[k] >> (v[k] & 63)) & 1ull)) continue;
                    const float s0 = map_mean(lo[k].y, lo[k].x), s1 = map_mean(hi[k].x, lo[k].x), s2 = map_mean(hi[k].y, lo[k].x);
                    const float e0 = px - s0, e1 = py - s1, e2 = pz - s2;
                    const float q = (e0 * e0 + e1 * e1) + e2 * e2;
                    if (!(q <= r2)) continue;
                    if (bv < 0 || q < bq || (q == bq && v[k] < bv)) { bq = q; bv = v[k]; bs[0] = s0; bs[1] = s1; bs[2] = s2; }
                }
            }
        }
    }
    if (nearest && i < M) nearest[i] = bv;
    double* __restrict__ out = part + (int64_t)(i >> 6) * SUMS;
    const int lane = threadIdx.x & 63;
    if (align_zero_row<SUMS>(cell, out, lane)) return;
    double s[SUMS];
#pragma unroll
    for (int c = 0; c < SUMS; ++c) s[c] = 0.0;
    if constexpr (PLANE) {
        if (bv >= 0) {                                             // bv < V: a row of nrm
            const float* __restrict__ np = nrm + (int64_t)bv * 3;
            const float nx = np[0], ny = np[1], nz = np[2];
            const float nn = (nx * nx + ny * ny) + nz * nz;
            if (nn > 0.0f && nn < INFINITY) {                      // NaN compares false
                const double p[3] = {(double)x, (double)y, (double)z}, n[3] = {(double)nx, (double)ny, (double)nz};
                const double d[3] = {p[0] - (double)bs[0], p[1] - (double)bs[1], p[2] - (double)bs[2]};
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
    } else {
        if (bv >= 0) {
            const double xd[3] = {(double)x, (double)y, (double)z}, sd[3] = {(double)bs[0], (double)bs[1], (double)bs[2]};
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
    }
    s[SUMS - 1] = cell ? 1.0 : 0.0;
    align_store_row<SUMS>(s, out, lane);
}

// The host entry of both steps: the checks, the pair kernel (with or without a pose) and the combine kernel.  `nrm` is null for psam_track_step.
template <bool PLANE>
static inline int32_t track_entry(const char* name, const void* map, size_t map_bytes, int32_t max_voxels, int32_t max_pairs, int32_t V, const float* nrm,
                                  const uint64_t* skip, int32_t min_count, int32_t reach, float r2, const float* qry, int32_t M, const uint64_t* qry_bits,
                                  const float* pose, int32_t* nearest, double* sums, void* ws, size_t ws_bytes, hipStream_t stream) {
    constexpr int SUMS = PLANE ? PLANE_SUMS : TRACK_SUMS;
    if (!(map && qry && sums && ws && (!PLANE || nrm))) return transfer_refuse(PSAM_EINVAL, name, "null pointer");
    if (!(M > 0 && M <= MAP_MAX_POINTS)) return transfer_refuse(PSAM_EINVAL, name, "need 0 < M <= 2^28");
    if (!map_caps_ok(max_voxels, max_pairs)) return transfer_refuse(PSAM_EINVAL, name, "need 0 < max_voxels <= 2^28 and 0 < max_pairs <= 2^28");
    if (!(V > 0 && V <= max_voxels)) return transfer_refuse(PSAM_EINVAL, name, "need 0 < V <= max_voxels");
    if (!(reach >= 1 && reach <= TRACK_MAX_REACH)) return transfer_refuse(PSAM_EINVAL, name, "need 1 <= reach <= 4");
    if (!(min_count >= 1)) return transfer_refuse(PSAM_EINVAL, name, "min_count must be at least 1");
    if (!(std::isfinite(r2) && r2 > 0.0f)) return transfer_refuse(PSAM_EINVAL, name, "r2 must be finite and positive");
    RigidPose P = {};
    if (pose && !pose_load(pose, P)) return transfer_refuse(PSAM_EINVAL, name, "pose must be finite");
    if (!(((uintptr_t)map & 15) == 0 && (((uintptr_t)sums | (uintptr_t)ws | (uintptr_t)skip | (uintptr_t)qry_bits) & 7) == 0 &&
          (((uintptr_t)qry | (uintptr_t)nearest | (uintptr_t)nrm) & 3) == 0))
        return transfer_refuse(PSAM_EALIGN, name,
                               PLANE ? "map must be 16-byte aligned, sums, ws, skip and qry_bits 8-byte aligned, qry, normals and nearest 4-byte aligned"
                                     : "map must be 16-byte aligned, sums, ws, skip and qry_bits 8-byte aligned, qry and nearest 4-byte aligned");
    if (map_bytes < map_layout(nullptr, max_voxels, max_pairs).bytes) return transfer_refuse(PSAM_EWORKSPACE, name, "map block too small (psam_map_bytes)");
    if (ws_bytes < align_workspace_bytes<SUMS>(M))
        return transfer_refuse(PSAM_EWORKSPACE, name, PLANE ? "workspace too small (psam_scanmap_plane_workspace_bytes)" : "workspace too small (psam_track_workspace_bytes)");
    const MapBlock b = map_layout((void*)map, max_voxels, max_pairs);
    double* part = (double*)ws;
    const auto kernel = pose ? track_pair_kernel<true, PLANE> : track_pair_kernel<false, PLANE>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)psam_cdiv(M, ALIGN_THREADS)), dim3(ALIGN_THREADS), 0,
                       stream, (const int*)b.header, (const u64*)b.keys, (const int*)b.id, b.cv, (const u64*)b.rows, (int)V, (const u64*)skip, (int)min_count,
                       (int)reach, r2, qry, (int)M, (const u64*)qry_bits, P, (int*)nearest, part, nrm);
    int32_t st = align_launch_status(name, "launch failed");
    if (st != PSAM_OK) return st;
    const int waves = (int)align_waves(M);
    hipLaunchKernelGGL(align_combine_kernel<SUMS>, dim3(1), dim3(ALIGN_SEGMENTS * ALIGN_COLUMNS), 0, stream, (const double*)part, waves,
                       (int)psam_cdiv(waves, ALIGN_SEGMENTS), sums);
    return align_launch_status(name, "combine launch failed");
}

PSAM_API size_t psam_track_workspace_bytes(int32_t M) { return align_workspace_bytes<TRACK_SUMS>(M); }

PSAM_API int32_t psam_track_step(const void* map, size_t map_bytes, int32_t max_voxels, int32_t max_pairs, int32_t V, const uint64_t* skip, int32_t min_count,
                                 int32_t reach, float r2, const float* qry, int32_t M, const uint64_t* qry_bits, const float* pose, int32_t* nearest,
                                 double* sums, void* ws, size_t ws_bytes, hipStream_t stream) {
    return track_entry<false>("psam_track_step", map, map_bytes, max_voxels, max_pairs, V, nullptr, skip, min_count, reach, r2, qry, M, qry_bits, pose, nearest,
                              sums, ws, ws_bytes, stream);
}

PSAM_API size_t psam_scanmap_plane_workspace_bytes(int32_t M) { return align_workspace_bytes<PLANE_SUMS>(M); }

PSAM_API int32_t psam_scanmap_plane_step(const void* map, size_t map_bytes, int32_t max_voxels, int32_t max_pairs, int32_t V, const float* normals,
                                       const uint64_t* skip, int32_t min_count, int32_t reach, float r2, const float* qry, int32_t M,
                                       const uint64_t* qry_bits, const float* pose, int32_t* nearest, double* sums, void* ws, size_t ws_bytes,
                                       hipStream_t stream) {
    return track_entry<true>("psam_scanmap_plane_step", map, map_bytes, max_voxels, max_pairs, V, normals, skip, min_count, reach, r2, qry, M, qry_bits, pose,
                             nearest, sums, ws, ws_bytes, stream);
}
