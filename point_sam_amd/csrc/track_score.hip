// Relocalising a scan in the scan map (point_sam_amd/scanmap.py: ScanMap.track_score, ScanMap.relocalize): the inner question of a global pose
// search, asked of the map itself -- under each of P candidate poses, how many queries land on a voxel of the map?
//   psam_relocalize_score   counts[p] = the number of queries that have AT LEAST ONE candidate under pose p, all P poses from one call
//
// Definition (include/pointsam_hip.h, "scan map relocalisation"; tests/track_score_reference.py states it again in numpy).  The posed coordinate, the
// cell, the acceptance test and the candidates of a query are psam_track_step's, bit for bit: pose_apply (rigid_pose.h), map_point with the map's
// inv_h (map_block.h), the (2 reach + 1)^3 cells around cell(p) with cells off the grid skipped, voxel id < V, count >= min_count, the voxel's bit in
// `skip` clear, and q = (dx dx + dy dy) + dz dz <= r2 in fp32 against map_mean's bits, NaN false.  The cube IS the definition; no cell is pruned by a
// geometric bound, for track.hip's reason.  So counts[p] == psam_track_step's sums[0] under pose p and the same r2, skip and min_count, for every p.
// A query without a cell, and a pose that is not finite (NaN coordinates, no cell), score 0.
//
// Means table.  track.hip pays three fp64 divisions per candidate; here they would be paid P * M * cells times.  A pre-kernel therefore writes one
// float4 per voxel id < V into the workspace: map_mean of the row's three sums -- the same function on the same words, so the same bits -- or NaN
// for a voxel that may not be paired (count < min_count, or its skip bit set), for which q <= r2 is then false without a test of its own.  The walk
// becomes key -> id -> one 16-byte load.  The table is rebuilt by every call (the map may have grown, skip may have changed); nothing is cached.
//
// Shape: align_score.hip's.  One thread per query, the query in registers; a workgroup takes RELOC_THREADS queries through the RELOC_POSES poses of
// one chunk (grid: query tiles x pose chunks; past 65535 chunks a workgroup strides over them).  A pose's twelve words are read at a wave-uniform
// address, so they arrive by scalar loads.  Per pose a wave adds __popcll(__ballot(hit)) with ONE integer atomicAdd, and none when nobody hit; the
// entry zeroes counts on the stream first.  Integer addition commutes and the totals stay below 2^28, so the words are a function of the inputs
// alone.
//
// Early exit.  Existence is settled by the first candidate that passes EVERY test -- a skipped, sparse or out-of-radius voxel does not end the
// walk.  The query's own cell is visited first (a query that sits on the map costs one probe), then the cube in batches; the order cannot change
// the result.  Latency: track.hip's staging -- the first probes of a batch, then the rest of the chains, then the ids, then the rows, every load of
// a stage unconditional (a cell that is off the grid or holds no voxel reads slot 0 / row 0, in bounds and unused).  Every array is indexed by
// unrolled constants: nothing goes to scratch.  The map block is only read; no allocation, no host synchronisation.
#include "map_block.h"
#include "transfer_index.h"      // transfer_refuse

#include <cmath>

constexpr int RELOC_THREADS = 256;
constexpr int RELOC_POSES = PSAM_RELOCALIZE_POSES;
constexpr int RELOC_MAX_POSES = 1 << 20;
constexpr int RELOC_MAX_GRID_Y = 65535;
constexpr int RELOC_MAX_REACH = PSAM_TRACK_MAX_REACH;
constexpr int RELOC_BATCH = 9;                                     // reach 1: three batches of one 3 x 3 plane each

// means[v] = (map_mean of the three sums, 0) for a voxel that may be paired, NaN otherwise
__global__ __launch_bounds__(MAP_THREADS) void relocalize_means_kernel(const u64* __restrict__ rows, int V, const u64* __restrict__ skip, int min_count,
                                                                        float4* __restrict__ means) {
#pragma clang fp contract(off)
    const int v = blockIdx.x * MAP_THREADS + threadIdx.x;
    if (v >= V) return;
    const ulonglong2* __restrict__ row = (const ulonglong2*)(rows + (int64_t)v * MAP_ROW);
    const ulonglong2 lo = row[0], hi = row[1];                     // count and the three sums of the position
    const u64 word = skip ? skip[v >> 6] : 0ull;
    const float nan = __builtin_nanf("");
    float4 out = make_float4(nan, nan, nan, 0.0f);
    if (lo.x >= (u64)min_count && !((word >> (v & 63)) & 1ull)) out = make_float4(map_mean(lo.y, lo.x), map_mean(hi.x, lo.x), map_mean(hi.y, lo.x), 0.0f);
    means[v] = out;
}

// whether the row read for a cell is a candidate: `found` says the cell holds a voxel with an id below V; a NaN row compares false
__device__ __forceinline__ bool relocalize_candidate(bool found, const float4& s, float px, float py, float pz, float r2) {
#pragma clang fp contract(off)
    const float e0 = px - s.x, e1 = py - s.y, e2 = pz - s.z;
    const float q = (e0 * e0 + e1 * e1) + e2 * e2;
    return found && q <= r2;
}

__global__ __launch_bounds__(RELOC_THREADS) void relocalize_score_kernel(const int* __restrict__ header, const u64* __restrict__ keys, const int* __restrict__ id,
                                                                          int cv, const float4* __restrict__ means, int V, int reach, float r2,
                                                                          const float* __restrict__ qry, int M, const float* __restrict__ poses, int P,
                                                                          int* __restrict__ counts) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * RELOC_THREADS + threadIdx.x;
    if ((i & ~(WAVE - 1)) >= M) return;                            // wave-uniform: the block's waves past the last query
    const bool live = i < M;
    float xyz[3] = {0.0f, 0.0f, 0.0f};
    if (live) { xyz[0] = qry[(int64_t)i * 3 + 0]; xyz[1] = qry[(int64_t)i * 3 + 1]; xyz[2] = qry[(int64_t)i * 3 + 2]; }
    const int lane = threadIdx.x & 63;
    const float inv_h = map_inv_h(header);
    const unsigned mask = (unsigned)cv - 1u;
    const int n = 2 * reach + 1, cells = n * n * n;
    const int chunks = (P + RELOC_POSES - 1) / RELOC_POSES;
    for (int c = blockIdx.y; c < chunks; c += gridDim.y) {
        const int end = min((c + 1) * RELOC_POSES, P);
        for (int p = c * RELOC_POSES; p < end; ++p) {              // p is wave-uniform, and so is the address of the pose
            RigidPose T;
#pragma unroll
            for (int a = 0; a < 12; ++a) T.m[a] = poses[(int64_t)p * 12 + a];
            bool hit = false;
            if (live) {
                float px, py, pz;
                pose_apply(T, xyz[0], xyz[1], xyz[2], px, py, pz);  // scan frame -> map frame
                u64 fixed[3], own;
                if (map_point<true>(xyz, 0, T, inv_h, fixed, own)) {      // poses the point again: the same arithmetic, the same bits as p
                    {                                              // the query's own cell first
                        const unsigned pos = (unsigned)voxel_hash(own) & mask;
                        const int slot = map_find_rest(keys, cv, own, pos, keys[pos]);
                        const int v = id[slot >= 0 ? slot : 0];
                        const bool found = slot >= 0 && v >= 0 && v < V;
                        hit = relocalize_candidate(found, means[found ? v : 0], px, py, pz, r2);
                    }
                    const int c0 = (int)(own & ((1ull << VOXEL_AXIS_BITS) - 1ull)), c1 = (int)((own >> VOXEL_AXIS_BITS) & ((1ull << VOXEL_AXIS_BITS) - 1ull)),
                              c2 = (int)(own >> (2 * VOXEL_AXIS_BITS));
                    int d0 = -reach, d1 = -reach, d2 = -reach;     // the offset of the next cell of the cube, axis 0 fastest
                    for (int base = 0; base < cells && !hit; base += RELOC_BATCH) {
                        u64 key[RELOC_BATCH], cur[RELOC_BATCH];
                        unsigned pos[RELOC_BATCH];
                        int slot[RELOC_BATCH], v[RELOC_BATCH];
#pragma unroll
                        for (int k = 0; k < RELOC_BATCH; ++k) {    // stage 1: the first probe of every cell of the batch; the own cell is done
                            const int a0 = c0 + d0, a1 = c1 + d1, a2 = c2 + d2;
                            const bool wanted = base + k < cells && (d0 | d1 | d2) != 0 &&
                                                ((unsigned)a0 | (unsigned)a1 | (unsigned)a2) < (1u << VOXEL_AXIS_BITS);
                            key[k] = wanted ? voxel_key((u64)a0, (u64)a1, (u64)a2) : VOXEL_EMPTY;
                            pos[k] = wanted ? (unsigned)voxel_hash(key[k]) & mask : 0u;
                            cur[k] = keys[pos[k]];
                            if (++d0 > reach) { d0 = -reach; if (++d1 > reach) { d1 = -reach; ++d2; } }
                        }
#pragma unroll
                        for (int k = 0; k < RELOC_BATCH; ++k)      // stage 2: the rest of a chain; a cell that is not wanted has no slot
                            slot[k] = key[k] == VOXEL_EMPTY ? -1 : map_find_rest(keys, cv, key[k], pos[k], cur[k]);
#pragma unroll
                        for (int k = 0; k < RELOC_BATCH; ++k) v[k] = id[slot[k] >= 0 ? slot[k] : 0];      // stage 3
                        float4 s[RELOC_BATCH];
#pragma unroll
                        for (int k = 0; k < RELOC_BATCH; ++k) {    // stage 4: the row of the means table
                            if (!(slot[k] >= 0 && v[k] >= 0 && v[k] < V)) v[k] = -1;
                            s[k] = means[v[k] >= 0 ? v[k] : 0];
                        }
#pragma unroll
                        for (int k = 0; k < RELOC_BATCH; ++k) hit = hit | relocalize_candidate(v[k] >= 0, s[k], px, py, pz, r2);
                    }
                }
            }
            const u64 hits = __ballot(hit);
            if (hits != 0 && lane == 0) atomicAdd(&counts[p], (int)__popcll(hits));
        }
    }
}

PSAM_API size_t psam_relocalize_workspace_bytes(int32_t V) { return V > 0 && V <= MAP_MAX_POINTS ? (size_t)V * sizeof(float4) : 0; }

PSAM_API int32_t psam_relocalize_score(const void* map, size_t map_bytes, int32_t max_voxels, int32_t max_pairs, int32_t V, const uint64_t* skip,
                                       int32_t min_count, int32_t reach, float r2, const float* qry, int32_t M, const float* poses, int32_t P,
                                       int32_t* counts, void* ws, size_t ws_bytes, hipStream_t stream) {
    static const char* const name = "psam_relocalize_score";
    if (!(map && qry && poses && counts && ws)) return transfer_refuse(PSAM_EINVAL, name, "null pointer");
    if (!(M > 0 && M <= MAP_MAX_POINTS)) return transfer_refuse(PSAM_EINVAL, name, "need 0 < M <= 2^28");
    if (!map_caps_ok(max_voxels, max_pairs)) return transfer_refuse(PSAM_EINVAL, name, "need 0 < max_voxels <= 2^28 and 0 < max_pairs <= 2^28");
    if (!(V > 0 && V <= max_voxels)) return transfer_refuse(PSAM_EINVAL, name, "need 0 < V <= max_voxels");
    if (!(reach >= 1 && reach <= RELOC_MAX_REACH)) return transfer_refuse(PSAM_EINVAL, name, "need 1 <= reach <= 4");
    if (!(min_count >= 1)) return transfer_refuse(PSAM_EINVAL, name, "min_count must be at least 1");
    if (!(std::isfinite(r2) && r2 > 0.0f)) return transfer_refuse(PSAM_EINVAL, name, "r2 must be finite and positive");
    if (!(P > 0 && P <= RELOC_MAX_POSES)) return transfer_refuse(PSAM_EINVAL, name, "need 0 < P <= 2^20");
    if (!((((uintptr_t)map | (uintptr_t)ws) & 15) == 0 && ((uintptr_t)skip & 7) == 0 && (((uintptr_t)qry | (uintptr_t)poses | (uintptr_t)counts) & 3) == 0))
        return transfer_refuse(PSAM_EALIGN, name, "map and ws must be 16-byte aligned, skip 8-byte aligned, qry, poses and counts 4-byte aligned");
    if (map_bytes < map_layout(nullptr, max_voxels, max_pairs).bytes) return transfer_refuse(PSAM_EWORKSPACE, name, "map block too small (psam_map_bytes)");
    if (ws_bytes < psam_relocalize_workspace_bytes(V)) return transfer_refuse(PSAM_EWORKSPACE, name, "workspace too small (psam_relocalize_workspace_bytes)");
    if (hipMemsetAsync(counts, 0, (size_t)P * sizeof(int32_t), stream) != hipSuccess) {
        (void)hipGetLastError();
        psam_set_error("psam_relocalize_score: clearing counts failed");
        return PSAM_EINVAL;
    }
    const MapBlock b = map_layout((void*)map, max_voxels, max_pairs);
    hipLaunchKernelGGL(relocalize_means_kernel, dim3((unsigned)psam_cdiv(V, MAP_THREADS)), dim3(MAP_THREADS), 0, stream, (const u64*)b.rows, (int)V,
                       (const u64*)skip, (int)min_count, (float4*)ws);
    const int32_t st = psam_launch_status("psam_relocalize_score: means launch failed");
    if (st != PSAM_OK) return st;
    const int64_t chunks = psam_cdiv(P, RELOC_POSES);
    const dim3 grid((unsigned)psam_cdiv(M, RELOC_THREADS), (unsigned)(chunks < RELOC_MAX_GRID_Y ? chunks : RELOC_MAX_GRID_Y)), block(RELOC_THREADS);
    hipLaunchKernelGGL(relocalize_score_kernel, grid, block, 0, stream, (const int*)b.header, (const u64*)b.keys, (const int*)b.id, b.cv,
                       (const float4*)ws, (int)V, (int)reach, r2, qry, (int)M, poses, (int)P, (int*)counts);
    return psam_launch_status("psam_relocalize_score: launch failed");
}
