// Scan map normals (point_sam_amd/scanmap.py: ScanMap.normals): one surface normal and curvature per map voxel, from the map's own block.
//   psam_scanmap_normals   per voxel the exact integer scatter matrix of the MEANS of the allowed voxels in the (2 reach + 1)^3 cells around it,
//                          found by probing the map's own voxel table, and normals.hip's eigen-solve on it -- no cloud is read out of the map,
//                          nothing is voxelised again and no neighbour list is built
//
// Definition (include/pointsam_hip.h, "scan map normals"; tests/map_normals_reference.py states it again in numpy).  A voxel u is allowed iff u < V,
// count(u) >= min_count and its bit in `skip` is clear: track.hip's candidates without the radius.  The point of a voxel is its mean s (map_mean:
// psam_map_cloud's bits, what the tracker pairs with) in normals.hip's fixed point (map_fixed).  With n voxels, s = sum q and P = sum q q^T,
// S = n P - s s^T is an integer matrix and fits ONE signed 64-bit word per entry: n <= 125 and q <= 2^21 give P_ab <= 125 * 2^42 < 2^49,
// n P_ab < 2^56 and s_a s_b <= (125 * 2^21)^2 < 2^56.  No limbs, no atomics, no workspace; neither the order of the cube nor the schedule enters any
// output.  S goes to fp64 once (normal_to_double: round to nearest even), and from there on the code is normals.hip's (normal_eigen.h), with the sign
// rule that needs no viewpoint.
//
// Form.  One thread per voxel, and per cell of the cube track.hip's walk of dependent loads: key -> id -> row.  As there, the cube is taken
// MAPN_BATCH cells at a time and each stage is issued for the whole batch before the next stage consumes it; a cell that is off the grid or holds no
// voxel reads slot 0 / row 0 instead, in bounds and unused.  Every per-batch array is indexed by unrolled constants: nothing goes to scratch.
#include "map_block.h"
#include "normal_eigen.h"

constexpr int MAPN_THREADS = 256;
constexpr int MAPN_MAX_REACH = PSAM_SCANMAP_NORMALS_MAX_REACH;
constexpr int MAPN_BATCH = 9;                                      // reach 1: three batches of one 3 x 3 plane each; reach 2: fourteen, the last one cell short

__global__ __launch_bounds__(MAPN_THREADS) void map_normals_kernel(const u64* __restrict__ keys, const int* __restrict__ id, int cv, const u64* __restrict__ rows,
                                                                  const u64* __restrict__ key_of_id, int V, const u64* __restrict__ skip, int min_count,
                                                                  int reach, int min_voxels, int* __restrict__ count, double* __restrict__ scatter,
                                                                  float* __restrict__ normal, float* __restrict__ curvature) {
#pragma clang fp contract(off)
    const int self = blockIdx.x * MAPN_THREADS + threadIdx.x;
    if (self >= V) return;
    const u64 own = key_of_id[self];
    const u64 own_count = rows[(int64_t)self * MAP_ROW];
    const u64 own_word = skip ? skip[self >> 6] : 0ull;
    const bool allowed = own_count >= (u64)min_count && !((own_word >> (self & 63)) & 1ull);
    int n = 0;
    u64 s[3] = {0ull, 0ull, 0ull}, pr[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};      // xx, xy, xz, yy, yz, zz
    if (allowed) {
        const int c0 = (int)(own & ((1ull << VOXEL_AXIS_BITS) - 1ull)), c1 = (int)((own >> VOXEL_AXIS_BITS) & ((1ull << VOXEL_AXIS_BITS) - 1ull)),
                  c2 = (int)(own >> (2 * VOXEL_AXIS_BITS));
        const int w = 2 * reach + 1, cells = w * w * w;
        const unsigned mask = (unsigned)cv - 1u;
        int d0 = -reach, d1 = -reach, d2 = -reach;                 // the offset of the next cell of the cube, axis 0 fastest
        for (int base = 0; base < cells; base += MAPN_BATCH) {
            u64 key[MAPN_BATCH], cur[MAPN_BATCH];
            unsigned pos[MAPN_BATCH];
            int slot[MAPN_BATCH], v[MAPN_BATCH];
#pragma unroll
            for (int k = 0; k < MAPN_BATCH; ++k) {                 // stage 1: the first probe of every cell of the batch
                const int a0 = c0 + d0, a1 = c1 + d1, a2 = c2 + d2;
                const bool on_grid = base + k < cells && ((unsigned)a0 | (unsigned)a1 | (unsigned)a2) < (1u << VOXEL_AXIS_BITS);
                key[k] = on_grid ? voxel_key((u64)a0, (u64)a1, (u64)a2) : VOXEL_EMPTY;
                pos[k] = on_grid ? (unsigned)voxel_hash(key[k]) & mask : 0u;
                cur[k] = keys[pos[k]];
                if (++d0 > reach) { d0 = -reach; if (++d1 > reach) { d1 = -reach; ++d2; } }
            }
#pragma unroll
            for (int k = 0; k < MAPN_BATCH; ++k)                   // stage 2: the rest of a chain; a cell off the grid has no slot
                slot[k] = key[k] == VOXEL_EMPTY ? -1 : map_find_rest(keys, cv, key[k], pos[k], cur[k]);
#pragma unroll
            for (int k = 0; k < MAPN_BATCH; ++k) v[k] = id[slot[k] >= 0 ? slot[k] : 0];      // stage 3
            ulonglong2 lo[MAPN_BATCH], hi[MAPN_BATCH];
            u64 word[MAPN_BATCH];
#pragma unroll
            for (int k = 0; k < MAPN_BATCH; ++k) {                 // stage 4: count and the three sums of the position; the voxel's word of `skip`
                if (!(slot[k] >= 0 && v[k] >= 0 && v[k] < V)) v[k] = -1;
                const int at = v[k] >= 0 ? v[k] : 0;
                const ulonglong2* __restrict__ row = (const ulonglong2*)(rows + (int64_t)at * MAP_ROW);
                lo[k] = row[0];
                hi[k] = row[1];
                word[k] = skip ? skip[at >> 6] : 0ull;
            }
#pragma unroll
            for (int k = 0; k < MAPN_BATCH; ++k) {
                if (v[k] < 0 || lo[k].x < (u64)min_count || ((word[k] >> (v[k] & 63)) & 1ull)) continue;
                u64 q[3];
                if (!(map_fixed(map_mean(lo[k].y, lo[k].x), q[0]) & map_fixed(map_mean(hi[k].x, lo[k].x), q[1]) & map_fixed(map_mean(hi[k].y, lo[k].x), q[2])))
                    continue;                                      // a mean of accepted points lies in [-1, 1]: never taken
                n += 1;
                s[0] += q[0]; s[1] += q[1]; s[2] += q[2];
                pr[0] += q[0] * q[0]; pr[1] += q[0] * q[1]; pr[2] += q[0] * q[2];
                pr[3] += q[1] * q[1]; pr[4] += q[1] * q[2]; pr[5] += q[2] * q[2];
            }
        }
    }
    // S = n P - s s^T, exact in int64 (the bounds at the top)
    const int ia[6] = {0, 0, 0, 1, 1, 2}, ib[6] = {0, 1, 2, 1, 2, 2};
    double S[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) S[c] = normal_to_double((i128)((long long)((u64)n * pr[c]) - (long long)(s[ia[c]] * s[ib[c]])));
    count[self] = n;
    if (scatter) {
#pragma unroll
        for (int c = 0; c < 6; ++c) scatter[(int64_t)self * 6 + c] = S[c];
    }
    float out[3] = {0.0f, 0.0f, 0.0f}, curv = 0.0f;
    if (n >= min_voxels && n > 0) {
        normal_solve(S, out, curv);
        if (normal_flip_default(out)) { out[0] = -out[0]; out[1] = -out[1]; out[2] = -out[2]; }
    }
    normal[(int64_t)self * 3 + 0] = out[0]; normal[(int64_t)self * 3 + 1] = out[1]; normal[(int64_t)self * 3 + 2] = out[2];
    curvature[self] = curv;
}

PSAM_API int32_t psam_scanmap_normals(const void* map, size_t map_bytes, int32_t max_voxels, int32_t max_pairs, int32_t V, const uint64_t* skip, int32_t min_count,
                                      int32_t reach, int32_t min_voxels, int32_t* count, double* scatter, float* normal, float* curvature, hipStream_t stream) {
    PSAM_REQUIRE(map && count && normal && curvature, PSAM_EINVAL, "psam_scanmap_normals: null pointer");
    PSAM_REQUIRE(map_caps_ok(max_voxels, max_pairs), PSAM_EINVAL, "psam_scanmap_normals: need 0 < max_voxels <= 2^28 and 0 < max_pairs <= 2^28");
    PSAM_REQUIRE(V > 0 && V <= max_voxels, PSAM_EINVAL, "psam_scanmap_normals: need 0 < V <= max_voxels");
    PSAM_REQUIRE(reach >= 1 && reach <= MAPN_MAX_REACH, PSAM_EINVAL, "psam_scanmap_normals: need 1 <= reach <= 2");
    PSAM_REQUIRE(min_voxels >= 1, PSAM_EINVAL, "psam_scanmap_normals: min_voxels must be at least 1");
    PSAM_REQUIRE(min_count >= 1, PSAM_EINVAL, "psam_scanmap_normals: min_count must be at least 1");
    PSAM_REQUIRE(((uintptr_t)map & 15) == 0 && (((uintptr_t)skip | (uintptr_t)scatter) & 7) == 0 &&
                     (((uintptr_t)count | (uintptr_t)normal | (uintptr_t)curvature) & 3) == 0,
                 PSAM_EALIGN, "psam_scanmap_normals: map must be 16-byte aligned, skip and scatter 8-byte aligned, count, normal and curvature 4-byte aligned");
    PSAM_REQUIRE(map_bytes >= map_layout(nullptr, max_voxels, max_pairs).bytes, PSAM_EWORKSPACE, "psam_scanmap_normals: map block too small (psam_map_bytes)");
    const MapBlock b = map_layout((void*)map, max_voxels, max_pairs);
    hipLaunchKernelGGL(map_normals_kernel, dim3((unsigned)psam_cdiv(V, MAPN_THREADS)), dim3(MAPN_THREADS), 0, stream, (const u64*)b.keys, (const int*)b.id, b.cv,
                       (const u64*)b.rows, (const u64*)b.key_of_id, (int)V, (const u64*)skip, (int)min_count, (int)reach, (int)min_voxels, (int*)count, scatter,
                       normal, curvature);
    return psam_launch_status("psam_scanmap_normals: launch failed");
}
