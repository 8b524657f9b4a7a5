// Scan map carving (point_sam_amd/scanmap.py: ScanMap.carve): the cells between a sensor's origin and the points it measured are free space, and a
// map voxel that rays keep passing through is a ghost.  The definition is in include/pointsam_hip.h ("scan map carving"); tests/carve_reference.py
// states it again in numpy.  Everything here is integer set arithmetic over the map's voxel ids, so the result is a function of the inputs alone for
// any order of the points and the waves.
//
// The carve block (the caller's; psam_carve_bytes): 16 int32 header words (CARVE_H_* below), then one int4 per map voxel id: hits, misses, last_hit,
// last_missed.  The map block is only read: its header (inv_h, flags), its table keys / id.
//
// One carve = four launches, each a kernel boundary; the per-carve table is voxel_table.h's over the scan's own points in the workspace:
//   clear    the workspace table; the header's words of the last carve (4 .. 11)
//   insert   pose, acceptance, key (map_block.h's map_point); voxel_claim_run: rep[i] = the workspace slot, low[slot] = the key's lowest point index --
//            the deduplication of the rays.  One thread puts the origin through the same arithmetic and leaves its key in the workspace, and
//            advances the header's carve count and stamp
//   mark     the lowest point of each key asks the map's table; a voxel found is hit: atomicMax(last_hit, stamp), and the winner increments hits.
//            A key other than the origin's is a ray: its slot is appended to the ray list (one atomic per block of 1024; the list's order depends on the
//            arrival of the blocks, what is done per ray does not)
//   walk     one thread per entry of the ray list walks its ray (carve_walk below), so the lanes of a wave all walk -- in a raster-ordered scan
//            most points share their cell with a neighbour and only one in tens begins a ray; a crossed map voxel beyond the margin whose
//            last_hit is not this stamp is missed: atomicMax(last_missed, stamp), and the winner increments misses
// A dead map (flags != 0) is neither marked nor walked.
//
// The walk.  With n_a = |e_a - o_a| the ray leaves its cell along axis a for the (k_a + 1)-th time at t_a = (2 k_a + 1) / (2 n_a); the next crossing
// is the least t_a, and axes tied there step together (the segment passes through an edge or a corner and touches, but does not cross, the cells
// beside it).  The comparison t_a < t_b is (2 k_a + 1) n_b < (2 k_b + 1) n_a; the kernel keeps the three differences
//   D_ab = (2 k_a + 1) n_b - (2 k_b + 1) n_a          |D_ab| < 2^43: int64, exact
// and a step of axis a adds 2 n_b to D_ab and 2 n_c to D_ac: no multiplication in the loop, and no 32-bit variant of it to choose between.  An axis
// with n_a = 0 has D_ab = n_b > 0 against every axis that moves, and an axis that has arrived (k_a = n_a) has t_a > 1 > t_b of every axis that has
// not: neither is ever stepped, without a test of its own.  k, n, cur and D are named scalars updated by selects: nothing is indexed by "the best
// axis", so nothing goes to scratch.  The Chebyshev distance to the end cell never grows along the walk, so the walk ends where it first is <= margin.
//
// One thread per ray is what is built.  The other form -- a prefix sum over the rays' longest-axis lengths, threads taking fixed chunks of crossings and
// entering a ray by the closed form of the header -- is not built; DESIGN.md 4.18 says what this one measures.
#include "map_block.h"

#include <climits>
#include <cmath>

constexpr int CARVE_HEADER_INTS = 16;
// header words (int32), word 0 = max_voxels (carve_init_kernel); 10, 11: crossed cells beyond the margin, one u64
constexpr int CARVE_H_CARVES = 1, CARVE_H_STAMP = 2, CARVE_H_ORIGIN = 3, CARVE_H_RAYS = 4, CARVE_H_ACCEPTED = 5, CARVE_H_REJECTED = 6, CARVE_H_HIT = 7,
              CARVE_H_MISSED = 8, CARVE_H_CROSSED = 10;
constexpr int CARVE_LAST_WORDS = 8;                // words 4 .. 11 are of the last carve: zeroed by the clear launch
constexpr int CARVE_MAX_MARGIN = 1 << VOXEL_AXIS_BITS;
static_assert(CARVE_HEADER_INTS == PSAM_CARVE_HEADER_INTS, "header size");

struct CarveWs {
    VoxelWs table;       // keys, low, rep of voxel_table.h over the scan's M points (no block counts: nothing is ranked)
    int* rays;           // [M]: the workspace slots of the rays' end cells; their number is the header's CARVE_H_RAYS
    u64* origin;         // [2]: the origin's key (VOXEL_EMPTY: it has no cell), spare
    size_t bytes;
};

static inline CarveWs carve_ws_layout(void* ws, int64_t M) {
    CarveWs w = {};
    w.table = voxel_layout(ws, M, false, false);
    size_t o = w.table.bytes;
    w.table.rep = (int*)((char*)ws + o);   o += align16((size_t)M * sizeof(int));
    w.rays = (int*)((char*)ws + o);        o += align16((size_t)M * sizeof(int));
    w.origin = (u64*)((char*)ws + o);      o += 16;
    w.bytes = o;
    return w;
}

struct CarveOrigin {
    float v[3];
};

static inline bool carve_voxels_ok(int64_t max_voxels) { return max_voxels > 0 && max_voxels <= MAP_MAX_POINTS; }

// ------------------------------------------------------------------------------------------------ clear
__global__ __launch_bounds__(MAP_THREADS) void carve_init_kernel(uint4* __restrict__ block, int64_t granules, int max_voxels) {
    const int64_t stride = (int64_t)gridDim.x * MAP_THREADS;
    for (int64_t g = (int64_t)blockIdx.x * MAP_THREADS + threadIdx.x; g < granules; g += stride)
        block[g] = make_uint4(g == 0 ? (unsigned)max_voxels : 0u, 0u, 0u, 0u);      // granule 0 begins with header word 0
}

// ------------------------------------------------------------------------------------------------ insert
template <bool POSED>
__global__ __launch_bounds__(MAP_THREADS) void carve_insert_kernel(const float* __restrict__ xyz, int M, RigidPose P, CarveOrigin origin, int stamp,
                                                                   const int* __restrict__ map_header, u64* __restrict__ keys, unsigned* __restrict__ low,
                                                                   int capacity, int* __restrict__ rep, u64* __restrict__ origin_key, int* __restrict__ header) {
    const int i = blockIdx.x * MAP_THREADS + threadIdx.x;      // whole waves stay in the kernel: voxel_claim_run needs every lane
    const float inv_h = map_inv_h(map_header);
    u64 key = VOXEL_EMPTY;
    if (i < M) {
        u64 q[3], k;
        if (map_point<POSED>(xyz, i, P, inv_h, q, k)) key = k;
    }
    const int slot = voxel_claim_run(keys, low, capacity, key, i);      // 2 M slots for at most M keys: never -1 for a key
    if (i < M) rep[i] = slot;
    const u64 accepted = __ballot(key != VOXEL_EMPTY);
    if ((threadIdx.x & 63) == 0 && accepted) atomicAdd(&header[CARVE_H_ACCEPTED], __popcll(accepted));
    if (i != 0) return;
    u64 q[3], k = VOXEL_EMPTY;
    const bool have = map_point<POSED>(origin.v, 0, P, inv_h, q, k);
    origin_key[0] = have ? k : VOXEL_EMPTY;
    header[CARVE_H_ORIGIN] = have ? 1 : 0;
    header[CARVE_H_REJECTED] = M;                                  // the mark launch takes the accepted points off
    if (stamp > header[CARVE_H_STAMP]) {                           // the same stamp again is the same carve again
        header[CARVE_H_STAMP] = stamp;
        header[CARVE_H_CARVES] = header[CARVE_H_CARVES] + 1;
    }
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// ------------------------------------------------------------------------------------------------ mark
// Blocks of SCAN_THREADS: the rays of a block take their places in the list by voxel_table.h's ballot scan behind ONE atomic on the header's ray count.
// (One atomic per wave was the first form: 156 000 returning atomics on one word made this launch 3.06 ms of a 6.45 ms carve at 10^7 points.)
__global__ __launch_bounds__(SCAN_THREADS) void carve_mark_kernel(const int* __restrict__ rep, const unsigned* __restrict__ low, const u64* __restrict__ ws_keys,
                                                                 int M, const u64* __restrict__ origin_key, const int* __restrict__ map_header,
                                                                 const u64* __restrict__ keys, const int* __restrict__ id, int cv, int max_voxels, int stamp,
                                                                 int* __restrict__ header, int* __restrict__ rows, int* __restrict__ rays) {
    __shared__ int s_cnt[SCAN_WAVES], s_hit[SCAN_WAVES], s_base;
    const int i = blockIdx.x * SCAN_THREADS + threadIdx.x, lane = threadIdx.x & 63;
    // The lowest index of a key is the first lane of its run of equal slots (a run's first lane has the run's lowest index, and lane 0 begins a
    // run), so only a run's first lane asks low[]: a coalesced read of rep[] for all, a scattered one per run -- in raster order, per tens of points.
    const int slot = i < M ? rep[i] : -1;
    const int before = __shfl_up(slot, 1, 64);
    int hit = 0;
    bool ray = false;
    if ((lane == 0 || before != slot) && slot >= 0 && low[slot] == (unsigned)i) {
        const u64 key = ws_keys[slot], okey = origin_key[0];
        ray = okey != VOXEL_EMPTY && key != okey;
        if (map_header[MAP_H_FLAGS] == 0) {
            const int at = voxel_find(keys, cv, key);
            const int v = at >= 0 ? id[at] : -1;
            if (v >= 0 && v < max_voxels && atomicMax(&rows[(int64_t)v * 4 + 2], stamp) < stamp) {
                atomicAdd(&rows[(int64_t)v * 4 + 0], 1);
                hit = 1;
            }
        }
    }
    const u64 ray_lanes = scan_note(ray, s_cnt);
    hit = wave_sum_i32(hit);
    if (lane == 0) s_hit[threadIdx.x >> 6] = hit;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int block_rays = scan_total(s_cnt), block_hits = scan_total(s_hit);
        s_base = block_rays ? atomicAdd(&header[CARVE_H_RAYS], block_rays) : 0;      // at most M rays in all: the list holds M
        if (block_hits) atomicAdd(&header[CARVE_H_HIT], block_hits);
        if (i == 0) atomicSub(&header[CARVE_H_REJECTED], header[CARVE_H_ACCEPTED]);      // accepted was complete a kernel boundary ago
    }
    __syncthreads();
    if (ray) rays[scan_rank(ray_lanes, s_cnt, s_base)] = slot;
}

// ------------------------------------------------------------------------------------------------ walk
// The crossed cells of the ray from cell `okey` to cell `ekey` whose Chebyshev distance to the end is > margin: each is looked up in the map, and a
// voxel found that was not hit in this carve is missed.  -> the number of such cells; `missed` counts the voxels this thread was the first to miss.
__device__ __forceinline__ unsigned carve_walk(u64 okey, u64 ekey, int margin, int stamp, const u64* __restrict__ keys, const int* __restrict__ id, int cv,
                                               int max_voxels, int* __restrict__ rows, int& missed) {
    constexpr u64 AXIS = (1ull << VOXEL_AXIS_BITS) - 1ull;
    const int d0 = (int)(ekey & AXIS) - (int)(okey & AXIS), d1 = (int)((ekey >> VOXEL_AXIS_BITS) & AXIS) - (int)((okey >> VOXEL_AXIS_BITS) & AXIS),
              d2 = (int)(ekey >> (2 * VOXEL_AXIS_BITS)) - (int)(okey >> (2 * VOXEL_AXIS_BITS));
    const long long n0 = d0 < 0 ? -d0 : d0, n1 = d1 < 0 ? -d1 : d1, n2 = d2 < 0 ? -d2 : d2;
    // a step of an axis moves the key by +-1, +-2^21, +-2^42: two's complement, the fields never borrow because every cell stays inside the box of o and e
    const u64 s0 = d0 < 0 ? ~0ull : 1ull, s1 = (d1 < 0 ? ~0ull : 1ull) << VOXEL_AXIS_BITS, s2 = (d2 < 0 ? ~0ull : 1ull) << (2 * VOXEL_AXIS_BITS);
    int r0 = (int)n0, r1 = (int)n1, r2 = (int)n2;                  // crossings left per axis: n_a - k_a
    long long D01 = n1 - n0, D02 = n2 - n0, D12 = n2 - n1;         // k = 0
    u64 cur = okey;
    unsigned crossed = 0;
    const int steps = r0 + r1 + r2;                                // every trip steps at least one axis: the loop is bounded whatever else
    for (int trip = 0; trip < steps; ++trip) {
        const bool t0 = D01 <= 0 && D02 <= 0, t1 = D01 >= 0 && D12 <= 0, t2 = D02 >= 0 && D12 >= 0;
        cur += (t0 ? s0 : 0ull) + (t1 ? s1 : 0ull) + (t2 ? s2 : 0ull);
        r0 -= t0; r1 -= t1; r2 -= t2;
        D01 += (t0 ? 2 * n1 : 0ll) - (t1 ? 2 * n0 : 0ll);
        D02 += (t0 ? 2 * n2 : 0ll) - (t2 ? 2 * n0 : 0ll);
        D12 += (t1 ? 2 * n2 : 0ll) - (t2 ? 2 * n1 : 0ll);
        if (max(r0, max(r1, r2)) <= margin) break;                 // includes the end cell itself: all three are 0 there
        ++crossed;
        const int at = voxel_find(keys, cv, cur);
        if (at < 0) continue;
        const int v = id[at];
        if (v < 0 || v >= max_voxels) continue;
        int* __restrict__ row = rows + (int64_t)v * 4;
        if (row[2] == stamp) continue;                             // hit in this carve: the mark launch ended a kernel boundary ago
        if (__hip_atomic_load(&row[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= stamp) continue;      // a stale value only costs the atomic below
        if (atomicMax(&row[3], stamp) < stamp) {
            atomicAdd(&row[1], 1);
            ++missed;
        }
    }
    return crossed;
}

__global__ __launch_bounds__(MAP_THREADS) void carve_walk_kernel(const int* __restrict__ rays, const u64* __restrict__ ws_keys, int capacity,
                                                                 const u64* __restrict__ origin_key, const int* __restrict__ map_header,
                                                                 const u64* __restrict__ keys, const int* __restrict__ id, int cv, int max_voxels, int margin,
                                                                 int stamp, int* __restrict__ header, int* __restrict__ rows) {
    const int r = blockIdx.x * MAP_THREADS + threadIdx.x;
    const u64 okey = origin_key[0];
    const int count = header[CARVE_H_RAYS];                         // complete a kernel boundary ago; this kernel does not write it
    if (okey == VOXEL_EMPTY || map_header[MAP_H_FLAGS] != 0 || (int)(blockIdx.x * MAP_THREADS) >= count) return;      // uniform over the block
    int missed = 0;
    unsigned crossed = 0;
    if (r < count) {
        const int slot = rays[r];
        if (slot >= 0 && slot < capacity) {
            const u64 ekey = ws_keys[slot];
            if (ekey != okey && ekey != VOXEL_EMPTY) crossed = carve_walk(okey, ekey, margin, stamp, keys, id, cv, max_voxels, rows, missed);
        }
    }
    // a wave's rays cross fewer than 64 * 3 * 2^21 < 2^30 cells
    const int wave_crossed = wave_sum_i32((int)crossed), wave_missed = wave_sum_i32(missed);
    if ((threadIdx.x & 63) != 0) return;
    if (wave_crossed) atomicAdd((u64*)&header[CARVE_H_CROSSED], (u64)wave_crossed);
    if (wave_missed) atomicAdd(&header[CARVE_H_MISSED], wave_missed);
}

// ------------------------------------------------------------------------------------------------ read-out
__global__ __launch_bounds__(MAP_THREADS) void carve_fields_kernel(const int4* __restrict__ rows, int V, int* __restrict__ hits, int* __restrict__ misses,
                                                                   int* __restrict__ last_hit, int* __restrict__ last_missed) {
    const int v = blockIdx.x * MAP_THREADS + threadIdx.x;
    if (v >= V) return;
    const int4 r = rows[v];
    if (hits) hits[v] = r.x;
    if (misses) misses[v] = r.y;
    if (last_hit) last_hit[v] = r.z;
    if (last_missed) last_missed[v] = r.w;
}

// ------------------------------------------------------------------------------------------------ entries
static inline unsigned carve_blocks(int64_t n) { return (unsigned)psam_cdiv(n, MAP_THREADS); }

PSAM_API size_t psam_carve_bytes(int32_t max_voxels) {
    if (!carve_voxels_ok(max_voxels)) return 0;
    return CARVE_HEADER_INTS * sizeof(int) + (size_t)max_voxels * 16;
}

PSAM_API size_t psam_carve_workspace_bytes(int32_t M) {
    if (M <= 0 || M > MAP_MAX_POINTS) return 0;
    return carve_ws_layout(nullptr, M).bytes;
}

#define CARVE_REQUIRE_BLOCK(name)                                                                                                                       \
    PSAM_REQUIRE(carve_voxels_ok(max_voxels), PSAM_EINVAL, name ": need 0 < max_voxels <= 2^28");                                                      \
    PSAM_REQUIRE(carve_bytes >= psam_carve_bytes(max_voxels), PSAM_EWORKSPACE, name ": carve block too small (psam_carve_bytes)");                     \
    PSAM_REQUIRE(((uintptr_t)carve & 15) == 0, PSAM_EALIGN, name ": carve block must be 16-byte aligned")

PSAM_API int32_t psam_carve_clear(void* carve, size_t carve_bytes, int32_t max_voxels, hipStream_t stream) {
    PSAM_REQUIRE(carve, PSAM_EINVAL, "psam_carve_clear: null pointer");
    CARVE_REQUIRE_BLOCK("psam_carve_clear");
    const int64_t granules = (int64_t)(psam_carve_bytes(max_voxels) / 16);
    hipLaunchKernelGGL(carve_init_kernel, dim3((unsigned)(granules < 4096 * MAP_THREADS ? psam_cdiv(granules, MAP_THREADS) : 4096)), dim3(MAP_THREADS), 0, stream,
                       (uint4*)carve, granules, (int)max_voxels);
    return psam_launch_status("psam_carve_clear: launch failed");
}

PSAM_API int32_t psam_carve_scan(const void* map, size_t map_bytes, int32_t max_voxels, int32_t max_pairs, void* carve, size_t carve_bytes, const float* xyz,
                                 int32_t M, const float* pose, const float* origin, int32_t margin, int32_t stamp, void* ws, size_t ws_bytes,
                                 hipStream_t stream) {
    PSAM_REQUIRE(map && carve && xyz && origin && ws, PSAM_EINVAL, "psam_carve_scan: null pointer");
    PSAM_REQUIRE(M > 0 && M <= MAP_MAX_POINTS, PSAM_EINVAL, "psam_carve_scan: need 0 < M <= 2^28");
    PSAM_REQUIRE(margin >= 0 && margin < CARVE_MAX_MARGIN, PSAM_EINVAL, "psam_carve_scan: need 0 <= margin < 2^21");
    PSAM_REQUIRE(stamp >= 1, PSAM_EINVAL, "psam_carve_scan: need 1 <= stamp <= 2^31 - 1");
    PSAM_REQUIRE(map_caps_ok(max_voxels, max_pairs), PSAM_EINVAL, "psam_carve_scan: need 0 < max_voxels <= 2^28 and 0 < max_pairs <= 2^28");
    PSAM_REQUIRE(map_bytes >= map_layout(nullptr, max_voxels, max_pairs).bytes, PSAM_EWORKSPACE, "psam_carve_scan: map block too small (psam_map_bytes)");
    PSAM_REQUIRE(((uintptr_t)map & 15) == 0, PSAM_EALIGN, "psam_carve_scan: map block must be 16-byte aligned");
    CARVE_REQUIRE_BLOCK("psam_carve_scan");
    RigidPose P = {};
    PSAM_REQUIRE(!pose || pose_load(pose, P), PSAM_EINVAL, "psam_carve_scan: pose must be finite");
    PSAM_REQUIRE(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]), PSAM_EINVAL, "psam_carve_scan: origin must be finite");
    PSAM_REQUIRE(ws_bytes >= psam_carve_workspace_bytes(M), PSAM_EWORKSPACE, "psam_carve_scan: workspace too small (psam_carve_workspace_bytes)");
    PSAM_REQUIRE(((uintptr_t)ws & 15) == 0, PSAM_EALIGN, "psam_carve_scan: workspace must be 16-byte aligned");
    const MapBlock b = map_layout((void*)map, max_voxels, max_pairs);
    const CarveWs w = carve_ws_layout(ws, M);
    int* header = (int*)carve;
    int* rows = header + CARVE_HEADER_INTS;
    const CarveOrigin o = {{origin[0], origin[1], origin[2]}};
    const int capacity = (int)voxel_capacity(M);
    const unsigned blocks = carve_blocks(M);
    int32_t st = voxel_clear<CARVE_LAST_WORDS>(w.table, header + CARVE_H_RAYS, stream, "psam_carve_scan: clear launch failed");
    if (st != PSAM_OK) return st;
    auto insert = pose ? carve_insert_kernel<true> : carve_insert_kernel<false>;
    hipLaunchKernelGGL(insert, dim3(blocks), dim3(MAP_THREADS), 0, stream, xyz, (int)M, P, o, (int)stamp, (const int*)b.header, w.table.keys, w.table.low,
                       capacity, w.table.rep, w.origin, header);
    if ((st = psam_launch_status("psam_carve_scan: insert launch failed")) != PSAM_OK) return st;
    hipLaunchKernelGGL(carve_mark_kernel, dim3((unsigned)scan_blocks(M)), dim3(SCAN_THREADS), 0, stream, (const int*)w.table.rep, (const unsigned*)w.table.low,
                       (const u64*)w.table.keys, (int)M, (const u64*)w.origin, (const int*)b.header, (const u64*)b.keys, (const int*)b.id, b.cv,
                       (int)max_voxels, (int)stamp, header, rows, w.rays);
    if ((st = psam_launch_status("psam_carve_scan: mark launch failed")) != PSAM_OK) return st;
    hipLaunchKernelGGL(carve_walk_kernel, dim3(blocks), dim3(MAP_THREADS), 0, stream, (const int*)w.rays, (const u64*)w.table.keys, capacity, (const u64*)w.origin, (const int*)b.header, (const u64*)b.keys, (const int*)b.id, b.cv,
                       (int)max_voxels, (int)margin, (int)stamp, header, rows);
    return psam_launch_status("psam_carve_scan: walk launch failed");
}

PSAM_API int32_t psam_carve_fields(const void* carve, size_t carve_bytes, int32_t max_voxels, int32_t V, int32_t* hits, int32_t* misses, int32_t* last_hit,
                                   int32_t* last_missed, hipStream_t stream) {
    PSAM_REQUIRE(carve && (hits || misses || last_hit || last_missed), PSAM_EINVAL, "psam_carve_fields: null pointer");
    CARVE_REQUIRE_BLOCK("psam_carve_fields");
    PSAM_REQUIRE(V > 0 && V <= max_voxels, PSAM_EINVAL, "psam_carve_fields: need 0 < V <= max_voxels");
    hipLaunchKernelGGL(carve_fields_kernel, dim3(carve_blocks(V)), dim3(MAP_THREADS), 0, stream, (const int4*)((const int*)carve + CARVE_HEADER_INTS), (int)V, hits,
                       misses, last_hit, last_missed);
    return psam_launch_status("psam_carve_fields: launch failed");
}
