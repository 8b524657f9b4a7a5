// Scan maps (point_sam_amd/scanmap.py): posed scans accumulate into one persistent, labelled voxel map in the normalised frame.  A map voxel is the
// voxel of psam_voxel_downsample at origin (-1, -1, -1) (csrc/voxel_cell.h), the pose arithmetic is csrc/rigid_pose.h's, and positions and colours
// are summed in the fixed point of normals.hip, q = floor((double)v * 2^20) + 2^20: every sum is an integer, so every output is the same bits for
// any arrival order of the waves.
//
// The map block (the caller's; psam_map_bytes):
//   header    16 int32, MAP_H_* below
//   table     keys [Cv] u64 and id [Cv] int32, Cv = voxel_capacity(max_voxels): key -> permanent id.  A key enters it only in the rank pass, after
//             the add's new voxels were counted against max_voxels, so it never holds more than max_voxels keys: load factor <= 0.5, every probe ends
//   pairs     keys [Cp] u64 = (id << 32) | label and count [Cp] u32, Cp = voxel_capacity(max_pairs)
//   rows      [max_voxels, 8] u64: count, sum q (3), sum c (3), then first_seen and last_seen as two int32
//   best      [max_voxels] u64: the maximum over the voxel's pairs of (count << 32) | ~label -- the highest count, on a tie the LOWER label.  A
//             pair's count only grows, so the maximum over every value a pair ever had is the maximum over the final values: it is kept by one atomic
//             maximum beside the pair's increment, and psam_map_labels unpacks it without a pass over the pair table
//   key_of_id [max_voxels] u64
//
// No overflow.  An add is refused (MAP_FLAG_COUNTS) where it would take the map's accepted observations past 2^31 - 1, so for every map
//   count <= 2^31 - 1 (an int32, as are the votes)          q <= 2^21: sum q <= 2^52 (one u64 word)          a pair's count <= 2^31 - 1 (one u32 word)
//
// One add = six launches, each a kernel boundary; the per-add table is voxel_table.h's, over the add's own points in the workspace:
//   clear       the workspace table, the add's counters
//   insert      pose, acceptance, key; voxel_claim_run: rep[i] = the workspace slot (-1: rejected), low[slot] = the key's lowest point index
//   look-up     the point with the lowest index of each key asks the map's table: wid[slot] = the voxel's id, or -1 for a voxel new in this add;
//               new voxels are counted per block
//   offsets     scan_block_offsets; one thread checks the capacities, raises the flags and advances the header
//   rank        a new voxel's id = V_before + its rank (new ids follow the lowest point index); its key enters the map's table.  Not under a flag
//   accumulate  one thread per point: ids[i]; per run of equal voxels on consecutive lanes seven integer atomic adds into the voxel's row and
//               last_seen; per run of equal (voxel, label >= 0) the pair's claim, its increment and the voxel's best word.  A pair whose count was 0
//               is new: past max_pairs it raises MAP_FLAG_PAIRS, and every wave that sees a flag stops, so a full pair table (whose probe ends
//               bounded, voxel_claim) is only ever met under overflow
// Both overflow conditions are functions of the inputs alone: the number of distinct keys, and of distinct (id, label) pairs.
#include "map_block.h"       // the block, its header and a point's way into it; with rigid_pose.h and voxel_table.h

#include <climits>
#include <cmath>

struct MapAddWs {
    VoxelWs table;       // keys, low, rep, block of voxel_table.h over the add's M points
    int* wid;            // [C]: per workspace slot the voxel's id
    int* counter;        // [4]: accepted, new, V before the add, spare
    size_t bytes;
};
constexpr int MAP_C_ACCEPTED = 0, MAP_C_NEW = 1, MAP_C_VBEFORE = 2;

static inline MapAddWs map_add_layout(void* ws, int64_t M) {
    MapAddWs w = {};
    w.table = voxel_layout(ws, M, true, false);
    size_t o = w.table.bytes;
    w.wid = (int*)((char*)ws + o);         o += align16((size_t)voxel_capacity(M) * sizeof(int));
    w.counter = (int*)((char*)ws + o);     o += align16(4 * sizeof(int));
    w.bytes = o;
    return w;
}

__device__ __forceinline__ bool map_colour(const float* __restrict__ rgb, int64_t i, u64 (&c)[3]) {
    return map_fixed(rgb[i * 3 + 0], c[0]) & map_fixed(rgb[i * 3 + 1], c[1]) & map_fixed(rgb[i * 3 + 2], c[2]);
}

// ------------------------------------------------------------------------------------------------ init
__global__ __launch_bounds__(MAP_THREADS) void map_init_kernel(int* __restrict__ header, int max_voxels, int max_pairs, float inv_h, uint4* __restrict__ zero,
                                                               int64_t granules) {
    const int64_t stride = (int64_t)gridDim.x * MAP_THREADS;
    for (int64_t g = (int64_t)blockIdx.x * MAP_THREADS + threadIdx.x; g < granules; g += stride) zero[g] = make_uint4(0u, 0u, 0u, 0u);
    if (blockIdx.x == 0 && threadIdx.x < MAP_HEADER_INTS) {
        const int t = threadIdx.x;
        header[t] = t == MAP_H_MAX_VOXELS ? max_voxels : t == MAP_H_MAX_PAIRS ? max_pairs : t == MAP_H_INV_H ? __builtin_bit_cast(int, inv_h) : 0;
    }
}

// ------------------------------------------------------------------------------------------------ add
template <bool POSED>
__global__ __launch_bounds__(MAP_THREADS) void map_insert_kernel(const float* __restrict__ xyz, const float* __restrict__ rgb, int M, RigidPose P,
                                                                 const int* __restrict__ header, u64* __restrict__ keys, unsigned* __restrict__ low,
                                                                 int capacity, int* __restrict__ rep, int* __restrict__ counter) {
    const int i = blockIdx.x * MAP_THREADS + threadIdx.x;      // whole waves stay in the kernel: voxel_claim_run needs every lane
    u64 key = VOXEL_EMPTY;
    if (i < M) {
        u64 q[3], c[3], k;
        if (map_point<POSED>(xyz, i, P, map_inv_h(header), q, k) & map_colour(rgb, i, c)) key = k;
    }
    const int slot = voxel_claim_run(keys, low, capacity, key, i);      // the add's own table holds 2 M slots for at most M keys: never -1 for a key
    if (i < M) rep[i] = slot;
    const u64 accepted = __ballot(key != VOXEL_EMPTY);
    if ((threadIdx.x & 63) == 0 && accepted) atomicAdd(&counter[MAP_C_ACCEPTED], __popcll(accepted));
}

// whether point i is the lowest index of its key in this add, and then its workspace slot
__device__ __forceinline__ bool map_first_of_key(const int* __restrict__ rep, const unsigned* __restrict__ low, int M, int i, int& slot) {
    if (i >= M) return false;
    slot = rep[i];
    return slot >= 0 && low[slot] == (unsigned)i;
}

__global__ __launch_bounds__(SCAN_THREADS) void map_lookup_kernel(const int* __restrict__ rep, const unsigned* __restrict__ low, const u64* __restrict__ ws_keys,
                                                                 int M, const u64* __restrict__ keys, const int* __restrict__ id, int cv,
                                                                 int* __restrict__ wid, int* __restrict__ block_count) {
    __shared__ int s_cnt[SCAN_WAVES];
    const int i = blockIdx.x * SCAN_THREADS + threadIdx.x;
    int slot;
    bool fresh = false;
    if (map_first_of_key(rep, low, M, i, slot)) {
        const int m = voxel_find(keys, cv, ws_keys[slot]);
        const int v = m >= 0 ? id[m] : -1;
        wid[slot] = v;
        fresh = v < 0;
    }
    scan_note(fresh, s_cnt);
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = scan_total(s_cnt);
}

__global__ __launch_bounds__(SCAN_THREADS) void map_offsets_kernel(int* __restrict__ block, int blocks, int M, int* __restrict__ counter, int* __restrict__ header) {
    int lo, hi, c = 0;
    scan_span(blocks, threadIdx.x, lo, hi);
    for (int b = lo; b < hi; ++b) c += block[b];
    scan_block_offsets(block, blocks, lo, hi, c, &counter[MAP_C_NEW]);
    if (threadIdx.x != SCAN_THREADS - 1) return;                   // the thread that wrote the total
    const int fresh = block[blocks], accepted = counter[MAP_C_ACCEPTED], V = header[MAP_H_V];
    u64* observed = (u64*)&header[MAP_H_OBSERVED];
    int flags = header[MAP_H_FLAGS];
    if ((int64_t)V + fresh > header[MAP_H_MAX_VOXELS]) flags |= MAP_FLAG_VOXELS;
    if (*observed + (u64)accepted > (u64)INT_MAX || header[MAP_H_ADDS] == INT_MAX) flags |= MAP_FLAG_COUNTS;
    counter[MAP_C_VBEFORE] = V;
    header[MAP_H_FLAGS] = flags;
    header[MAP_H_NEW] = fresh;
    header[MAP_H_ACCEPTED] = accepted;
    header[MAP_H_REJECTED] = M - accepted;
    if (flags) return;
    header[MAP_H_V] = V + fresh;
    header[MAP_H_ADDS] = header[MAP_H_ADDS] + 1;
    *observed = *observed + (u64)accepted;
}

__global__ __launch_bounds__(SCAN_THREADS) void map_rank_kernel(const int* __restrict__ rep, const unsigned* __restrict__ low, const u64* __restrict__ ws_keys,
                                                               int M, const int* __restrict__ block_offset, const int* __restrict__ counter,
                                                               int* __restrict__ header, u64* __restrict__ keys, int* __restrict__ id, int cv,
                                                               u64* __restrict__ rows, u64* __restrict__ key_of_id, int* __restrict__ wid) {
    __shared__ int s_cnt[SCAN_WAVES];
    const int i = blockIdx.x * SCAN_THREADS + threadIdx.x;
    int slot = -1;
    const bool fresh = map_first_of_key(rep, low, M, i, slot) && wid[slot] < 0;
    const u64 m = scan_note(fresh, s_cnt);
    __syncthreads();
    if (!fresh || header[MAP_H_FLAGS]) return;                     // the flags were last written a kernel boundary ago
    const int v = counter[MAP_C_VBEFORE] + scan_rank(m, s_cnt, block_offset[blockIdx.x]);      // < max_voxels: the offsets pass checked the total
    const u64 key = ws_keys[slot];
    const int at = voxel_claim(keys, cv, key);                     // the map's table holds at most max_voxels of its >= 2 max_voxels slots
    if (at < 0) { atomicOr(&header[MAP_H_FLAGS], MAP_FLAG_VOXELS); return; }
    id[at] = v;
    wid[slot] = v;                                                 // only this thread touches wid[slot] in this kernel
    key_of_id[v] = key;
    ((int*)&rows[(int64_t)v * MAP_ROW + 7])[0] = header[MAP_H_ADDS];      // first_seen
}

// Scans arrive in raster order, so consecutive lanes often share a voxel: a run of equal voxels on consecutive lanes is summed inside the wave (a
// segmented suffix sum by shuffles; a wave's sum of q stays below 64 * 2^21 = 2^27, one 32-bit word) and its first lane issues the seven atomics for
// all of it; a run of equal (voxel, label) pairs is one claim, one increment by its length and one maximum.  Integer sums: the same bits as one
// atomic per point, the form this replaced after it measured slower (scan maps).  Whole waves stay in the kernel.
__device__ __forceinline__ int map_run_length(u64 leaders, int lane) {
    const u64 above = leaders & ~((2ull << lane) - 1ull);          // lane 63: 2 << 63 wraps to 0, the mask to all ones, `above` to 0
    return (above ? __builtin_ctzll(above) : 64) - lane;
}

template <bool POSED>
__global__ __launch_bounds__(MAP_THREADS) void map_accumulate_kernel(const float* __restrict__ xyz, const float* __restrict__ rgb,
                                                                          const int* __restrict__ labels, int M, RigidPose P, const int* __restrict__ rep,
                                                                          const int* __restrict__ wid, int* __restrict__ header, u64* __restrict__ rows,
                                                                          u64* __restrict__ pair_keys, unsigned* __restrict__ pair_count, int cp,
                                                                          u64* __restrict__ best, int* __restrict__ ids) {
    const int i = blockIdx.x * MAP_THREADS + threadIdx.x, lane = threadIdx.x & 63;
    const int slot = i < M ? rep[i] : -1;
    if (i < M && slot < 0) ids[i] = -1;
    const bool dead = __ballot(__hip_atomic_load(&header[MAP_H_FLAGS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) != 0ull;      // one answer per wave
    int v = -1, label = -1;
    unsigned w[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    if (slot >= 0 && !dead) {
        v = wid[slot];
        ids[i] = v;
        u64 q[3], c[3], key;
        map_point<POSED>(xyz, i, P, map_inv_h(header), q, key);
        map_colour(rgb, i, c);
#pragma unroll
        for (int a = 0; a < 3; ++a) { w[a] = (unsigned)q[a]; w[3 + a] = (unsigned)c[a]; }
        if (labels) label = labels[i];
    }
    const int prev_v = __shfl_up(v, 1, 64), prev_label = __shfl_up(label, 1, 64);
    const bool lead = lane == 0 || prev_v != v;
    const u64 leaders = __ballot(lead);
    const int first = 63 - __clzll(leaders & (~0ull >> (63 - lane)));      // the run's first lane
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int there = __shfl_down(first, d, 64);               // every lane shuffles: a lane that sat out would hand its readers nothing
        const bool same = lane + d < 64 && there == first;         // runs are contiguous: lane + d in the run means all between are
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const unsigned t = __shfl_down(w[k], d, 64);
            if (same) w[k] += t;
        }
    }
    if (lead && v >= 0) {
        u64* __restrict__ row = rows + (int64_t)v * MAP_ROW;
        atomicAdd(&row[0], (u64)map_run_length(leaders, lane));
#pragma unroll
        for (int k = 0; k < 6; ++k) atomicAdd(&row[1 + k], (u64)w[k]);
        ((int*)&row[7])[1] = header[MAP_H_ADDS];
    }
    const bool pair_lead = lead || prev_label != label;
    const u64 pair_leaders = __ballot(pair_lead);
    if (!pair_lead || v < 0 || label < 0) return;
    const unsigned n = (unsigned)map_run_length(pair_leaders, lane);
    const int at = voxel_claim(pair_keys, cp, ((u64)(unsigned)v << 32) | (u64)(unsigned)label);
    if (at < 0) { atomicOr(&header[MAP_H_FLAGS], MAP_FLAG_PAIRS); return; }
    const unsigned before = atomicAdd(&pair_count[at], n);
    if (before == 0u && atomicAdd(&header[MAP_H_PAIRS], 1) + 1 > header[MAP_H_MAX_PAIRS]) atomicOr(&header[MAP_H_FLAGS], MAP_FLAG_PAIRS);
    atomicMax(&best[v], ((u64)(before + n) << 32) | (u64)(unsigned)~label);
}

// ------------------------------------------------------------------------------------------------ read-outs
template <bool POSED>
__global__ __launch_bounds__(MAP_THREADS) void map_locate_kernel(const float* __restrict__ xyz, int M, RigidPose P, const int* __restrict__ header,
                                                                 const u64* __restrict__ keys, const int* __restrict__ id, int cv, int* __restrict__ ids) {
    const int i = blockIdx.x * MAP_THREADS + threadIdx.x;
    if (i >= M) return;
    u64 q[3], key;
    int v = -1;
    if (map_point<POSED>(xyz, i, P, map_inv_h(header), q, key)) {
        const int at = voxel_find(keys, cv, key);
        if (at >= 0) v = id[at];
    }
    ids[i] = v;
}

__global__ __launch_bounds__(MAP_THREADS) void map_labels_kernel(const int* __restrict__ header, const u64* __restrict__ best, int V, int min_votes,
                                                                 int* __restrict__ label, int* __restrict__ votes) {
    const int v = blockIdx.x * MAP_THREADS + threadIdx.x;
    if (v >= V) return;
    const u64 b = v < header[MAP_H_V] ? best[v] : 0ull;
    const int n = (int)(b >> 32);
    const bool ok = n >= min_votes;                                // min_votes >= 1: a voxel without a pair has b = 0
    label[v] = ok ? (int)~(unsigned)b : -1;
    votes[v] = ok ? n : 0;
}

__global__ __launch_bounds__(MAP_THREADS) void map_cloud_kernel(const int* __restrict__ header, const u64* __restrict__ rows, int V, float* __restrict__ xyz,
                                                                float* __restrict__ rgb) {
    const int v = blockIdx.x * MAP_THREADS + threadIdx.x;
    if (v >= V) return;
    const u64* __restrict__ row = rows + (int64_t)v * MAP_ROW;
    const bool have = v < header[MAP_H_V];
    const u64 n = have ? row[0] : 0ull;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        xyz[(int64_t)v * 3 + a] = n ? map_mean(row[1 + a], n) : 0.0f;
        rgb[(int64_t)v * 3 + a] = n ? map_mean(row[4 + a], n) : 0.0f;
    }
}

__global__ __launch_bounds__(MAP_THREADS) void map_fields_kernel(const int* __restrict__ header, const u64* __restrict__ rows, const u64* __restrict__ key_of_id,
                                                                 int V, int* __restrict__ count, int* __restrict__ first_seen, int* __restrict__ last_seen,
                                                                 int64_t* __restrict__ keys, int64_t* __restrict__ sums) {
    const int v = blockIdx.x * MAP_THREADS + threadIdx.x;
    if (v >= V) return;
    const bool have = v < header[MAP_H_V];
    const u64* __restrict__ row = rows + (int64_t)v * MAP_ROW;
    if (count) count[v] = have ? (int)row[0] : 0;
    if (first_seen) first_seen[v] = have ? ((const int*)&row[7])[0] : 0;
    if (last_seen) last_seen[v] = have ? ((const int*)&row[7])[1] : 0;
    if (keys) keys[v] = have ? (int64_t)key_of_id[v] : -1;
    if (sums) {
#pragma unroll
        for (int a = 0; a < 6; ++a) sums[(int64_t)v * 6 + a] = have ? (int64_t)row[1 + a] : 0;
    }
}

// ------------------------------------------------------------------------------------------------ entries
static inline unsigned map_blocks(int64_t n) { return (unsigned)psam_cdiv(n, MAP_THREADS); }

PSAM_API size_t psam_map_bytes(int32_t max_voxels, int32_t max_pairs) {
    if (!map_caps_ok(max_voxels, max_pairs)) return 0;
    return map_layout(nullptr, max_voxels, max_pairs).bytes;
}

PSAM_API size_t psam_map_add_workspace_bytes(int32_t M) {
    if (M <= 0 || M > MAP_MAX_POINTS) return 0;
    return map_add_layout(nullptr, M).bytes;
}

#define MAP_REQUIRE_BLOCK(name)                                                                                                                         \
    PSAM_REQUIRE(map_caps_ok(max_voxels, max_pairs), PSAM_EINVAL, name ": need 0 < max_voxels <= 2^28 and 0 < max_pairs <= 2^28");                     \
    PSAM_REQUIRE(map_bytes >= psam_map_bytes(max_voxels, max_pairs), PSAM_EWORKSPACE, name ": map block too small (psam_map_bytes)");                  \
    PSAM_REQUIRE(((uintptr_t)map & 15) == 0, PSAM_EALIGN, name ": map block must be 16-byte aligned")

PSAM_API int32_t psam_map_clear(void* map, size_t map_bytes, int32_t max_voxels, int32_t max_pairs, float inv_h, hipStream_t stream) {
    PSAM_REQUIRE(map, PSAM_EINVAL, "psam_map_clear: null pointer");
    MAP_REQUIRE_BLOCK("psam_map_clear");
    PSAM_REQUIRE(std::isfinite(inv_h) && inv_h > 0.0f, PSAM_EINVAL, "psam_map_clear: inv_h must be finite and positive");
    const MapBlock b = map_layout(map, max_voxels, max_pairs);
    VoxelWs ones = {};
    ones.keys = b.keys;
    ones.table_bytes = b.ones_bytes;
    int32_t st = voxel_clear<0>(ones, nullptr, stream, "psam_map_clear: table clear launch failed");
    if (st != PSAM_OK) return st;
    const int64_t granules = (int64_t)((b.bytes - b.zero_at) / 16);
    hipLaunchKernelGGL(map_init_kernel, dim3((unsigned)(granules < 4096 * MAP_THREADS ? psam_cdiv(granules, MAP_THREADS) : 4096)), dim3(MAP_THREADS), 0, stream,
                       b.header, (int)max_voxels, (int)max_pairs, inv_h, (uint4*)((char*)map + b.zero_at), granules);
    return psam_launch_status("psam_map_clear: init launch failed");
}

PSAM_API int32_t psam_map_add(void* map, size_t map_bytes, int32_t max_voxels, int32_t max_pairs, const float* xyz, const float* rgb, const int32_t* labels,
                              int32_t M, const float* pose, int32_t* ids, void* ws, size_t ws_bytes, hipStream_t stream) {
    PSAM_REQUIRE(map && xyz && rgb && ids && ws, PSAM_EINVAL, "psam_map_add: null pointer");
    PSAM_REQUIRE(M > 0 && M <= MAP_MAX_POINTS, PSAM_EINVAL, "psam_map_add: need 0 < M <= 2^28");
    MAP_REQUIRE_BLOCK("psam_map_add");
    RigidPose P = {};
    PSAM_REQUIRE(!pose || pose_load(pose, P), PSAM_EINVAL, "psam_map_add: pose must be finite");
    PSAM_REQUIRE(ws_bytes >= psam_map_add_workspace_bytes(M), PSAM_EWORKSPACE, "psam_map_add: workspace too small (psam_map_add_workspace_bytes)");
    PSAM_REQUIRE(((uintptr_t)ws & 15) == 0, PSAM_EALIGN, "psam_map_add: workspace must be 16-byte aligned");
    const MapBlock b = map_layout(map, max_voxels, max_pairs);
    const MapAddWs w = map_add_layout(ws, M);
    const int capacity = (int)voxel_capacity(M);
    const unsigned point_blocks = map_blocks(M), blocks = (unsigned)scan_blocks(M);
    int32_t st = voxel_clear<4>(w.table, w.counter, stream, "psam_map_add: clear launch failed");
    if (st != PSAM_OK) return st;
    if (pose)
        hipLaunchKernelGGL(map_insert_kernel<true>, dim3(point_blocks), dim3(MAP_THREADS), 0, stream, xyz, rgb, (int)M, P, (const int*)b.header, w.table.keys,
                           w.table.low, capacity, w.table.rep, w.counter);
    else
        hipLaunchKernelGGL(map_insert_kernel<false>, dim3(point_blocks), dim3(MAP_THREADS), 0, stream, xyz, rgb, (int)M, P, (const int*)b.header, w.table.keys,
                           w.table.low, capacity, w.table.rep, w.counter);
    if ((st = psam_launch_status("psam_map_add: insert launch failed")) != PSAM_OK) return st;
    hipLaunchKernelGGL(map_lookup_kernel, dim3(blocks), dim3(SCAN_THREADS), 0, stream, (const int*)w.table.rep, (const unsigned*)w.table.low,
                       (const u64*)w.table.keys, (int)M, (const u64*)b.keys, (const int*)b.id, b.cv, w.wid, w.table.block);
    if ((st = psam_launch_status("psam_map_add: look-up launch failed")) != PSAM_OK) return st;
    hipLaunchKernelGGL(map_offsets_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, w.table.block, (int)blocks, (int)M, w.counter, b.header);
    if ((st = psam_launch_status("psam_map_add: offsets launch failed")) != PSAM_OK) return st;
    hipLaunchKernelGGL(map_rank_kernel, dim3(blocks), dim3(SCAN_THREADS), 0, stream, (const int*)w.table.rep, (const unsigned*)w.table.low,
                       (const u64*)w.table.keys, (int)M, (const int*)w.table.block, (const int*)w.counter, b.header, b.keys, b.id, b.cv, b.rows, b.key_of_id, w.wid);
    if ((st = psam_launch_status("psam_map_add: rank launch failed")) != PSAM_OK) return st;
    auto accumulate = pose ? map_accumulate_kernel<true> : map_accumulate_kernel<false>;
    hipLaunchKernelGGL(accumulate, dim3(point_blocks), dim3(MAP_THREADS), 0, stream, xyz, rgb, labels, (int)M, P, (const int*)w.table.rep, (const int*)w.wid,
                       b.header, b.rows, b.pair_keys, b.pair_count, b.cp, b.best, ids);
    return psam_launch_status("psam_map_add: accumulate launch failed");
}

PSAM_API int32_t psam_map_locate(const void* map, size_t map_bytes, int32_t max_voxels, int32_t max_pairs, const float* xyz, int32_t M, const float* pose,
                                 int32_t* ids, hipStream_t stream) {
    PSAM_REQUIRE(map && xyz && ids, PSAM_EINVAL, "psam_map_locate: null pointer");
    PSAM_REQUIRE(M > 0 && M <= MAP_MAX_POINTS, PSAM_EINVAL, "psam_map_locate: need 0 < M <= 2^28");
    MAP_REQUIRE_BLOCK("psam_map_locate");
    RigidPose P = {};
    PSAM_REQUIRE(!pose || pose_load(pose, P), PSAM_EINVAL, "psam_map_locate: pose must be finite");
    const MapBlock b = map_layout((void*)map, max_voxels, max_pairs);
    if (pose)
        hipLaunchKernelGGL(map_locate_kernel<true>, dim3(map_blocks(M)), dim3(MAP_THREADS), 0, stream, xyz, (int)M, P, (const int*)b.header, (const u64*)b.keys,
                           (const int*)b.id, b.cv, ids);
    else
        hipLaunchKernelGGL(map_locate_kernel<false>, dim3(map_blocks(M)), dim3(MAP_THREADS), 0, stream, xyz, (int)M, P, (const int*)b.header, (const u64*)b.keys,
                           (const int*)b.id, b.cv, ids);
    return psam_launch_status("psam_map_locate: launch failed");
}

PSAM_API int32_t psam_map_labels(const void* map, size_t map_bytes, int32_t max_voxels, int32_t max_pairs, int32_t V, int32_t min_votes, int32_t* label,
                                 int32_t* votes, hipStream_t stream) {
    PSAM_REQUIRE(map && label && votes, PSAM_EINVAL, "psam_map_labels: null pointer");
    MAP_REQUIRE_BLOCK("psam_map_labels");
    PSAM_REQUIRE(V > 0 && V <= max_voxels, PSAM_EINVAL, "psam_map_labels: need 0 < V <= max_voxels");
    PSAM_REQUIRE(min_votes >= 1, PSAM_EINVAL, "psam_map_labels: min_votes must be at least 1");
    const MapBlock b = map_layout((void*)map, max_voxels, max_pairs);
    hipLaunchKernelGGL(map_labels_kernel, dim3(map_blocks(V)), dim3(MAP_THREADS), 0, stream, (const int*)b.header, (const u64*)b.best, (int)V, (int)min_votes,
                       label, votes);
    return psam_launch_status("psam_map_labels: launch failed");
}

PSAM_API int32_t psam_map_cloud(const void* map, size_t map_bytes, int32_t max_voxels, int32_t max_pairs, int32_t V, float* xyz, float* rgb,
                                hipStream_t stream) {
    PSAM_REQUIRE(map && xyz && rgb, PSAM_EINVAL, "psam_map_cloud: null pointer");
    MAP_REQUIRE_BLOCK("psam_map_cloud");
    PSAM_REQUIRE(V > 0 && V <= max_voxels, PSAM_EINVAL, "psam_map_cloud: need 0 < V <= max_voxels");
    const MapBlock b = map_layout((void*)map, max_voxels, max_pairs);
    hipLaunchKernelGGL(map_cloud_kernel, dim3(map_blocks(V)), dim3(MAP_THREADS), 0, stream, (const int*)b.header, (const u64*)b.rows, (int)V, xyz, rgb);
    return psam_launch_status("psam_map_cloud: launch failed");
}

PSAM_API int32_t psam_map_fields(const void* map, size_t map_bytes, int32_t max_voxels, int32_t max_pairs, int32_t V, int32_t* count, int32_t* first_seen,
                                 int32_t* last_seen, int64_t* keys, int64_t* sums, hipStream_t stream) {
    PSAM_REQUIRE(map && (count || first_seen || last_seen || keys || sums), PSAM_EINVAL, "psam_map_fields: null pointer");
    MAP_REQUIRE_BLOCK("psam_map_fields");
    PSAM_REQUIRE(V > 0 && V <= max_voxels, PSAM_EINVAL, "psam_map_fields: need 0 < V <= max_voxels");
    PSAM_REQUIRE(((uintptr_t)keys & 7) == 0 && ((uintptr_t)sums & 7) == 0, PSAM_EALIGN, "psam_map_fields: keys and sums must be 8-byte aligned");
    const MapBlock b = map_layout((void*)map, max_voxels, max_pairs);
    hipLaunchKernelGGL(map_fields_kernel, dim3(map_blocks(V)), dim3(MAP_THREADS), 0, stream, (const int*)b.header, (const u64*)b.rows, (const u64*)b.key_of_id,
                       (int)V, count, first_seen, last_seen, keys, sums);
    return psam_launch_status("psam_map_fields: launch failed");
}
