// Connected components of packed masks (point_sam_amd/regions.py): which points of a mask hang together, and the clean-up built on that -- small
// holes filled, small islands removed, only the clicked part kept.  Everything is an integer or a bit, so every output is exact and reproducible.
//
// The graph.  Points are adjacent iff their voxel cells (voxel_cell.h: scene.hip's cells) differ by at most 1 on every axis.  All points of a voxel
// are mutually adjacent, so components are found on the VOXEL graph: V occupied voxels (psam_voxel_downsample's keep_idx / inv), 26 neighbour ranks
// each (psam_region_neighbors), and a row's point set reduced to per-voxel member counts.
//   psam_region_neighbors   a key -> rank table of its own (voxel_table.h's table: claimed, then found), then one look-up per (voxel, offset)
//   psam_region_labels      per point the id of its component (the lowest voxel rank in it), -1 outside the set
//   psam_region_clean       holes, islands, seeds: two component runs (the complement, then the filled mask) and word-wise rewrites of the rows
//
// Components of K rows at once, grid = (voxel blocks, rows), every launch a kernel boundary (no value is handed over inside a kernel):
//   init     count = 0, parent[v] = v, size = 0
//   count    count[inv[n]] += 1 for every member point n (integer atomic adds)
//   hook     union-find over the edges (v, nbr[v, o]), o < 13 (the other 13 are the same edges seen from the far end): both ends are walked to their
//            roots and the higher root is hooked under the lower by compare-and-swap.  A parent is always below its child, so a walk descends
//            strictly, cannot cycle, and ends at the lowest rank of the tree; parents are read and written with agent-scope atomics only.
//   flatten  parent[v] = root(v); size[root] += count[v]
// The root of a finished tree is the lowest rank of its component, whatever order the waves arrived in: it IS the component's id.  Every loop has a
// bound derived from V (a walk descends at least one rank per step; a failed hook lowers one of its two ends): a logic error ends as a wrong answer.
#include "common.h"
#include "region_union.h"    // region_find, region_union, region_shorten, region_flatten
#include "row_popcount.h"    // block_sum, row_popcount
#include "voxel_table.h"

#include <cmath>

constexpr int REGION_THREADS = 256;
constexpr int REGION_WAVES = REGION_THREADS / WAVE;
constexpr int REGION_MAX_ROWS = 65535;            // rows are the grid's y dimension
constexpr int REGION_MAX_POINTS = 1 << 28;

static inline unsigned region_blocks(int64_t n) { return (unsigned)psam_cdiv(n, REGION_THREADS); }

// ------------------------------------------------------------------------------------------------ neighbours
__device__ __forceinline__ bool region_cell(const float* __restrict__ xyz, int64_t i, float ox, float oy, float oz, float inv_h, u64& cx, u64& cy, u64& cz) {
    return voxel_axis(xyz[i * 3 + 0], ox, inv_h, cx) & voxel_axis(xyz[i * 3 + 1], oy, inv_h, cy) & voxel_axis(xyz[i * 3 + 2], oz, inv_h, cz);
}

// One thread per voxel: its key claims a slot, the slot's rank is an unsigned minimum (keys of distinct voxels differ, so the minimum is over one
// value; a repeated representative would still give one answer).
__global__ __launch_bounds__(REGION_THREADS) void region_table_insert_kernel(const float* __restrict__ xyz, const int64_t* __restrict__ keep_idx, int V,
                                                                           float ox, float oy, float oz, float inv_h, u64* __restrict__ keys,
                                                                           unsigned* __restrict__ rank, int capacity) {
    const int v = blockIdx.x * REGION_THREADS + threadIdx.x;
    if (v >= V) return;
    const int64_t i = keep_idx[v];
    u64 cx, cy, cz;
    if (i < 0 || !region_cell(xyz, i, ox, oy, oz, inv_h, cx, cy, cz)) return;      // no cell: never found, every neighbour of it is -1
    const int slot = voxel_claim(keys, capacity, voxel_key(cx, cy, cz));
    if (slot >= 0) atomicMin(&rank[slot], (unsigned)v);
}

// One thread per (voxel, offset).  Offset o of 26: o' = o below 13, o + 1 from 13 on (the centre is skipped); dz = o' / 9 - 1, dy = o' / 3 % 3 - 1,
// dx = o' % 3 - 1, so offset 25 - o is the opposite of offset o.
__global__ __launch_bounds__(REGION_THREADS) void region_table_lookup_kernel(const float* __restrict__ xyz, const int64_t* __restrict__ keep_idx, int V,
                                                                           float ox, float oy, float oz, float inv_h, const u64* __restrict__ keys,
                                                                           const unsigned* __restrict__ rank, int capacity, int* __restrict__ nbr) {
    const int64_t t = (int64_t)blockIdx.x * REGION_THREADS + threadIdx.x;
    if (t >= (int64_t)V * 26) return;
    const int v = (int)(t / 26), o = (int)(t % 26), oc = o < 13 ? o : o + 1;
    int found = -1;
    const int64_t i = keep_idx[v];
    u64 cx, cy, cz;
    if (i >= 0 && region_cell(xyz, i, ox, oy, oz, inv_h, cx, cy, cz)) {
        const int64_t nx = (int64_t)cx + (oc % 3 - 1), ny = (int64_t)cy + (oc / 3 % 3 - 1), nz = (int64_t)cz + (oc / 9 - 1);
        const int64_t lim = (int64_t)1 << VOXEL_AXIS_BITS;
        if (nx >= 0 && nx < lim && ny >= 0 && ny < lim && nz >= 0 && nz < lim) {
            const int slot = voxel_find(keys, capacity, voxel_key((u64)nx, (u64)ny, (u64)nz));      // the table is finished: a kernel boundary
            if (slot >= 0) found = (int)rank[slot];
        }
    }
    nbr[t] = found;
}

PSAM_API size_t psam_region_neighbors_workspace_bytes(int32_t V) {
    if (V <= 0 || V > REGION_MAX_POINTS) return 0;
    return voxel_layout(nullptr, V, false, false).bytes;
}

PSAM_API int32_t psam_region_neighbors(const float* xyz, const int64_t* keep_idx, int32_t V, const float* origin, float inv_h, int32_t* nbr, void* ws,
                                       size_t ws_bytes, hipStream_t stream) {
    PSAM_REQUIRE(xyz && keep_idx && origin && nbr && ws, PSAM_EINVAL, "psam_region_neighbors: null pointer");
    PSAM_REQUIRE(V > 0 && V <= REGION_MAX_POINTS, PSAM_EINVAL, "psam_region_neighbors: need 0 < V <= 2^28");
    PSAM_REQUIRE(std::isfinite(inv_h) && inv_h > 0.0f, PSAM_EINVAL, "psam_region_neighbors: inv_h must be finite and positive");
    PSAM_REQUIRE(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]), PSAM_EINVAL, "psam_region_neighbors: origin must be finite");
    PSAM_REQUIRE(ws_bytes >= psam_region_neighbors_workspace_bytes(V), PSAM_EWORKSPACE,
                 "psam_region_neighbors: workspace too small (psam_region_neighbors_workspace_bytes)");
    PSAM_REQUIRE(((uintptr_t)ws & 15) == 0, PSAM_EALIGN, "psam_region_neighbors: workspace must be 16-byte aligned");
    const VoxelWs w = voxel_layout(ws, V, false, false);
    const int capacity = (int)voxel_capacity(V);
    int32_t st = voxel_clear<0>(w, nullptr, stream, "psam_region_neighbors: clear launch failed");
    if (st != PSAM_OK) return st;
    hipLaunchKernelGGL(region_table_insert_kernel, dim3(region_blocks(V)), dim3(REGION_THREADS), 0, stream, xyz, keep_idx, (int)V, origin[0], origin[1],
                       origin[2], inv_h, w.keys, w.low, capacity);
    if ((st = psam_launch_status("psam_region_neighbors: insert launch failed")) != PSAM_OK) return st;
    hipLaunchKernelGGL(region_table_lookup_kernel, dim3(region_blocks((int64_t)V * 26)), dim3(REGION_THREADS), 0, stream, xyz, keep_idx, (int)V, origin[0],
                       origin[1], origin[2], inv_h, (const u64*)w.keys, (const unsigned*)w.low, capacity, nbr);
    return psam_launch_status("psam_region_neighbors: look-up launch failed");
}

// ------------------------------------------------------------------------------------------------ components
// Per row k: cnt, parent, size (and, with seeds, flag) are [V] slices at k * V of [K, V] arrays.  `active` (may be NULL: every row) skips rows.
// (the walks and the hook: region_union.h)
__global__ __launch_bounds__(REGION_THREADS) void region_init_kernel(int* __restrict__ cnt, int* __restrict__ parent, int* __restrict__ size,
                                                                   int* __restrict__ flag, int V, u64* __restrict__ best, int* __restrict__ any_seed) {
    const int v = blockIdx.x * REGION_THREADS + threadIdx.x, k = blockIdx.y;
    if (v == 0) {
        if (best) best[k] = 0ull;
        if (any_seed) any_seed[k] = 0;
    }
    if (v >= V) return;
    const int64_t e = (int64_t)k * V + v;
    cnt[e] = 0;
    parent[e] = v;
    if (size) size[e] = 0;
    if (flag) flag[e] = 0;
}

__global__ __launch_bounds__(REGION_THREADS) void region_count_kernel(const u64* __restrict__ bits, int W, const int64_t* __restrict__ inv, int N, int V,
                                                                    int complement, const int* __restrict__ active, int* __restrict__ cnt) {
    const int n = blockIdx.x * REGION_THREADS + threadIdx.x, k = blockIdx.y;
    if (n >= N || (active && !active[k])) return;
    const bool in = (((bits[(int64_t)k * W + (n >> 6)] >> (n & 63)) & 1ull) != 0) != (complement != 0);
    if (!in) return;
    const int64_t v = inv[n];
    if ((u64)v < (u64)V) atomicAdd(&cnt[(int64_t)k * V + v], 1);
}

__global__ __launch_bounds__(REGION_THREADS) void region_hook_kernel(const int* __restrict__ cnt, int* parent, const int* __restrict__ nbr,
                                                                   int V) {
    const int v = blockIdx.x * REGION_THREADS + threadIdx.x, k = blockIdx.y;
    if (v >= V) return;
    const int* __restrict__ c = cnt + (int64_t)k * V;
    int* par = parent + (int64_t)k * V;      // written by every thread of the row: atomics only, no __restrict__
    if (c[v] == 0) return;
    for (int o = 0; o < 13; ++o) {
        const int u = nbr[(int64_t)v * 26 + o];
        if ((unsigned)u >= (unsigned)V || c[u] == 0) continue;
        region_union(par, v, u, V);
    }
    region_shorten(par, v, V);
}

__global__ __launch_bounds__(REGION_THREADS) void region_flatten_kernel(const int* __restrict__ cnt, int* parent, int* __restrict__ size, int V) {
    const int v = blockIdx.x * REGION_THREADS + threadIdx.x, k = blockIdx.y;
    if (v >= V) return;
    const int64_t row = (int64_t)k * V;
    const int c = cnt[row + v];
    if (c == 0) return;
    const int r = region_flatten(parent + row, v, V);
    if (size) atomicAdd(&size[row + r], c);
}

struct CompWs {
    int* cnt;             // [K, V]
    int* parent;          // [K, V]
    int* size;            // [K, V]   clean only
    int* flag;            // [K, V]   clean with seeds only
    int* active;          // [K]      clean only
    int* any_seed;        // [K]
    u64* best;            // [K]
    size_t bytes;
};

static inline CompWs comp_layout(void* ws, int64_t K, int64_t V, bool clean, bool seeds) {
    CompWs w = {};
    char* p = (char*)ws;
    size_t o = 0;
    const size_t kv = align16((size_t)K * (size_t)V * sizeof(int));
    w.cnt = (int*)(p + o);      o += kv;
    w.parent = (int*)(p + o);   o += kv;
    if (clean) {
        w.size = (int*)(p + o);     o += kv;
        if (seeds) { w.flag = (int*)(p + o); o += kv; }
        w.active = (int*)(p + o);   o += align16((size_t)K * sizeof(int));
        w.any_seed = (int*)(p + o); o += align16((size_t)K * sizeof(int));
        w.best = (u64*)(p + o);     o += align16((size_t)K * sizeof(u64));
    }
    w.bytes = o;
    return w;
}

// init, count, hook, flatten for K rows
static int32_t region_components(const u64* bits, const int64_t* inv, const int* nbr, int K, int N, int V, int complement, const CompWs& w, bool row_words,
                                 hipStream_t stream, const char* what) {
    const dim3 vgrid(region_blocks(V), (unsigned)K), threads(REGION_THREADS);
    const int W = (int)psam_cdiv(N, 64);
    hipLaunchKernelGGL(region_init_kernel, vgrid, threads, 0, stream, w.cnt, w.parent, w.size, w.flag, V, row_words ? w.best : nullptr,
                       row_words ? w.any_seed : nullptr);
    int32_t st = psam_launch_status(what);
    if (st != PSAM_OK) return st;
    hipLaunchKernelGGL(region_count_kernel, dim3(region_blocks(N), (unsigned)K), threads, 0, stream, bits, W, inv, N, V, complement, (const int*)w.active, w.cnt);
    if ((st = psam_launch_status(what)) != PSAM_OK) return st;
    hipLaunchKernelGGL(region_hook_kernel, vgrid, threads, 0, stream, (const int*)w.cnt, w.parent, nbr, V);
    if ((st = psam_launch_status(what)) != PSAM_OK) return st;
    hipLaunchKernelGGL(region_flatten_kernel, vgrid, threads, 0, stream, (const int*)w.cnt, w.parent, w.size, V);
    return psam_launch_status(what);
}

// ------------------------------------------------------------------------------------------------ labels
__global__ __launch_bounds__(REGION_THREADS) void region_labels_kernel(const u64* __restrict__ bits, int W, const int64_t* __restrict__ inv,
                                                                     const int* __restrict__ parent, int N, int V, int complement, int* __restrict__ labels) {
    const int n = blockIdx.x * REGION_THREADS + threadIdx.x, k = blockIdx.y;
    if (n >= N) return;
    const bool in = (((bits[(int64_t)k * W + (n >> 6)] >> (n & 63)) & 1ull) != 0) != (complement != 0);
    const int64_t v = inv[n];
    labels[(int64_t)k * N + n] = (in && (u64)v < (u64)V) ? parent[(int64_t)k * V + v] : -1;
}

static inline bool region_shape_ok(int32_t K, int32_t N, int32_t V) {
    return K > 0 && K <= REGION_MAX_ROWS && N > 0 && N <= REGION_MAX_POINTS && V > 0 && V <= REGION_MAX_POINTS;
}

PSAM_API size_t psam_region_labels_workspace_bytes(int32_t K, int32_t N, int32_t V) {
    if (!region_shape_ok(K, N, V)) return 0;
    return comp_layout(nullptr, K, V, false, false).bytes;
}

PSAM_API int32_t psam_region_labels(const uint64_t* bits, const int64_t* inv, const int32_t* nbr, int32_t K, int32_t N, int32_t V, int32_t complement,
                                    int32_t* labels, void* ws, size_t ws_bytes, hipStream_t stream) {
    PSAM_REQUIRE(bits && inv && nbr && labels && ws, PSAM_EINVAL, "psam_region_labels: null pointer");
    PSAM_REQUIRE(region_shape_ok(K, N, V), PSAM_EINVAL, "psam_region_labels: need 0 < K <= 65535, 0 < N <= 2^28, 0 < V <= 2^28");
    PSAM_REQUIRE(ws_bytes >= psam_region_labels_workspace_bytes(K, N, V), PSAM_EWORKSPACE,
                 "psam_region_labels: workspace too small (psam_region_labels_workspace_bytes)");
    PSAM_REQUIRE(((uintptr_t)ws & 15) == 0, PSAM_EALIGN, "psam_region_labels: workspace must be 16-byte aligned");
    const CompWs w = comp_layout(ws, K, V, false, false);
    int32_t st = region_components((const u64*)bits, inv, nbr, K, N, V, complement, w, false, stream, "psam_region_labels: component launch failed");
    if (st != PSAM_OK) return st;
    hipLaunchKernelGGL(region_labels_kernel, dim3(region_blocks(N), (unsigned)K), dim3(REGION_THREADS), 0, stream, (const u64*)bits, (int)psam_cdiv(N, 64), inv,
                       (const int*)w.parent, (int)N, (int)V, (int)complement, labels);
    return psam_launch_status("psam_region_labels: labels launch failed");
}

// ------------------------------------------------------------------------------------------------ clean
// active[k] = the row is selected and not empty (an empty mask stays empty; an unselected row is copied)
__global__ __launch_bounds__(REGION_THREADS) void region_rows_kernel(const u64* __restrict__ bits, int W, const unsigned char* __restrict__ select,
                                                                   int* __restrict__ active) {
    __shared__ int s_cnt[REGION_WAVES];
    const int k = blockIdx.x;
    const int s = row_popcount<REGION_THREADS>(bits + (int64_t)k * W, W, s_cnt);
    if (threadIdx.x == 0) active[k] = (s > 0 && (!select || select[k] != 0)) ? 1 : 0;
}

// Step 1, one wave per word: the mask plus every complement component below min_hole points (parent / size: the complement's components; unused
// with min_hole == 0).  The ballot is the output word, so bits past N are zero.  An inactive row is copied word for word.
__global__ __launch_bounds__(REGION_THREADS) void region_fill_kernel(const u64* __restrict__ bits, int W, const int64_t* __restrict__ inv,
                                                                   const int* __restrict__ parent, const int* __restrict__ size,
                                                                   const int* __restrict__ active, int N, int V, int min_hole, u64* __restrict__ out) {
    const int lane = threadIdx.x & 63, k = blockIdx.y;
    const int w = blockIdx.x * REGION_WAVES + (threadIdx.x >> 6);
    if (w >= W) return;                                            // wave-uniform
    const u64 word = bits[(int64_t)k * W + w];
    if (!active[k]) {
        if (lane == 0) out[(int64_t)k * W + w] = word;
        return;
    }
    const int64_t n = (int64_t)w * 64 + lane;
    bool on = n < N && ((word >> lane) & 1ull);
    if (min_hole > 0 && n < N && !on) {
        const int64_t v = inv[n];
        if ((u64)v < (u64)V) {
            const int64_t row = (int64_t)k * V;
            on = size[row + parent[row + v]] < min_hole;
        }
    }
    const u64 m = __ballot(on);
    if (lane == 0) out[(int64_t)k * W + w] = m;
}

// The row's largest component: the maximum of (size << 32 | 0x7fffffff - id) over its roots, so a size tie goes to the lowest id.
__global__ __launch_bounds__(REGION_THREADS) void region_best_kernel(const int* __restrict__ cnt, const int* __restrict__ parent, const int* __restrict__ size,
                                                                   int V, u64* __restrict__ best) {
    const int v = blockIdx.x * REGION_THREADS + threadIdx.x, k = blockIdx.y;
    const int64_t row = (int64_t)k * V;
    u64 key = 0;
    if (v < V && cnt[row + v] > 0 && parent[row + v] == v) key = ((u64)(unsigned)size[row + v] << 32) | (u64)(unsigned)(0x7fffffff - v);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const u64 o = __shfl_xor(key, d, 64); key = o > key ? o : key; }
    if ((threadIdx.x & 63) == 0 && key != 0) atomicMax(&best[k], key);
}

__device__ __forceinline__ bool region_survives(int size, int root, int min_island, u64 best) {
    return min_island <= 0 || size >= min_island || root == 0x7fffffff - (int)(unsigned)(best & 0xffffffffull);
}

// One thread per (row, seed): a seed that is a member of the row after step 2 flags its component.  Every writer stores the same value.
__global__ __launch_bounds__(REGION_THREADS) void region_seed_kernel(const u64* __restrict__ filled, int W, const int64_t* __restrict__ inv,
                                                                   const int* __restrict__ parent, const int* __restrict__ size,
                                                                   const u64* __restrict__ best, const int* __restrict__ active,
                                                                   const int* __restrict__ seeds, int K, int N, int V, int S, int min_island,
                                                                   int* __restrict__ flag, int* __restrict__ any_seed) {
    const int64_t t = (int64_t)blockIdx.x * REGION_THREADS + threadIdx.x;
    if (t >= (int64_t)K * S) return;
    const int k = (int)(t / S), n = seeds[t];
    if (!active[k] || n < 0 || n >= N) return;
    if (((filled[(int64_t)k * W + (n >> 6)] >> (n & 63)) & 1ull) == 0) return;
    const int64_t v = inv[n];
    if ((u64)v >= (u64)V) return;
    const int64_t row = (int64_t)k * V;
    const int r = parent[row + v];
    if (!region_survives(size[row + r], r, min_island, best[k])) return;
    flag[row + r] = 1;
    any_seed[k] = 1;
}

// Steps 2 and 3, one wave per word, in place on the filled row (a wave reads and writes only its own word): a point stays if its component
// survives the island rule and, when a seed landed in the row, its component is flagged.
__global__ __launch_bounds__(REGION_THREADS) void region_final_kernel(u64* __restrict__ out, int W, const int64_t* __restrict__ inv,
                                                                    const int* __restrict__ parent, const int* __restrict__ size,
                                                                    const u64* __restrict__ best, const int* __restrict__ active,
                                                                    const int* __restrict__ flag, const int* __restrict__ any_seed, int N, int V,
                                                                    int min_island) {
    const int lane = threadIdx.x & 63, k = blockIdx.y;
    const int w = blockIdx.x * REGION_WAVES + (threadIdx.x >> 6);
    if (w >= W || !active[k]) return;                              // wave-uniform
    const u64 word = out[(int64_t)k * W + w];
    const int64_t n = (int64_t)w * 64 + lane;
    bool on = n < N && ((word >> lane) & 1ull);
    if (on) {
        const int64_t v = inv[n];
        if ((u64)v < (u64)V) {
            const int64_t row = (int64_t)k * V;
            const int r = parent[row + v];
            on = region_survives(size[row + r], r, min_island, best[k]) && (!flag || !any_seed[k] || flag[row + r] != 0);
        }
    }
    const u64 m = __ballot(on);
    if (lane == 0) out[(int64_t)k * W + w] = m;
}

__global__ __launch_bounds__(REGION_THREADS) void region_area_kernel(const u64* __restrict__ bits, const u64* __restrict__ out, int W, int* __restrict__ area,
                                                                   unsigned char* __restrict__ changed) {
    __shared__ int s_cnt[REGION_WAVES], s_diff[REGION_WAVES];
    const int k = blockIdx.x;
    int c = 0, diff = 0;
    for (int w = threadIdx.x; w < W; w += REGION_THREADS) {
        const u64 o = out[(int64_t)k * W + w];
        c += __popcll(o);
        diff |= o != bits[(int64_t)k * W + w] ? 1 : 0;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) diff |= __shfl_xor(diff, d, 64);
    if ((threadIdx.x & 63) == 0) s_diff[threadIdx.x >> 6] = diff;
    const int s = block_sum<REGION_THREADS>(c, s_cnt);             // its barrier is s_diff's too
    if (threadIdx.x == 0) {
        int f = 0;
        for (int w = 0; w < REGION_WAVES; ++w) f |= s_diff[w];
        area[k] = s;
        changed[k] = f ? 1 : 0;
    }
}

PSAM_API size_t psam_region_clean_workspace_bytes(int32_t K, int32_t N, int32_t V, int32_t S) {
    if (!region_shape_ok(K, N, V) || S < 0) return 0;
    return comp_layout(nullptr, K, V, true, S > 0).bytes;
}

PSAM_API int32_t psam_region_clean(const uint64_t* bits, const uint8_t* select, const int64_t* inv, const int32_t* nbr, const int32_t* seeds, int32_t K,
                                   int32_t N, int32_t V, int32_t S, int32_t min_island, int32_t min_hole, uint64_t* bits_out, int32_t* area_out,
                                   uint8_t* changed, void* ws, size_t ws_bytes, hipStream_t stream) {
    PSAM_REQUIRE(bits && inv && nbr && bits_out && area_out && changed && ws, PSAM_EINVAL, "psam_region_clean: null pointer");
    PSAM_REQUIRE(region_shape_ok(K, N, V), PSAM_EINVAL, "psam_region_clean: need 0 < K <= 65535, 0 < N <= 2^28, 0 < V <= 2^28");
    PSAM_REQUIRE(S >= 0 && (S == 0 || seeds), PSAM_EINVAL, "psam_region_clean: need S >= 0, and seeds [K, S] (null pointer) when S > 0");
    PSAM_REQUIRE((int64_t)K * S <= 0x7fffffff, PSAM_EINVAL, "psam_region_clean: K * S above 2^31 - 1");
    PSAM_REQUIRE(min_island >= 0 && min_hole >= 0, PSAM_EINVAL, "psam_region_clean: min_island and min_hole must not be negative");
    PSAM_REQUIRE(bits_out != bits, PSAM_EINVAL, "psam_region_clean: bits_out must not alias bits");
    PSAM_REQUIRE(ws_bytes >= psam_region_clean_workspace_bytes(K, N, V, S), PSAM_EWORKSPACE,
                 "psam_region_clean: workspace too small (psam_region_clean_workspace_bytes)");
    PSAM_REQUIRE(((uintptr_t)ws & 15) == 0, PSAM_EALIGN, "psam_region_clean: workspace must be 16-byte aligned");
    const CompWs w = comp_layout(ws, K, V, true, S > 0);
    const int W = (int)psam_cdiv(N, 64);
    const dim3 threads(REGION_THREADS), wgrid((unsigned)psam_cdiv(W, REGION_WAVES), (unsigned)K);
    hipLaunchKernelGGL(region_rows_kernel, dim3((unsigned)K), threads, 0, stream, (const u64*)bits, W, select, w.active);
    int32_t st = psam_launch_status("psam_region_clean: rows launch failed");
    if (st != PSAM_OK) return st;
    if (min_hole > 0) {
        st = region_components((const u64*)bits, inv, nbr, K, N, V, 1, w, false, stream, "psam_region_clean: hole component launch failed");
        if (st != PSAM_OK) return st;
    }
    hipLaunchKernelGGL(region_fill_kernel, wgrid, threads, 0, stream, (const u64*)bits, W, inv, (const int*)w.parent, (const int*)w.size, (const int*)w.active,
                       (int)N, (int)V, (int)min_hole, (u64*)bits_out);
    if ((st = psam_launch_status("psam_region_clean: fill launch failed")) != PSAM_OK) return st;
    if (min_island > 0 || S > 0) {
        st = region_components((const u64*)bits_out, inv, nbr, K, N, V, 0, w, true, stream, "psam_region_clean: island component launch failed");
        if (st != PSAM_OK) return st;
        hipLaunchKernelGGL(region_best_kernel, dim3(region_blocks(V), (unsigned)K), threads, 0, stream, (const int*)w.cnt, (const int*)w.parent,
                           (const int*)w.size, (int)V, w.best);
        if ((st = psam_launch_status("psam_region_clean: best launch failed")) != PSAM_OK) return st;
        if (S > 0) {
            hipLaunchKernelGGL(region_seed_kernel, dim3(region_blocks((int64_t)K * S)), threads, 0, stream, (const u64*)bits_out, W, inv, (const int*)w.parent,
                               (const int*)w.size, (const u64*)w.best, (const int*)w.active, seeds, (int)K, (int)N, (int)V, (int)S, (int)min_island, w.flag,
                               w.any_seed);
            if ((st = psam_launch_status("psam_region_clean: seed launch failed")) != PSAM_OK) return st;
        }
        hipLaunchKernelGGL(region_final_kernel, wgrid, threads, 0, stream, (u64*)bits_out, W, inv, (const int*)w.parent, (const int*)w.size, (const u64*)w.best,
                           (const int*)w.active, (const int*)w.flag, (const int*)w.any_seed, (int)N, (int)V, (int)min_island);
        if ((st = psam_launch_status("psam_region_clean: final launch failed")) != PSAM_OK) return st;
    }
    hipLaunchKernelGGL(region_area_kernel, dim3((unsigned)K), threads, 0, stream, (const u64*)bits, (const u64*)bits_out, W, area_out, changed);
    return psam_launch_status("psam_region_clean: area launch failed");
}
