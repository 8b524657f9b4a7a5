// Superpoints (point_sam_amd/superpoints.py): a geometric over-segmentation of a cloud into small, roughly planar patches, grown on the voxel graph of
// regions.hip from the normals of normals.hip, and the snapping of packed masks to whole superpoints.  Integers, bits and a fixed fp64 expression: every
// output is exact and does not depend on the order in which the waves run.
//
// psam_superpoints, every launch a kernel boundary:
//   init      own = 0, parent[v] = v, size = 0, used = 0, and the caller's size [V] = 0
//   own       own[inv[n]] += 1: the points of every voxel
//   hook      union-find (region_union.h) over the edges (v, nbr[v, o]), o < 13, that pass the join rule below
//   flatten   label[v] = root(v) = the lowest voxel rank of v's component; size[label] += own[v]
//   absorb    `rounds` times, double-buffered: a voxel of a superpoint below min_size points takes the label of its best neighbour in a superpoint of
//             at least min_size points (labels and sizes as they were at the start of the round); then the sizes are counted again
//   compact   the labels still in use, in increasing order of their value, become 0 .. S - 1 (the ballot scan of voxel_table.h)
// Join rule of an edge (v, u): count >= min_points and curvature <= max_curvature at both ends, and |n_v . n_u| >= cos_angle with the dot product in
// fp64 from the stored fp32 normals, (x x' + y y') + z z': each product is exact (48 significant bits), the two additions round, nothing is contracted.
//
// psam_superpoint_snap: cnt[k, s] = the set bits of row k whose point has label s, counted by walking the set bits (the walk of geometry.hip: a wave owns
// 256 consecutive words of a row, four per lane) with integer atomic adds; then one wave per output word, whose ballot is the word.
#include "common.h"
#include "region_union.h"
#include "row_popcount.h"    // block_sum
#include "voxel_table.h"     // the ballot scan

#include <cmath>

constexpr int SP_THREADS = 256;
constexpr int SP_WAVES = SP_THREADS / WAVE;
constexpr int SP_MAX_POINTS = 1 << 28;
constexpr int SP_MAX_ROWS = 65535;                 // rows are the grid's y dimension
constexpr int SP_MAX_ROUNDS = 64;
constexpr int SP_LANE_WORDS = 4;
constexpr int SP_RANGE_WORDS = WAVE * SP_LANE_WORDS;

static inline unsigned sp_blocks(int64_t n) { return (unsigned)psam_cdiv(n, SP_THREADS); }

// |n_v . n_u| as the contract writes it
__device__ __forceinline__ double sp_dot(const float* __restrict__ normal, int v, int u) {
#pragma clang fp contract(off)
    const double x = (double)normal[(int64_t)v * 3 + 0] * (double)normal[(int64_t)u * 3 + 0];
    const double y = (double)normal[(int64_t)v * 3 + 1] * (double)normal[(int64_t)u * 3 + 1];
    const double z = (double)normal[(int64_t)v * 3 + 2] * (double)normal[(int64_t)u * 3 + 2];
    return fabs((x + y) + z);
}

// ------------------------------------------------------------------------------------------------ union
__global__ __launch_bounds__(SP_THREADS) void sp_init_kernel(int* __restrict__ own, int* __restrict__ parent, int* __restrict__ size, int* __restrict__ used,
                                                           int* __restrict__ size_out, int V) {
    const int v = blockIdx.x * SP_THREADS + threadIdx.x;
    if (v >= V) return;
    own[v] = 0;
    parent[v] = v;
    size[v] = 0;
    used[v] = 0;
    size_out[v] = 0;                                               // the caller's [V]: entries from S on stay zero
}

__global__ __launch_bounds__(SP_THREADS) void sp_own_kernel(const int64_t* __restrict__ inv, int N, int V, int* __restrict__ own) {
    const int n = blockIdx.x * SP_THREADS + threadIdx.x;
    if (n >= N) return;
    const int64_t v = inv[n];
    if ((u64)v < (u64)V) atomicAdd(&own[v], 1);
}

__device__ __forceinline__ bool sp_smooth(const int* __restrict__ count, const float* __restrict__ curvature, int v, int min_points, float max_curvature) {
    return count[v] >= min_points && curvature[v] <= max_curvature;
}

__global__ __launch_bounds__(SP_THREADS) void sp_hook_kernel(const int* __restrict__ count, const float* __restrict__ curvature,
                                                           const float* __restrict__ normal, const int* __restrict__ nbr, int V, int min_points,
                                                           float max_curvature, double cos_angle, int* parent) {
    const int v = blockIdx.x * SP_THREADS + threadIdx.x;
    if (v >= V || !sp_smooth(count, curvature, v, min_points, max_curvature)) return;
    for (int o = 0; o < 13; ++o) {      // the other 13 offsets are the same edges seen from the far end
        const int u = nbr[(int64_t)v * 26 + o];
        if ((unsigned)u >= (unsigned)V || !sp_smooth(count, curvature, u, min_points, max_curvature)) continue;
        if (sp_dot(normal, v, u) >= cos_angle) region_union(parent, v, u, V);
    }
    region_shorten(parent, v, V);
}

__global__ __launch_bounds__(SP_THREADS) void sp_flatten_kernel(const int* __restrict__ own, int* parent, int* __restrict__ size, int V) {
    const int v = blockIdx.x * SP_THREADS + threadIdx.x;
    if (v >= V) return;
    const int r = region_flatten(parent, v, V);
    if (own[v] > 0) atomicAdd(&size[r], own[v]);
}

// ------------------------------------------------------------------------------------------------ absorb
// One round: label_in / size_in are the round's start, label_out the result; size_out is cleared here and counted by sp_size_kernel.
__global__ __launch_bounds__(SP_THREADS) void sp_absorb_kernel(const int* __restrict__ label_in, const int* __restrict__ size_in,
                                                             const float* __restrict__ normal, const int* __restrict__ nbr, int V, int min_size,
                                                             int* __restrict__ label_out, int* __restrict__ size_out) {
    const int v = blockIdx.x * SP_THREADS + threadIdx.x;
    if (v >= V) return;
    int best = label_in[v];
    if (size_in[best] < min_size) {
        double score = -1.0;
        for (int o = 0; o < 26; ++o) {
            const int u = nbr[(int64_t)v * 26 + o];
            if ((unsigned)u >= (unsigned)V) continue;
            const int l = label_in[u];
            if (size_in[l] < min_size) continue;
            const double d = sp_dot(normal, v, u);                 // an invalid normal is (0, 0, 0): the product is 0
            if (d > score || (d == score && l < best)) { score = d; best = l; }
        }
    }
    label_out[v] = best;
    size_out[v] = 0;
}

__global__ __launch_bounds__(SP_THREADS) void sp_size_kernel(const int* __restrict__ label, const int* __restrict__ own, int V, int* __restrict__ size) {
    const int v = blockIdx.x * SP_THREADS + threadIdx.x;
    if (v < V && own[v] > 0) atomicAdd(&size[label[v]], own[v]);
}

// ------------------------------------------------------------------------------------------------ compact
__global__ __launch_bounds__(SP_THREADS) void sp_used_kernel(const int* __restrict__ label, int V, int* __restrict__ used) {
    const int v = blockIdx.x * SP_THREADS + threadIdx.x;
    if (v < V) used[label[v]] = 1;                                 // every writer stores the same value
}

// Blocks of SCAN_THREADS consecutive voxel ranks; a ballot word for every wave of every block, also of the last one's tail.
__global__ __launch_bounds__(SCAN_THREADS) void sp_mark_kernel(const int* __restrict__ used, int V, u64* __restrict__ ballots, int* __restrict__ block_count) {
    __shared__ int s_cnt[SCAN_WAVES];
    const int v = blockIdx.x * SCAN_THREADS + threadIdx.x;
    const u64 m = scan_note(v < V && used[v] != 0, s_cnt);
    if ((threadIdx.x & 63) == 0) ballots[v >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = scan_total(s_cnt);
}

__global__ __launch_bounds__(SCAN_THREADS) void sp_offsets_kernel(int* __restrict__ block, int blocks, int* __restrict__ count) {
    int lo, hi, c = 0;
    scan_span(blocks, threadIdx.x, lo, hi);
    for (int b = lo; b < hi; ++b) c += block[b];
    scan_block_offsets(block, blocks, lo, hi, c, count);
}

// used[v] becomes the new id of label v (labels in use only); size_out[id] = its points
__global__ __launch_bounds__(SCAN_THREADS) void sp_rank_kernel(const u64* __restrict__ ballots, const int* __restrict__ block_offset,
                                                             const int* __restrict__ size, int V, int* __restrict__ used, int* __restrict__ size_out) {
    __shared__ int s_cnt[SCAN_WAVES];
    const int v = blockIdx.x * SCAN_THREADS + threadIdx.x;
    const bool keep = (ballots[v >> 6] >> (threadIdx.x & 63)) & 1ull;      // one word per wave; bits of ranks past the end are 0
    const u64 m = scan_note(keep, s_cnt);
    __syncthreads();
    if (v >= V || !keep) return;
    const int id = scan_rank(m, s_cnt, block_offset[blockIdx.x]);
    used[v] = id;
    size_out[id] = size[v];
}

__global__ __launch_bounds__(SP_THREADS) void sp_voxel_label_kernel(const int* __restrict__ label, const int* __restrict__ id, int V,
                                                                  int* __restrict__ voxel_label) {
    const int v = blockIdx.x * SP_THREADS + threadIdx.x;
    if (v < V) voxel_label[v] = id[label[v]];
}

__global__ __launch_bounds__(SP_THREADS) void sp_point_label_kernel(const int* __restrict__ voxel_label, const int64_t* __restrict__ inv, int N, int V,
                                                                  int* __restrict__ point_label) {
    const int n = blockIdx.x * SP_THREADS + threadIdx.x;
    if (n >= N) return;
    const int64_t v = inv[n];
    point_label[n] = (u64)v < (u64)V ? voxel_label[v] : -1;
}

struct SuperWs {
    int* own;             // [V]
    int* label[2];        // [V]: parents, then labels, double-buffered by the absorb rounds
    int* size[2];         // [V]
    int* used;            // [V]: a label is in use, then its new id
    u64* ballots;         // [blocks * SCAN_WAVES]
    int* block;           // [blocks + 1]
    size_t bytes;
};

static inline SuperWs super_layout(void* ws, int64_t V) {
    SuperWs w = {};
    char* p = (char*)ws;
    size_t o = 0;
    const size_t row = align16((size_t)V * sizeof(int));
    w.own = (int*)(p + o);          o += row;
    w.label[0] = (int*)(p + o);     o += row;
    w.label[1] = (int*)(p + o);     o += row;
    w.size[0] = (int*)(p + o);      o += row;
    w.size[1] = (int*)(p + o);      o += row;
    w.used = (int*)(p + o);         o += row;
    w.ballots = (u64*)(p + o);      o += align16((size_t)scan_blocks(V) * SCAN_WAVES * sizeof(u64));
    w.block = (int*)(p + o);        o += align16(((size_t)scan_blocks(V) + 1) * sizeof(int));
    w.bytes = o;
    return w;
}

static inline bool super_shape_ok(int32_t N, int32_t V) { return N > 0 && N <= SP_MAX_POINTS && V > 0 && V <= N; }

PSAM_API size_t psam_superpoints_workspace_bytes(int32_t N, int32_t V) { return super_shape_ok(N, V) ? super_layout(nullptr, V).bytes : 0; }

PSAM_API int32_t psam_superpoints(const int64_t* inv, const int32_t* nbr, const int32_t* count, const float* normal, const float* curvature, int32_t N,
                                  int32_t V, int32_t min_points, float max_curvature, double cos_angle, int32_t min_size, int32_t absorb_rounds,
                                  int32_t* voxel_label, int32_t* point_label, int32_t* size, int32_t* num, void* ws, size_t ws_bytes, hipStream_t stream) {
    PSAM_REQUIRE(inv && nbr && count && normal && curvature && voxel_label && point_label && size && num && ws, PSAM_EINVAL,
                 "psam_superpoints: null pointer");
    PSAM_REQUIRE(super_shape_ok(N, V), PSAM_EINVAL, "psam_superpoints: need 0 < N <= 2^28 and 0 < V <= N");
    PSAM_REQUIRE(min_points >= 1 && min_size >= 0, PSAM_EINVAL, "psam_superpoints: need min_points >= 1 and min_size >= 0");
    PSAM_REQUIRE(absorb_rounds >= 0 && absorb_rounds <= SP_MAX_ROUNDS, PSAM_EINVAL, "psam_superpoints: absorb_rounds must be in 0 .. 64");
    PSAM_REQUIRE(max_curvature >= 0.0f && cos_angle >= -1.0 && cos_angle <= 1.0, PSAM_EINVAL,
                 "psam_superpoints: need max_curvature >= 0 and cos_angle in [-1, 1] (not NaN)");
    PSAM_REQUIRE(ws_bytes >= psam_superpoints_workspace_bytes(N, V), PSAM_EWORKSPACE,
                 "psam_superpoints: workspace too small (psam_superpoints_workspace_bytes)");
    PSAM_REQUIRE(((uintptr_t)ws & 15) == 0, PSAM_EALIGN, "psam_superpoints: workspace must be 16-byte aligned");
    const SuperWs w = super_layout(ws, V);
    const dim3 vgrid(sp_blocks(V)), ngrid(sp_blocks(N)), threads(SP_THREADS);
    const char* what = "psam_superpoints: union launch failed";
    hipLaunchKernelGGL(sp_init_kernel, vgrid, threads, 0, stream, w.own, w.label[0], w.size[0], w.used, (int*)size, (int)V);
    int32_t st = psam_launch_status(what);
    if (st != PSAM_OK) return st;
    hipLaunchKernelGGL(sp_own_kernel, ngrid, threads, 0, stream, inv, (int)N, (int)V, w.own);
    if ((st = psam_launch_status(what)) != PSAM_OK) return st;
    hipLaunchKernelGGL(sp_hook_kernel, vgrid, threads, 0, stream, (const int*)count, curvature, normal, (const int*)nbr, (int)V, (int)min_points, max_curvature,
                       cos_angle, w.label[0]);
    if ((st = psam_launch_status(what)) != PSAM_OK) return st;
    hipLaunchKernelGGL(sp_flatten_kernel, vgrid, threads, 0, stream, (const int*)w.own, w.label[0], w.size[0], (int)V);
    if ((st = psam_launch_status(what)) != PSAM_OK) return st;
    int cur = 0;
    what = "psam_superpoints: absorb launch failed";
    for (int r = 0; r < absorb_rounds && min_size > 0; ++r, cur ^= 1) {
        hipLaunchKernelGGL(sp_absorb_kernel, vgrid, threads, 0, stream, (const int*)w.label[cur], (const int*)w.size[cur], normal, (const int*)nbr, (int)V,
                           (int)min_size, w.label[cur ^ 1], w.size[cur ^ 1]);
        if ((st = psam_launch_status(what)) != PSAM_OK) return st;
        hipLaunchKernelGGL(sp_size_kernel, vgrid, threads, 0, stream, (const int*)w.label[cur ^ 1], (const int*)w.own, (int)V, w.size[cur ^ 1]);
        if ((st = psam_launch_status(what)) != PSAM_OK) return st;
    }
    what = "psam_superpoints: compact launch failed";
    const int blocks = (int)scan_blocks(V);
    hipLaunchKernelGGL(sp_used_kernel, vgrid, threads, 0, stream, (const int*)w.label[cur], (int)V, w.used);
    if ((st = psam_launch_status(what)) != PSAM_OK) return st;
    hipLaunchKernelGGL(sp_mark_kernel, dim3((unsigned)blocks), dim3(SCAN_THREADS), 0, stream, (const int*)w.used, (int)V, w.ballots, w.block);
    if ((st = psam_launch_status(what)) != PSAM_OK) return st;
    hipLaunchKernelGGL(sp_offsets_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, w.block, blocks, (int*)num);
    if ((st = psam_launch_status(what)) != PSAM_OK) return st;
    hipLaunchKernelGGL(sp_rank_kernel, dim3((unsigned)blocks), dim3(SCAN_THREADS), 0, stream, (const u64*)w.ballots, (const int*)w.block, (const int*)w.size[cur],
                       (int)V, w.used, (int*)size);
    if ((st = psam_launch_status(what)) != PSAM_OK) return st;
    hipLaunchKernelGGL(sp_voxel_label_kernel, vgrid, threads, 0, stream, (const int*)w.label[cur], (const int*)w.used, (int)V, (int*)voxel_label);
    if ((st = psam_launch_status(what)) != PSAM_OK) return st;
    hipLaunchKernelGGL(sp_point_label_kernel, ngrid, threads, 0, stream, (const int*)voxel_label, inv, (int)N, (int)V, (int*)point_label);
    return psam_launch_status("psam_superpoints: point label launch failed");
}

// ------------------------------------------------------------------------------------------------ snap
__global__ __launch_bounds__(SP_THREADS) void snap_clear_kernel(int* __restrict__ cnt, int64_t words) {
    const int64_t stride = (int64_t)gridDim.x * SP_THREADS;
    for (int64_t t = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x; t < words; t += stride) cnt[t] = 0;
}

// A wave owns SP_RANGE_WORDS consecutive words of row blockIdx.y; word j of lane l is base + 64 j + l, so every load of the wave is one contiguous
// 512-byte segment.  Bits at positions >= N are dropped before anything is indexed with them.
__global__ __launch_bounds__(SP_THREADS) void snap_count_kernel(const u64* __restrict__ bits, int64_t W, int N, const int* __restrict__ label, int S,
                                                              int* __restrict__ cnt) {
    const int lane = threadIdx.x & 63, k = blockIdx.y;
    const int64_t w0 = ((int64_t)blockIdx.x * SP_WAVES + (threadIdx.x >> 6)) * SP_RANGE_WORDS;
    if (w0 >= W) return;                                           // wave-uniform
    const u64* __restrict__ row = bits + (int64_t)k * W;
    int* __restrict__ c = cnt + (int64_t)k * S;
    u64 word[SP_LANE_WORDS];
#pragma unroll
    for (int j = 0; j < SP_LANE_WORDS; ++j) {
        const int64_t w = w0 + j * WAVE + lane;
        u64 m = w < W ? row[w] : 0ull;
        if (w == W - 1 && (N & 63)) m &= (1ull << (N & 63)) - 1ull;
        word[j] = m;
    }
#pragma unroll
    for (int j = 0; j < SP_LANE_WORDS; ++j) {
        const int base = (int)(w0 + j * WAVE + lane) * 64;         // < N <= 2^28 wherever a bit is set
        u64 m = word[j];
        while (m) {
            const int b = __builtin_ctzll(m);
            m &= m - 1;
            const int l = label[base + b];
            if ((unsigned)l < (unsigned)S) atomicAdd(&c[l], 1);
        }
    }
}

// One wave per output word: the ballot is the word, so bits past N are zero.
__global__ __launch_bounds__(SP_THREADS) void snap_write_kernel(const int* __restrict__ cnt, const int* __restrict__ label, const int* __restrict__ size, int W,
                                                              int N, int S, int q16, u64* __restrict__ out) {
    const int lane = threadIdx.x & 63, k = blockIdx.y;
    const int w = blockIdx.x * SP_WAVES + (threadIdx.x >> 6);
    if (w >= W) return;                                            // wave-uniform
    const int64_t n = (int64_t)w * 64 + lane;
    bool on = false;
    if (n < N) {
        const int l = label[n];
        if ((unsigned)l < (unsigned)S) on = (int64_t)cnt[(int64_t)k * S + l] * 65536 > (int64_t)q16 * (int64_t)size[l];
    }
    const u64 m = __ballot(on);
    if (lane == 0) out[(int64_t)k * W + w] = m;
}

// area[k] = the popcount of the output row; changed[k] = it differs from the input row in a bit below N
__global__ __launch_bounds__(SP_THREADS) void snap_area_kernel(const u64* __restrict__ bits, const u64* __restrict__ out, int W, int N, int* __restrict__ area,
                                                             unsigned char* __restrict__ changed) {
    __shared__ int s_cnt[SP_WAVES], s_diff[SP_WAVES];
    const int k = blockIdx.x;
    int c = 0, diff = 0;
    for (int w = threadIdx.x; w < W; w += SP_THREADS) {
        const u64 o = out[(int64_t)k * W + w];
        u64 in = bits[(int64_t)k * W + w];
        if (w == W - 1 && (N & 63)) in &= (1ull << (N & 63)) - 1ull;
        c += __popcll(o);
        diff |= o != in ? 1 : 0;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) diff |= __shfl_xor(diff, d, 64);
    if ((threadIdx.x & 63) == 0) s_diff[threadIdx.x >> 6] = diff;
    const int s = block_sum<SP_THREADS>(c, s_cnt);                 // its barrier is s_diff's too
    if (threadIdx.x == 0) {
        int f = 0;
        for (int w = 0; w < SP_WAVES; ++w) f |= s_diff[w];
        area[k] = s;
        changed[k] = f ? 1 : 0;
    }
}

static inline bool snap_shape_ok(int32_t K, int32_t N, int32_t S) {
    return K > 0 && K <= SP_MAX_ROWS && N > 0 && N <= SP_MAX_POINTS && S > 0 && S <= N;
}

PSAM_API size_t psam_superpoint_snap_workspace_bytes(int32_t K, int32_t N, int32_t S) {
    return snap_shape_ok(K, N, S) ? align16((size_t)K * (size_t)S * sizeof(int)) : 0;
}

PSAM_API int32_t psam_superpoint_snap(const uint64_t* bits, const int32_t* point_label, const int32_t* size, int32_t K, int32_t N, int32_t S, int32_t q16,
                                      uint64_t* bits_out, int32_t* area_out, uint8_t* changed, void* ws, size_t ws_bytes, hipStream_t stream) {
    PSAM_REQUIRE(bits && point_label && size && bits_out && area_out && changed && ws, PSAM_EINVAL, "psam_superpoint_snap: null pointer");
    PSAM_REQUIRE(snap_shape_ok(K, N, S), PSAM_EINVAL, "psam_superpoint_snap: need 0 < K <= 65535, 0 < N <= 2^28 and 0 < S <= N");
    PSAM_REQUIRE(q16 >= 0 && q16 <= 65535, PSAM_EINVAL, "psam_superpoint_snap: q16 must be in 0 .. 65535");
    PSAM_REQUIRE(bits_out != bits, PSAM_EINVAL, "psam_superpoint_snap: bits_out must not alias bits");
    PSAM_REQUIRE(ws_bytes >= psam_superpoint_snap_workspace_bytes(K, N, S), PSAM_EWORKSPACE,
                 "psam_superpoint_snap: workspace too small (psam_superpoint_snap_workspace_bytes)");
    PSAM_REQUIRE(((uintptr_t)ws & 15) == 0, PSAM_EALIGN, "psam_superpoint_snap: workspace must be 16-byte aligned");
    int* cnt = (int*)ws;
    const int64_t words = (int64_t)K * S;
    const int W = (int)psam_cdiv(N, 64);
    const dim3 threads(SP_THREADS);
    hipLaunchKernelGGL(snap_clear_kernel, dim3(words < 4096 * (int64_t)SP_THREADS ? sp_blocks(words) : 4096u), threads, 0, stream, cnt, words);
    int32_t st = psam_launch_status("psam_superpoint_snap: clear launch failed");
    if (st != PSAM_OK) return st;
    hipLaunchKernelGGL(snap_count_kernel, dim3((unsigned)psam_cdiv(psam_cdiv(W, SP_RANGE_WORDS), SP_WAVES), (unsigned)K), threads, 0, stream, (const u64*)bits,
                       (int64_t)W, (int)N, (const int*)point_label, (int)S, cnt);
    if ((st = psam_launch_status("psam_superpoint_snap: count launch failed")) != PSAM_OK) return st;
    hipLaunchKernelGGL(snap_write_kernel, dim3((unsigned)psam_cdiv(W, SP_WAVES), (unsigned)K), threads, 0, stream, (const int*)cnt, (const int*)point_label,
                       (const int*)size, W, (int)N, (int)S, (int)q16, (u64*)bits_out);
    if ((st = psam_launch_status("psam_superpoint_snap: write launch failed")) != PSAM_OK) return st;
    hipLaunchKernelGGL(snap_area_kernel, dim3((unsigned)K), threads, 0, stream, (const u64*)bits, (const u64*)bits_out, W, (int)N, area_out, changed);
    return psam_launch_status("psam_superpoint_snap: area launch failed");
}
