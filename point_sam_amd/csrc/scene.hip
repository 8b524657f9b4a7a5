// Full-resolution scenes (point_sam_amd/scene.py): a scan of M points is reduced to a working cloud of one real point per occupied voxel, the model runs on
// the working cloud, and every point of the scan receives the result of its voxel's representative.  Everything here is integer work or a bit-for-bit
// copy, so every output is exact and reproducible:
//   psam_voxel_downsample    xyz [M, 3] -> keep_idx [count] (the lowest index of every occupied voxel, increasing) and inv [M] (position in keep_idx
//                            of each point's representative); with both NULL only the count
//   psam_scene_expand_rows   dst[r, i] = src[r, inv[i]] for rows of 32-bit words (fp32 logits, int32 labels)
//   psam_scene_expand_bits   bit i of full row k = bit inv[i] of working row k (the packed masks of csrc/masks.hip), and the full rows' popcounts
//
// Downsample.  Workspace = an open-addressing table of C = 2^ceil(log2(2 M)) slots (load factor <= 0.5): keys [C] u64, lowest index [C] u32; then
// one int32 per point and one int32 per block of SCAN_THREADS points.  Launches, each a kernel boundary (no value is handed over inside a kernel):
//   clear    keys = all ones (no voxel key has bit 63), lowest index = all ones, *flag = 0
//   insert   cell -> key -> linear probing from a hash of the key: a slot is claimed by compare-and-swap on the key, the lowest point index of the
//            slot kept by an unsigned atomic minimum; the point's slot goes to slot[i].  A run of equal keys on consecutive lanes is one probe
//            and one minimum (by the run's first lane, whose index is the run's lowest).
//   look-up  rep[i] = lowest index of slot[i] (in place of slot[i]); per block the number of points that are their own representative
//   offsets  exclusive scan of the block counts, the total -> *count
//   rank     rank of a representative = block offset + the waves before it + the ballot bits below its lane; keep_idx[rank] = i, and rep[i] = ~rank
//   inverse  inv[i] = rank of rep[i]
// Which slot a key lands in depends on the arrival order of the waves; slot numbers never leave the workspace, and the lowest index of a slot,
// the flags and the ranks do not depend on them.
#include "common.h"
#include "voxel_cell.h"      // cells, keys, the hash, the table's capacity: shared with regions.hip

#include <cmath>

constexpr int SCAN_THREADS = 1024;                // points per block of the look-up and rank kernels
constexpr int SCAN_WAVES = SCAN_THREADS / WAVE;
constexpr int VOXEL_THREADS = 256;

static inline int64_t scan_blocks(int64_t M) { return psam_cdiv(M, SCAN_THREADS); }

struct VoxelWs {
    u64* keys;            // [C]
    unsigned* low;        // [C]
    int* rep;             // [M]: slot, then representative, then (representatives only) ~rank
    int* block;           // [blocks + 1]
    size_t bytes;
};

static inline VoxelWs voxel_layout(void* ws, int64_t M) {
    const int64_t C = voxel_capacity(M);
    VoxelWs w;
    char* p = (char*)ws;
    size_t o = 0;
    w.keys = (u64*)(p + o);       o += align16((size_t)C * sizeof(u64));
    w.low = (unsigned*)(p + o);   o += align16((size_t)C * sizeof(unsigned));
    w.rep = (int*)(p + o);        o += align16((size_t)M * sizeof(int));
    w.block = (int*)(p + o);      o += align16(((size_t)scan_blocks(M) + 1) * sizeof(int));
    w.bytes = o;
    return w;
}

// ------------------------------------------------------------------------------------------------ clear
// keys and lowest indices are adjacent in the workspace (16-byte granules): one fill of all-ones words
__global__ __launch_bounds__(VOXEL_THREADS) void voxel_clear_kernel(uint4* __restrict__ table, int64_t granules, int* __restrict__ flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < granules; g += stride) table[g] = make_uint4(~0u, ~0u, ~0u, ~0u);
    if (blockIdx.x == 0 && threadIdx.x == 0) *flag = 0;
}

// ------------------------------------------------------------------------------------------------ insert
__global__ __launch_bounds__(VOXEL_THREADS) void voxel_insert_kernel(const float* __restrict__ xyz, int M, float ox, float oy, float oz, float inv_h,
                                                                    u64* __restrict__ keys, unsigned* __restrict__ low, int capacity,
                                                                    int* __restrict__ slot_of, int* __restrict__ flag) {
    const int i = blockIdx.x * VOXEL_THREADS + threadIdx.x;      // whole waves stay in the kernel: the cross-lane steps below need every lane
    const int lane = threadIdx.x & 63;
    u64 key = VOXEL_EMPTY;
    if (i < M) {
        u64 cx, cy, cz;
        const bool ok = voxel_axis(xyz[(int64_t)i * 3 + 0], ox, inv_h, cx) & voxel_axis(xyz[(int64_t)i * 3 + 1], oy, inv_h, cy) &
                        voxel_axis(xyz[(int64_t)i * 3 + 2], oz, inv_h, cz);
        if (ok) key = voxel_key(cx, cy, cz);
        else *flag = 1;                                            // every writer stores the same value
    }
    // a run of equal keys on consecutive lanes: its first lane probes and takes the minimum for all of them
    const u64 prev = __shfl_up(key, 1, 64);
    const bool leader = lane == 0 || prev != key;
    const u64 leaders = __ballot(leader);
    int slot = -1;
    if (leader && key != VOXEL_EMPTY) {
        const unsigned mask = (unsigned)capacity - 1u;
        unsigned pos = (unsigned)voxel_hash(key) & mask;
        for (int probe = 0; probe < capacity; ++probe) {           // at most M of the >= 2 M slots are ever taken: an empty one always ends the walk
            u64 cur = __hip_atomic_load(&keys[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == VOXEL_EMPTY) cur = atomicCAS(&keys[pos], VOXEL_EMPTY, key);
            if (cur == VOXEL_EMPTY || cur == key) { slot = (int)pos; break; }
            pos = (pos + 1u) & mask;
        }
        if (slot >= 0) atomicMin(&low[slot], (unsigned)i);
    }
    const int first = 63 - __clzll(leaders & (~0ull >> (63 - lane)));      // the run's first lane: the highest leader at or below this lane
    slot = __shfl(slot, first, 64);
    if (i < M) slot_of[i] = slot;
}

// ------------------------------------------------------------------------------------------------ look-up, offsets, rank, inverse
// A point without a cell (flag raised: the caller discards the outputs) counts as its own representative, so every index stays in range.
__global__ __launch_bounds__(SCAN_THREADS) void voxel_lookup_kernel(int* __restrict__ rep, const unsigned* __restrict__ low, int M,
                                                                   int* __restrict__ block_count) {
    __shared__ int s_cnt[SCAN_WAVES];
    const int i = blockIdx.x * SCAN_THREADS + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool own = false;
    if (i < M) {
        const int slot = rep[i];
        const int r = slot >= 0 ? (int)low[slot] : i;
        rep[i] = r;
        own = r == i;
    }
    const u64 m = __ballot(own);
    if (lane == 0) s_cnt[wave] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < SCAN_WAVES; ++w) s += s_cnt[w];
        block_count[blockIdx.x] = s;
    }
}

// second level: one workgroup, a contiguous span of block counts per thread; in place, the total lands behind the last block and in *count
__global__ __launch_bounds__(SCAN_THREADS) void voxel_offsets_kernel(int* __restrict__ block, int blocks, int* __restrict__ count) {
    __shared__ int s_sum[SCAN_THREADS];
    __shared__ int s_wave[SCAN_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (blocks + SCAN_THREADS - 1) / SCAN_THREADS;
    const int lo = min(tid * per, blocks), hi = min(lo + per, blocks);
    int c = 0;
    for (int b = lo; b < hi; ++b) c += block[b];
    // inclusive scan of the 1024 span sums: inside each wave by shuffles, then over the 16 wave totals
    int inc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d, 64); if (lane >= d) inc += t; }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += s_wave[w];
    s_sum[tid] = before + inc - c;                                 // exclusive
    __syncthreads();
    int run = s_sum[tid];
    for (int b = lo; b < hi; ++b) { const int v = block[b]; block[b] = run; run += v; }
    if (tid == SCAN_THREADS - 1) { block[blocks] = run; *count = run; }
}

__global__ __launch_bounds__(SCAN_THREADS) void voxel_rank_kernel(int* __restrict__ rep, int M, const int* __restrict__ block_offset,
                                                                 int64_t* __restrict__ keep_idx) {
    __shared__ int s_cnt[SCAN_WAVES];
    const int i = blockIdx.x * SCAN_THREADS + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool own = i < M && rep[i] == i;
    const u64 m = __ballot(own);
    if (lane == 0) s_cnt[wave] = __popcll(m);
    __syncthreads();
    if (!own) return;
    int rank = block_offset[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) rank += s_cnt[w];
    keep_idx[rank] = i;
    rep[i] = ~rank;                                                // read by the inverse kernel; only this thread touches rep[i] here
}

__global__ __launch_bounds__(VOXEL_THREADS) void voxel_inverse_kernel(const int* __restrict__ rep, int M, int64_t* __restrict__ inv) {
    const int i = blockIdx.x * VOXEL_THREADS + threadIdx.x;
    if (i >= M) return;
    int r = rep[i];
    if (r >= 0) r = rep[r];                                        // a representative's entry is ~rank (negative)
    inv[i] = (int64_t)~r;
}

PSAM_API size_t psam_voxel_downsample_workspace_bytes(int32_t M) {
    if (M <= 0 || M > VOXEL_MAX_POINTS) return 0;
    return voxel_layout(nullptr, M).bytes;
}

PSAM_API int32_t psam_voxel_downsample(const float* xyz, int32_t M, const float* origin, float inv_h, int64_t* keep_idx, int64_t* inv, int32_t* count,
                                       int32_t* flag, void* ws, size_t ws_bytes, hipStream_t stream) {
    PSAM_REQUIRE(xyz && origin && count && flag && ws, PSAM_EINVAL, "psam_voxel_downsample: null pointer");
    PSAM_REQUIRE((keep_idx == nullptr) == (inv == nullptr), PSAM_EINVAL, "psam_voxel_downsample: keep_idx and inv are given together or both null (count only)");
    PSAM_REQUIRE(M > 0 && M <= VOXEL_MAX_POINTS, PSAM_EINVAL, "psam_voxel_downsample: need 0 < M <= 2^28");
    PSAM_REQUIRE(std::isfinite(inv_h) && inv_h > 0.0f, PSAM_EINVAL, "psam_voxel_downsample: inv_h must be finite and positive");
    PSAM_REQUIRE(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]), PSAM_EINVAL, "psam_voxel_downsample: origin must be finite");
    PSAM_REQUIRE(ws_bytes >= psam_voxel_downsample_workspace_bytes(M), PSAM_EINVAL,
                 "psam_voxel_downsample: workspace too small (psam_voxel_downsample_workspace_bytes)");
    PSAM_REQUIRE(((uintptr_t)ws & 15) == 0, PSAM_EALIGN, "psam_voxel_downsample: workspace must be 16-byte aligned");
    const VoxelWs w = voxel_layout(ws, M);
    const int capacity = (int)voxel_capacity(M);
    const int64_t granules = ((char*)w.rep - (char*)w.keys) / 16;
    const unsigned point_blocks = (unsigned)psam_cdiv(M, VOXEL_THREADS), blocks = (unsigned)scan_blocks(M);
    hipLaunchKernelGGL(voxel_clear_kernel, dim3((unsigned)(granules < 4096 * VOXEL_THREADS ? psam_cdiv(granules, VOXEL_THREADS) : 4096)), dim3(VOXEL_THREADS),
                       0, stream, (uint4*)w.keys, granules, flag);
    int32_t st = psam_launch_status("psam_voxel_downsample: clear launch failed");
    if (st != PSAM_OK) return st;
    hipLaunchKernelGGL(voxel_insert_kernel, dim3(point_blocks), dim3(VOXEL_THREADS), 0, stream, xyz, (int)M, origin[0], origin[1], origin[2], inv_h, w.keys,
                       w.low, capacity, w.rep, flag);
    if ((st = psam_launch_status("psam_voxel_downsample: insert launch failed")) != PSAM_OK) return st;
    hipLaunchKernelGGL(voxel_lookup_kernel, dim3(blocks), dim3(SCAN_THREADS), 0, stream, w.rep, (const unsigned*)w.low, (int)M, w.block);
    if ((st = psam_launch_status("psam_voxel_downsample: look-up launch failed")) != PSAM_OK) return st;
    hipLaunchKernelGGL(voxel_offsets_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, w.block, (int)blocks, count);
    if ((st = psam_launch_status("psam_voxel_downsample: offsets launch failed")) != PSAM_OK) return st;
    if (!keep_idx) return PSAM_OK;
    hipLaunchKernelGGL(voxel_rank_kernel, dim3(blocks), dim3(SCAN_THREADS), 0, stream, w.rep, (int)M, (const int*)w.block, keep_idx);
    if ((st = psam_launch_status("psam_voxel_downsample: rank launch failed")) != PSAM_OK) return st;
    hipLaunchKernelGGL(voxel_inverse_kernel, dim3(point_blocks), dim3(VOXEL_THREADS), 0, stream, (const int*)w.rep, (int)M, inv);
    return psam_launch_status("psam_voxel_downsample: inverse launch failed");
}

// ------------------------------------------------------------------------------------------------ expand rows
// One thread per scan point: inv[i] is read once, then one gathered word and one coalesced store per row.  An index outside [0, Nw) (never
// produced by psam_voxel_downsample) reads nothing and stores a zero word.
__global__ __launch_bounds__(VOXEL_THREADS) void scene_expand_rows_kernel(const unsigned* __restrict__ src, int64_t src_ld, const int64_t* __restrict__ inv,
                                                                         int R, int Nw, int M, unsigned* __restrict__ dst, int64_t dst_ld) {
    const int i = blockIdx.x * VOXEL_THREADS + threadIdx.x;
    if (i >= M) return;
    const int64_t j = inv[i];
    const bool ok = (u64)j < (u64)Nw;
    int r = 0;
    for (; r + 4 <= R; r += 4) {
        unsigned v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = ok ? src[(int64_t)(r + u) * src_ld + j] : 0u;
#pragma unroll
        for (int u = 0; u < 4; ++u) dst[(int64_t)(r + u) * dst_ld + i] = v[u];
    }
    for (; r < R; ++r) dst[(int64_t)r * dst_ld + i] = ok ? src[(int64_t)r * src_ld + j] : 0u;
}

PSAM_API int32_t psam_scene_expand_rows(const void* src, int64_t src_ld, const int64_t* inv, int32_t R, int32_t Nw, int32_t M, void* dst, int64_t dst_ld,
                                        hipStream_t stream) {
    PSAM_REQUIRE(src && inv && dst, PSAM_EINVAL, "psam_scene_expand_rows: null pointer");
    PSAM_REQUIRE(R > 0 && Nw > 0 && M > 0 && src_ld >= Nw && dst_ld >= M, PSAM_EINVAL,
                 "psam_scene_expand_rows: need R > 0, Nw > 0, M > 0, src_ld >= Nw, dst_ld >= M");
    PSAM_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 3) == 0, PSAM_EALIGN, "psam_scene_expand_rows: src and dst must be 4-byte aligned");
    hipLaunchKernelGGL(scene_expand_rows_kernel, dim3((unsigned)psam_cdiv(M, VOXEL_THREADS)), dim3(VOXEL_THREADS), 0, stream, (const unsigned*)src, src_ld, inv,
                       (int)R, (int)Nw, (int)M, (unsigned*)dst, dst_ld);
    return psam_launch_status("psam_scene_expand_rows: launch failed");
}

// ------------------------------------------------------------------------------------------------ expand bits
// A wave owns 64 consecutive scan points per output word and BITS_WORDS consecutive words: every lane loads its BITS_WORDS indices once, then for
// every row the ballot of the tested bit IS the output word, and lanes 0 .. BITS_WORDS - 1 store the wave's words of the row as one contiguous
// 64-byte segment.  The working row is read as 32-bit halves (little endian: bit j of the row is bit j % 32 of half j / 32): a working cloud's row is a
// few KiB and stays in cache.  Points past M and indices outside [0, Nw) give a zero bit.  The areas are a pass of their own over the finished rows.
constexpr int BITS_WORDS = 8;
constexpr int BITS_THREADS = 256;
constexpr int BITS_BLOCK_WORDS = BITS_WORDS * BITS_THREADS / WAVE;

__global__ __launch_bounds__(BITS_THREADS) void scene_expand_bits_kernel(const unsigned* __restrict__ bits_w, int64_t Ww, const int64_t* __restrict__ inv,
                                                                        int K, int Nw, int M, u64* __restrict__ bits_f, int64_t Wf) {
    const int lane = threadIdx.x & 63;
    const int64_t w0 = ((int64_t)blockIdx.x * (BITS_THREADS / WAVE) + (threadIdx.x >> 6)) * BITS_WORDS;
    if (w0 >= Wf) return;                                          // wave-uniform
    int j[BITS_WORDS];
#pragma unroll
    for (int u = 0; u < BITS_WORDS; ++u) {
        const int64_t i = (w0 + u) * 64 + lane;
        const int64_t v = i < M ? inv[i] : -1;
        j[u] = (u64)v < (u64)Nw ? (int)v : -1;
    }
    const bool store = lane < BITS_WORDS && w0 + lane < Wf;
    for (int k = 0; k < K; ++k) {
        const unsigned* __restrict__ row = bits_w + (int64_t)k * Ww * 2;
        unsigned half[BITS_WORDS];
#pragma unroll
        for (int u = 0; u < BITS_WORDS; ++u) half[u] = j[u] >= 0 ? row[j[u] >> 5] : 0u;
        u64 mine = 0;
#pragma unroll
        for (int u = 0; u < BITS_WORDS; ++u) {
            const u64 m = __ballot(j[u] >= 0 && ((half[u] >> (j[u] & 31)) & 1u));
            mine = lane == u ? m : mine;
        }
        if (store) bits_f[(int64_t)k * Wf + w0 + lane] = mine;
    }
}

constexpr int AREA_THREADS = 256;

__global__ __launch_bounds__(AREA_THREADS) void scene_area_kernel(const u64* __restrict__ bits_f, int64_t Wf, int* __restrict__ area) {
    __shared__ int s_cnt[AREA_THREADS / WAVE];
    const u64* __restrict__ row = bits_f + (int64_t)blockIdx.x * Wf;
    int c = 0;
    for (int64_t w = threadIdx.x; w < Wf; w += AREA_THREADS) c += __popcll(row[w]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < AREA_THREADS / WAVE; ++w) s += s_cnt[w];
        area[blockIdx.x] = s;
    }
}

PSAM_API int32_t psam_scene_expand_bits(const uint64_t* bits_w, const int64_t* inv, int32_t K, int32_t Nw, int32_t M, uint64_t* bits_f, int32_t* area_f,
                                        hipStream_t stream) {
    PSAM_REQUIRE(bits_w && inv && bits_f, PSAM_EINVAL, "psam_scene_expand_bits: null pointer");
    PSAM_REQUIRE(K > 0 && Nw > 0 && M > 0, PSAM_EINVAL, "psam_scene_expand_bits: need K > 0, Nw > 0, M > 0");
    const int64_t Ww = psam_cdiv(Nw, 64), Wf = psam_cdiv(M, 64);
    hipLaunchKernelGGL(scene_expand_bits_kernel, dim3((unsigned)psam_cdiv(Wf, BITS_BLOCK_WORDS)), dim3(BITS_THREADS), 0, stream, (const unsigned*)bits_w, Ww,
                       inv, (int)K, (int)Nw, (int)M, (u64*)bits_f, Wf);
    int32_t st = psam_launch_status("psam_scene_expand_bits: launch failed");
    if (st != PSAM_OK || !area_f) return st;
    hipLaunchKernelGGL(scene_area_kernel, dim3((unsigned)K), dim3(AREA_THREADS), 0, stream, (const u64*)bits_f, Wf, area_f);
    return psam_launch_status("psam_scene_expand_bits: area launch failed");
}
