// Scene crops (point_sam_amd/scene.py: build_crop): a ball of a scan -- centre c, radius r -- becomes a cloud of its own, normalised to (x - c) / r,
// with its own (finer) voxel working cloud; the model runs on that cloud and the result is pasted back into the scan, with a fill value outside the
// ball.  Everything is integer work, a bit-for-bit copy or a fixed sequence of individually rounded fp32 operations (-ffp-contract=off), so every
// output is exact and reproducible:
//   psam_crop_downsample    xyz, rgb [M, 3] -> keep_idx [count] (the lowest MEMBER index of every occupied voxel of the ball, increasing), inv [M]
//                           (rank of each member's representative, -1 off the ball), wxyz [count, 3] (normalised), wrgb [count, 3]; count only
//                           with the four outputs NULL
//   psam_crop_expand_rows   dst[r, i] = inv[i] >= 0 ? src[r, inv[i]] : fill, rows of 32-bit words
//   psam_crop_expand_bits   bit i of full row k = inv[i] >= 0 ? bit inv[i] of crop row k : 0, and the full rows' popcounts
//
// Downsample.  The workspace is that of the scene's downsample (scene.hip): an open-addressing table of C = 2^ceil(log2(2 M)) slots, keys [C] u64 and
// lowest index [C] u32, one int32 per point, and two int32 per block of SCAN_THREADS points.  Launches, each a kernel boundary:
//   clear    keys and lowest indices = all ones, the three result words = 0
//   insert   membership (q <= r2), normalised coordinate, cell, key in ONE pass over xyz; only members are inserted (compare-and-swap on the key,
//            unsigned atomic minimum of the index), so a voxel's representative is a member.  state[i] = slot, NO_CELL (a member that is its own
//            representative: inv_h == 0, or a cell out of range with the flag raised) or OUTSIDE
//   look-up  state[i] = its representative's index (OUTSIDE stays); per block the representatives and the members
//   offsets  exclusive scan of the blocks' representatives -> count; sum of the blocks' members -> members
//   rank     rank of a representative from the block offset and the ballot; keep_idx[rank] = i, wxyz[rank] = u(i), wrgb[rank] = rgb[i];
//            state[i] = ~rank.  The gather rides on the rank pass: the representative's own thread holds i and rank, so no pass reads keep_idx back
//   inverse  inv[i] = rank of state[i], -1 for OUTSIDE
#include "common.h"
#include "crop_coord.h"      // CropBall, crop_member: shared with scene_interp.hip
#include "voxel_cell.h"

#include <climits>
#include <cmath>

constexpr int CROP_SCAN_THREADS = 1024;
constexpr int CROP_SCAN_WAVES = CROP_SCAN_THREADS / WAVE;
constexpr int CROP_THREADS = 256;
constexpr int CROP_NO_CELL = -1;                  // a member without a slot: its own representative
constexpr int CROP_OUTSIDE = INT_MIN;             // not a member; never a slot, an index or a ~rank (ranks stay below 2^28)

static inline int64_t crop_scan_blocks(int64_t M) { return psam_cdiv(M, CROP_SCAN_THREADS); }

struct CropWs {
    u64* keys;            // [C]
    unsigned* low;        // [C]
    int* state;           // [M]: slot / NO_CELL / OUTSIDE, then representative / OUTSIDE, then (representatives only) ~rank
    int* block;           // [blocks + 1]: representatives per block, then their exclusive scan and the total
    int* block_members;   // [blocks]
    size_t bytes;
};

static inline CropWs crop_layout(void* ws, int64_t M) {
    const int64_t C = voxel_capacity(M);
    CropWs w;
    char* p = (char*)ws;
    size_t o = 0;
    w.keys = (u64*)(p + o);            o += align16((size_t)C * sizeof(u64));
    w.low = (unsigned*)(p + o);        o += align16((size_t)C * sizeof(unsigned));
    w.state = (int*)(p + o);           o += align16((size_t)M * sizeof(int));
    w.block = (int*)(p + o);           o += align16(((size_t)crop_scan_blocks(M) + 1) * sizeof(int));
    w.block_members = (int*)(p + o);   o += align16((size_t)crop_scan_blocks(M) * sizeof(int));
    w.bytes = o;
    return w;
}

// ------------------------------------------------------------------------------------------------ clear
__global__ __launch_bounds__(CROP_THREADS) void crop_clear_kernel(uint4* __restrict__ table, int64_t granules, int* __restrict__ out3) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < granules; g += stride) table[g] = make_uint4(~0u, ~0u, ~0u, ~0u);
    if (blockIdx.x == 0 && threadIdx.x < 3) out3[threadIdx.x] = 0;
}

// ------------------------------------------------------------------------------------------------ insert
__global__ __launch_bounds__(CROP_THREADS) void crop_insert_kernel(const float* __restrict__ xyz, int M, CropBall ball, float inv_h, u64* __restrict__ keys,
                                                                  unsigned* __restrict__ low, int capacity, int* __restrict__ state, int* __restrict__ flag) {
    const int i = blockIdx.x * CROP_THREADS + threadIdx.x;       // whole waves stay in the kernel: the cross-lane steps below need every lane
    const int lane = threadIdx.x & 63;
    u64 key = VOXEL_EMPTY;
    bool member = false;
    if (i < M) {
        float u[3];
        member = crop_member(xyz + (int64_t)i * 3, ball, u);
        if (member && inv_h > 0.0f) {
            u64 cx, cy, cz;
            const bool okx = voxel_axis(u[0], -1.0f, inv_h, cx), oky = voxel_axis(u[1], -1.0f, inv_h, cy), okz = voxel_axis(u[2], -1.0f, inv_h, cz);
            if (okx && oky && okz) key = voxel_key(cx, cy, cz);
            else *flag = 1;                                        // every writer stores the same value
        }
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
    if (key == VOXEL_EMPTY) slot = member ? CROP_NO_CELL : CROP_OUTSIDE;   // a run of empty keys mixes members without a cell and points off the ball
    if (i < M) state[i] = slot;
}

// ------------------------------------------------------------------------------------------------ look-up, offsets, rank, inverse
__global__ __launch_bounds__(CROP_SCAN_THREADS) void crop_lookup_kernel(int* __restrict__ state, const unsigned* __restrict__ low, int M,
                                                                       int* __restrict__ block_count, int* __restrict__ block_members) {
    __shared__ int s_own[CROP_SCAN_WAVES];
    __shared__ int s_mem[CROP_SCAN_WAVES];
    const int i = blockIdx.x * CROP_SCAN_THREADS + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool own = false, member = false;
    if (i < M) {
        const int slot = state[i];
        member = slot != CROP_OUTSIDE;
        if (member) {
            const int r = slot >= 0 ? (int)low[slot] : i;
            state[i] = r;
            own = r == i;
        }
    }
    const u64 mo = __ballot(own), mm = __ballot(member);
    if (lane == 0) { s_own[wave] = __popcll(mo); s_mem[wave] = __popcll(mm); }
    __syncthreads();
    if (threadIdx.x == 0) {
        int a = 0, b = 0;
        for (int w = 0; w < CROP_SCAN_WAVES; ++w) { a += s_own[w]; b += s_mem[w]; }
        block_count[blockIdx.x] = a;
        block_members[blockIdx.x] = b;
    }
}

// one workgroup, a contiguous span of blocks per thread: the representatives' counts become their exclusive scan in place (total behind the last
// block and in out3[0]); the members' counts are only summed (out3[1])
__global__ __launch_bounds__(CROP_SCAN_THREADS) void crop_offsets_kernel(int* __restrict__ block, const int* __restrict__ block_members, int blocks,
                                                                        int* __restrict__ out3) {
    __shared__ int s_sum[CROP_SCAN_THREADS];
    __shared__ int s_wave[CROP_SCAN_WAVES];
    __shared__ int s_mem[CROP_SCAN_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (blocks + CROP_SCAN_THREADS - 1) / CROP_SCAN_THREADS;
    const int lo = min(tid * per, blocks), hi = min(lo + per, blocks);
    int c = 0, m = 0;
    for (int b = lo; b < hi; ++b) { c += block[b]; m += block_members[b]; }
    int inc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d, 64); if (lane >= d) inc += t; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m += __shfl_xor(m, d, 64);
    if (lane == 63) s_wave[wave] = inc;
    if (lane == 0) s_mem[wave] = m;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += s_wave[w];
    s_sum[tid] = before + inc - c;                                 // exclusive
    __syncthreads();
    int run = s_sum[tid];
    for (int b = lo; b < hi; ++b) { const int v = block[b]; block[b] = run; run += v; }
    if (tid == CROP_SCAN_THREADS - 1) { block[blocks] = run; out3[0] = run; }
    if (tid == 0) {
        int s = 0;
        for (int w = 0; w < CROP_SCAN_WAVES; ++w) s += s_mem[w];
        out3[1] = s;
    }
}

__global__ __launch_bounds__(CROP_SCAN_THREADS) void crop_rank_kernel(int* __restrict__ state, int M, const int* __restrict__ block_offset,
                                                                     const float* __restrict__ xyz, const float* __restrict__ rgb, CropBall ball,
                                                                     int64_t* __restrict__ keep_idx, float* __restrict__ wxyz, float* __restrict__ wrgb) {
    __shared__ int s_cnt[CROP_SCAN_WAVES];
    const int i = blockIdx.x * CROP_SCAN_THREADS + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool own = i < M && state[i] == i;
    const u64 m = __ballot(own);
    if (lane == 0) s_cnt[wave] = __popcll(m);
    __syncthreads();
    if (!own) return;
    int rank = block_offset[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) rank += s_cnt[w];
    keep_idx[rank] = i;
    state[i] = ~rank;                                              // read by the inverse kernel; only this thread touches state[i] here
    float u[3];
    crop_member(xyz + (int64_t)i * 3, ball, u);                    // the same operations as in the insert pass: the same bits
    const unsigned* __restrict__ c = (const unsigned*)rgb + (int64_t)i * 3;      // colours travel as words: bit for bit, NaN payloads included
    unsigned* __restrict__ oc = (unsigned*)wrgb + (int64_t)rank * 3;
    float* __restrict__ ou = wxyz + (int64_t)rank * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) { ou[a] = u[a]; oc[a] = c[a]; }
}

__global__ __launch_bounds__(CROP_THREADS) void crop_inverse_kernel(const int* __restrict__ state, int M, int64_t* __restrict__ inv) {
    const int i = blockIdx.x * CROP_THREADS + threadIdx.x;
    if (i >= M) return;
    int r = state[i];
    if (r == CROP_OUTSIDE) { inv[i] = -1; return; }
    if (r >= 0) r = state[r];                                      // a representative's entry is ~rank (negative, never CROP_OUTSIDE)
    inv[i] = (int64_t)~r;
}

PSAM_API size_t psam_crop_downsample_workspace_bytes(int32_t M) {
    if (M <= 0 || M > VOXEL_MAX_POINTS) return 0;
    return crop_layout(nullptr, M).bytes;
}

PSAM_API int32_t psam_crop_downsample(const float* xyz, const float* rgb, int32_t M, const float* center, float r2, float inv_r, float inv_h,
                                      int64_t* keep_idx, int64_t* inv, float* wxyz, float* wrgb, int32_t* result, void* ws, size_t ws_bytes,
                                      hipStream_t stream) {
    PSAM_REQUIRE(xyz && center && result && ws, PSAM_EINVAL, "psam_crop_downsample: null pointer");
    const bool full = keep_idx != nullptr;
    PSAM_REQUIRE((inv != nullptr) == full && (wxyz != nullptr) == full && (wrgb != nullptr) == full, PSAM_EINVAL,
                 "psam_crop_downsample: keep_idx, inv, wxyz and wrgb are given together or all null (count only)");
    PSAM_REQUIRE(!full || rgb, PSAM_EINVAL, "psam_crop_downsample: rgb is needed for wrgb");
    PSAM_REQUIRE(M > 0 && M <= VOXEL_MAX_POINTS, PSAM_EINVAL, "psam_crop_downsample: need 0 < M <= 2^28");
    PSAM_REQUIRE(std::isfinite(center[0]) && std::isfinite(center[1]) && std::isfinite(center[2]), PSAM_EINVAL, "psam_crop_downsample: center must be finite");
    PSAM_REQUIRE(std::isfinite(r2) && r2 > 0.0f && std::isfinite(inv_r) && inv_r > 0.0f, PSAM_EINVAL,
                 "psam_crop_downsample: r2 and inv_r must be finite and positive");
    PSAM_REQUIRE(std::isfinite(inv_h) && inv_h >= 0.0f, PSAM_EINVAL, "psam_crop_downsample: inv_h must be finite and positive, or 0 for no voxel reduction");
    PSAM_REQUIRE(ws_bytes >= psam_crop_downsample_workspace_bytes(M), PSAM_EINVAL,
                 "psam_crop_downsample: workspace too small (psam_crop_downsample_workspace_bytes)");
    PSAM_REQUIRE(((uintptr_t)ws & 15) == 0, PSAM_EALIGN, "psam_crop_downsample: workspace must be 16-byte aligned");
    const CropWs w = crop_layout(ws, M);
    const int capacity = (int)voxel_capacity(M);
    const int64_t granules = ((char*)w.state - (char*)w.keys) / 16;
    const unsigned point_blocks = (unsigned)psam_cdiv(M, CROP_THREADS), blocks = (unsigned)crop_scan_blocks(M);
    const CropBall ball = {center[0], center[1], center[2], r2, inv_r};
    hipLaunchKernelGGL(crop_clear_kernel, dim3((unsigned)(granules < 4096 * CROP_THREADS ? psam_cdiv(granules, CROP_THREADS) : 4096)), dim3(CROP_THREADS), 0,
                       stream, (uint4*)w.keys, granules, result);
    int32_t st = psam_launch_status("psam_crop_downsample: clear launch failed");
    if (st != PSAM_OK) return st;
    hipLaunchKernelGGL(crop_insert_kernel, dim3(point_blocks), dim3(CROP_THREADS), 0, stream, xyz, (int)M, ball, inv_h, w.keys, w.low, capacity, w.state,
                       result + 2);
    if ((st = psam_launch_status("psam_crop_downsample: insert launch failed")) != PSAM_OK) return st;
    hipLaunchKernelGGL(crop_lookup_kernel, dim3(blocks), dim3(CROP_SCAN_THREADS), 0, stream, w.state, (const unsigned*)w.low, (int)M, w.block, w.block_members);
    if ((st = psam_launch_status("psam_crop_downsample: look-up launch failed")) != PSAM_OK) return st;
    hipLaunchKernelGGL(crop_offsets_kernel, dim3(1), dim3(CROP_SCAN_THREADS), 0, stream, w.block, (const int*)w.block_members, (int)blocks, result);
    if ((st = psam_launch_status("psam_crop_downsample: offsets launch failed")) != PSAM_OK) return st;
    if (!full) return PSAM_OK;
    hipLaunchKernelGGL(crop_rank_kernel, dim3(blocks), dim3(CROP_SCAN_THREADS), 0, stream, w.state, (int)M, (const int*)w.block, xyz, rgb, ball, keep_idx, wxyz,
                       wrgb);
    if ((st = psam_launch_status("psam_crop_downsample: rank launch failed")) != PSAM_OK) return st;
    hipLaunchKernelGGL(crop_inverse_kernel, dim3(point_blocks), dim3(CROP_THREADS), 0, stream, (const int*)w.state, (int)M, inv);
    return psam_launch_status("psam_crop_downsample: inverse launch failed");
}

// ------------------------------------------------------------------------------------------------ expand rows
// One thread per scan point: inv[i] is read once, then one gathered word (or the fill) and one coalesced store per row.  Any index outside [0, Nw)
// takes the fill, -1 among them.
__global__ __launch_bounds__(CROP_THREADS) void crop_expand_rows_kernel(const unsigned* __restrict__ src, int64_t src_ld, const int64_t* __restrict__ inv, int R,
                                                                       int Nw, int M, unsigned fill, unsigned* __restrict__ dst, int64_t dst_ld) {
    const int i = blockIdx.x * CROP_THREADS + threadIdx.x;
    if (i >= M) return;
    const int64_t j = inv[i];
    const bool ok = (u64)j < (u64)Nw;
    int r = 0;
    for (; r + 4 <= R; r += 4) {
        unsigned v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = ok ? src[(int64_t)(r + u) * src_ld + j] : fill;
#pragma unroll
        for (int u = 0; u < 4; ++u) dst[(int64_t)(r + u) * dst_ld + i] = v[u];
    }
    for (; r < R; ++r) dst[(int64_t)r * dst_ld + i] = ok ? src[(int64_t)r * src_ld + j] : fill;
}

PSAM_API int32_t psam_crop_expand_rows(const void* src, int64_t src_ld, const int64_t* inv, int32_t R, int32_t Nw, int32_t M, uint32_t fill, void* dst,
                                       int64_t dst_ld, hipStream_t stream) {
    PSAM_REQUIRE(src && inv && dst, PSAM_EINVAL, "psam_crop_expand_rows: null pointer");
    PSAM_REQUIRE(R > 0 && Nw > 0 && M > 0 && src_ld >= Nw && dst_ld >= M, PSAM_EINVAL,
                 "psam_crop_expand_rows: need R > 0, Nw > 0, M > 0, src_ld >= Nw, dst_ld >= M");
    PSAM_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 3) == 0, PSAM_EALIGN, "psam_crop_expand_rows: src and dst must be 4-byte aligned");
    hipLaunchKernelGGL(crop_expand_rows_kernel, dim3((unsigned)psam_cdiv(M, CROP_THREADS)), dim3(CROP_THREADS), 0, stream, (const unsigned*)src, src_ld, inv,
                       (int)R, (int)Nw, (int)M, (unsigned)fill, (unsigned*)dst, dst_ld);
    return psam_launch_status("psam_crop_expand_rows: launch failed");
}

// ------------------------------------------------------------------------------------------------ expand bits
// The scheme of scene.hip's expand: a wave owns CROP_BITS_WORDS consecutive output words, every lane loads its indices once, the ballot of the tested
// bit is the output word.  Most of a scan lies off the ball: a wave whose 512 points are all non-members (wave-uniform test) stores zero words for
// every row and gathers nothing.
constexpr int CROP_BITS_WORDS = 8;
constexpr int CROP_BITS_THREADS = 256;
constexpr int CROP_BITS_BLOCK_WORDS = CROP_BITS_WORDS * CROP_BITS_THREADS / WAVE;

__global__ __launch_bounds__(CROP_BITS_THREADS) void crop_expand_bits_kernel(const unsigned* __restrict__ bits_w, int64_t Ww, const int64_t* __restrict__ inv,
                                                                            int K, int Nw, int M, u64* __restrict__ bits_f, int64_t Wf) {
    const int lane = threadIdx.x & 63;
    const int64_t w0 = ((int64_t)blockIdx.x * (CROP_BITS_THREADS / WAVE) + (threadIdx.x >> 6)) * CROP_BITS_WORDS;
    if (w0 >= Wf) return;                                          // wave-uniform
    int j[CROP_BITS_WORDS];
    bool any = false;
#pragma unroll
    for (int u = 0; u < CROP_BITS_WORDS; ++u) {
        const int64_t i = (w0 + u) * 64 + lane;
        const int64_t v = i < M ? inv[i] : -1;
        j[u] = (u64)v < (u64)Nw ? (int)v : -1;
        any |= j[u] >= 0;
    }
    const bool store = lane < CROP_BITS_WORDS && w0 + lane < Wf;
    if (__ballot(any) == 0) {                                      // wave-uniform: the whole span is off the ball
        if (store)
            for (int k = 0; k < K; ++k) bits_f[(int64_t)k * Wf + w0 + lane] = 0;
        return;
    }
    for (int k = 0; k < K; ++k) {
        const unsigned* __restrict__ row = bits_w + (int64_t)k * Ww * 2;
        unsigned half[CROP_BITS_WORDS];
#pragma unroll
        for (int u = 0; u < CROP_BITS_WORDS; ++u) half[u] = j[u] >= 0 ? row[j[u] >> 5] : 0u;
        u64 mine = 0;
#pragma unroll
        for (int u = 0; u < CROP_BITS_WORDS; ++u) {
            const u64 m = __ballot(j[u] >= 0 && ((half[u] >> (j[u] & 31)) & 1u));
            mine = lane == u ? m : mine;
        }
        if (store) bits_f[(int64_t)k * Wf + w0 + lane] = mine;
    }
}

constexpr int CROP_AREA_THREADS = 256;

__global__ __launch_bounds__(CROP_AREA_THREADS) void crop_area_kernel(const u64* __restrict__ bits_f, int64_t Wf, int* __restrict__ area) {
    __shared__ int s_cnt[CROP_AREA_THREADS / WAVE];
    const u64* __restrict__ row = bits_f + (int64_t)blockIdx.x * Wf;
    int c = 0;
    for (int64_t w = threadIdx.x; w < Wf; w += CROP_AREA_THREADS) c += __popcll(row[w]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < CROP_AREA_THREADS / WAVE; ++w) s += s_cnt[w];
        area[blockIdx.x] = s;
    }
}

PSAM_API int32_t psam_crop_expand_bits(const uint64_t* bits_w, const int64_t* inv, int32_t K, int32_t Nw, int32_t M, uint64_t* bits_f, int32_t* area_f,
                                       hipStream_t stream) {
    PSAM_REQUIRE(bits_w && inv && bits_f, PSAM_EINVAL, "psam_crop_expand_bits: null pointer");
    PSAM_REQUIRE(K > 0 && Nw > 0 && M > 0, PSAM_EINVAL, "psam_crop_expand_bits: need K > 0, Nw > 0, M > 0");
    const int64_t Ww = psam_cdiv(Nw, 64), Wf = psam_cdiv(M, 64);
    hipLaunchKernelGGL(crop_expand_bits_kernel, dim3((unsigned)psam_cdiv(Wf, CROP_BITS_BLOCK_WORDS)), dim3(CROP_BITS_THREADS), 0, stream, (const unsigned*)bits_w,
                       Ww, inv, (int)K, (int)Nw, (int)M, (u64*)bits_f, Wf);
    int32_t st = psam_launch_status("psam_crop_expand_bits: launch failed");
    if (st != PSAM_OK || !area_f) return st;
    hipLaunchKernelGGL(crop_area_kernel, dim3((unsigned)K), dim3(CROP_AREA_THREADS), 0, stream, (const u64*)bits_f, Wf, area_f);
    return psam_launch_status("psam_crop_expand_bits: area launch failed");
}
