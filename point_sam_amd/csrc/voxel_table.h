// The voxel table and the scan behind it, shared by scene.hip (the working cloud), crops.hip (a ball's working cloud) and regions.hip (key -> rank
// of the neighbourhood graph): the table's format, its probe and the "lowest index wins" rule are one decision and live here once.
//
// Table.  Open addressing over C = voxel_capacity(n) = 2^ceil(log2(2 n)) slots (load factor <= 0.5): keys [C] u64, all ones = empty (no voxel key has
// bit 63), and one u32 per slot, the lowest index that arrived with the slot's key (all ones until one does).  The probe is linear from
// voxel_hash(key).  Which slot a key lands in depends on the arrival order of the waves; slot numbers never leave the workspace, and the lowest
// index of a slot does not depend on them.
//
// Downsample = table + scan.  The workspace adds one int32 per point (`rep`), one int32 per block of SCAN_THREADS points plus the total, and for a
// crop one more int32 per block (its member counts).  Launches, each a kernel boundary (no value is handed over inside a kernel); the caller's own
// kernels are marked *:
//   clear     keys and lowest indices = all ones, the caller's result words = 0
//   insert*   point -> key; voxel_claim_run: a slot is claimed by compare-and-swap on the key, the slot's lowest point index kept by an unsigned
//             atomic minimum; rep[i] = the slot.  A run of equal keys on consecutive lanes is one probe and one minimum (by the run's first lane,
//             whose index is the run's lowest).  A point without a key keeps a negative code of the caller's
//   look-up*  rep[i] = lowest index of slot rep[i]; per block the number of points that are their own representative (scan_note, scan_total)
//   offsets*  scan_block_offsets: exclusive scan of the block counts in place, the total behind the last block and in *count
//   rank*     scan_rank: rank of a representative = block offset + the waves before it + the ballot bits below its lane; rep[i] = ~rank
//   inverse   inv[i] = rank of rep[i], -1 for VOXEL_OUTSIDE
// Translation units that include this are compiled with -ffp-contract=off and without -fgpu-rdc: the two kernels here are templates so that they
// can live in a header, and a translation unit that launches one gets its own instance.
#pragma once
#include "voxel_cell.h"

#include <climits>

constexpr int SCAN_THREADS = 1024;                // points per block of the look-up and rank kernels, threads of the offsets kernel
constexpr int SCAN_WAVES = SCAN_THREADS / WAVE;
constexpr int TABLE_THREADS = 256;                // the clear and inverse kernels
constexpr int VOXEL_OUTSIDE = INT_MIN;            // rep[i] of a point that takes no part (off a crop's ball): never a slot, an index or a ~rank

static inline int64_t scan_blocks(int64_t M) { return psam_cdiv(M, SCAN_THREADS); }

// ------------------------------------------------------------------------------------------------ workspace
struct VoxelWs {
    u64* keys;            // [C]
    unsigned* low;        // [C]
    int* rep;             // [n]: slot or a negative code, then representative, then (representatives only) ~rank.  scan only
    int* block;           // [blocks + 1]: representatives per block, then their exclusive scan and the total.  scan only
    int* block_members;   // [blocks].  members only
    size_t table_bytes;   // keys and low: adjacent, a whole number of 16-byte granules
    size_t bytes;
};

// scan = false: the table alone (regions.hip)
static inline VoxelWs voxel_layout(void* ws, int64_t n, bool scan, bool members) {
    const int64_t C = voxel_capacity(n);
    VoxelWs w = {};
    char* p = (char*)ws;
    size_t o = 0;
    w.keys = (u64*)(p + o);            o += align16((size_t)C * sizeof(u64));
    w.low = (unsigned*)(p + o);        o += align16((size_t)C * sizeof(unsigned));
    w.table_bytes = o;
    if (scan) {
        w.rep = (int*)(p + o);         o += align16((size_t)n * sizeof(int));
        w.block = (int*)(p + o);       o += align16(((size_t)scan_blocks(n) + 1) * sizeof(int));
        if (members) { w.block_members = (int*)(p + o); o += align16((size_t)scan_blocks(n) * sizeof(int)); }
    }
    w.bytes = o;
    return w;
}

// ------------------------------------------------------------------------------------------------ clear
// one fill of all-ones words over keys and lowest indices; zero[0 .. ZERO_WORDS) = 0 (the caller's result words: ZERO_WORDS <= THREADS, may be 0)
template <int THREADS, int ZERO_WORDS>
__global__ __launch_bounds__(THREADS) void voxel_clear_kernel(uint4* __restrict__ table, int64_t granules, int* __restrict__ zero) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < granules; g += stride) table[g] = make_uint4(~0u, ~0u, ~0u, ~0u);
    if (ZERO_WORDS > 0 && blockIdx.x == 0 && threadIdx.x < ZERO_WORDS) zero[threadIdx.x] = 0;
}

template <int ZERO_WORDS>
static inline int32_t voxel_clear(const VoxelWs& w, int* zero, hipStream_t stream, const char* what) {
    const int64_t granules = (int64_t)(w.table_bytes / 16);
    hipLaunchKernelGGL((voxel_clear_kernel<TABLE_THREADS, ZERO_WORDS>), dim3((unsigned)(granules < 4096 * TABLE_THREADS ? psam_cdiv(granules, TABLE_THREADS) : 4096)),
                       dim3(TABLE_THREADS), 0, stream, (uint4*)w.keys, granules, zero);
    return psam_launch_status(what);
}

// ------------------------------------------------------------------------------------------------ probes
// The slot of `key`, claimed if the key is new.  At most n of the >= 2 n slots are ever taken, so an empty one always ends the walk (-1 otherwise).
__device__ __forceinline__ int voxel_claim(u64* __restrict__ keys, int capacity, u64 key) {
    const unsigned mask = (unsigned)capacity - 1u;
    unsigned pos = (unsigned)voxel_hash(key) & mask;
    for (int probe = 0; probe < capacity; ++probe) {
        u64 cur = __hip_atomic_load(&keys[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == VOXEL_EMPTY) cur = atomicCAS(&keys[pos], VOXEL_EMPTY, key);
        if (cur == VOXEL_EMPTY || cur == key) return (int)pos;
        pos = (pos + 1u) & mask;
    }
    return -1;
}

// The slot of `key` in a finished table (a kernel boundary after the last claim), -1 if it is not there.
__device__ __forceinline__ int voxel_find(const u64* __restrict__ keys, int capacity, u64 key) {
    const unsigned mask = (unsigned)capacity - 1u;
    unsigned pos = (unsigned)voxel_hash(key) & mask;
    for (int probe = 0; probe < capacity; ++probe) {
        const u64 cur = keys[pos];
        if (cur == VOXEL_EMPTY) break;
        if (cur == key) return (int)pos;
        pos = (pos + 1u) & mask;
    }
    return -1;
}

// Every lane of the wave calls this (inactive points with key = VOXEL_EMPTY).  A run of equal keys on consecutive lanes: its first lane claims
// the slot and takes the minimum of low[slot] with its index i for all of them.  -> the slot, -1 for VOXEL_EMPTY.
__device__ __forceinline__ int voxel_claim_run(u64* __restrict__ keys, unsigned* __restrict__ low, int capacity, u64 key, int i) {
    const int lane = threadIdx.x & 63;
    const u64 prev = __shfl_up(key, 1, 64);
    const bool leader = lane == 0 || prev != key;
    const u64 leaders = __ballot(leader);
    int slot = -1;
    if (leader && key != VOXEL_EMPTY) {
        slot = voxel_claim(keys, capacity, key);
        if (slot >= 0) atomicMin(&low[slot], (unsigned)i);
    }
    const int first = 63 - __clzll(leaders & (~0ull >> (63 - lane)));      // the run's first lane: the highest leader at or below this lane
    return __shfl(slot, first, 64);
}

// ------------------------------------------------------------------------------------------------ scan
// Blocks of SCAN_THREADS threads, every thread takes part.  scan_note: the wave's ballot of `pred`, its popcount to s_cnt[wave]; after a
// __syncthreads() scan_total gives the block's count and scan_rank the number of set threads before this one, from `offset` on.
__device__ __forceinline__ u64 scan_note(bool pred, int* s_cnt) {
    const u64 m = __ballot(pred);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(m);
    return m;
}

__device__ __forceinline__ int scan_total(const int* s_cnt) {
    int s = 0;
    for (int w = 0; w < SCAN_WAVES; ++w) s += s_cnt[w];
    return s;
}

__device__ __forceinline__ int scan_rank(u64 m, const int* s_cnt, int offset) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int rank = offset + __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) rank += s_cnt[w];
    return rank;
}

// The span of block counts thread `tid` of the one-workgroup second level owns.
__device__ __forceinline__ void scan_span(int blocks, int tid, int& lo, int& hi) {
    const int per = (blocks + SCAN_THREADS - 1) / SCAN_THREADS;
    lo = min(tid * per, blocks);
    hi = min(lo + per, blocks);
}

// Second level: one workgroup of SCAN_THREADS threads, a contiguous span [lo, hi) of block counts per thread (scan_span) whose sum c the caller
// has taken (with whatever else it reads per block); in place, the total lands behind the last block and in *count.  Two __syncthreads(): shared
// words the caller wrote before the call are visible after it.
__device__ __forceinline__ void scan_block_offsets(int* __restrict__ block, int blocks, int lo, int hi, int c, int* __restrict__ count) {
    __shared__ int s_sum[SCAN_THREADS];
    __shared__ int s_wave[SCAN_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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

// ------------------------------------------------------------------------------------------------ inverse
// OUTSIDE: rep may hold VOXEL_OUTSIDE (a crop); a scene stores none and skips the test
template <int THREADS, bool OUTSIDE>
__global__ __launch_bounds__(THREADS) void voxel_inverse_kernel(const int* __restrict__ rep, int M, int64_t* __restrict__ inv) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= M) return;
    int r = rep[i];
    if (OUTSIDE && r == VOXEL_OUTSIDE) { inv[i] = -1; return; }
    if (r >= 0) r = rep[r];                                        // a representative's entry is ~rank (negative, never VOXEL_OUTSIDE: ranks stay below 2^28)
    inv[i] = (int64_t)~r;
}
