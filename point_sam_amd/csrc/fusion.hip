// Multi-view label fusion (point_sam_amd/fusion.py): the 2-D segmentations of V views of one cloud become packed region rows for the host to link, and
// one vote per point over the linked labels.
//   psam_fuse_region_bits  labels [V, H, W] -> bits [R + V, ceil(N / 64)]: one row per (view, region) of the points visible with that label, and one
//                          row per view of the points visible at all; their popcounts
//   psam_fuse_vote         labels [V, H, W] (+ remap) -> per point the winner of at most 8 distinct global labels, its votes, and the counts of
//                          visible, labelled and dropped observations
//   psam_label_bits        labels [N] -> bits [K, ceil(N / 64)]: row k = the points labelled k
//
// Definition: include/pointsam_hip.h, "label fusion"; tests/fusion_reference.py follows it operation for operation.  An observation of point i in view
// v is view_camera.h's projection and visibility rule (view_lift_kernel's), the camera a row of a device table [V, 17]: 12 pose words, fx, fy, cx, cy,
// near.  Integers and bits only after the visibility test: every output is a function of the inputs alone, and there is no atomic anywhere.
//
// Every fp32 operation is rounded on its own (-ffp-contract=off).  The caller owns every buffer; no allocation, no host synchronisation.
#include "common.h"
#include "rigid_pose.h"
#include "row_popcount.h"    // the area pass of the rows
#include "view_camera.h"

#include <cmath>

constexpr int FUSE_THREADS = 256;
constexpr int FUSE_CAMERA_WORDS = 17;
constexpr int FUSE_MAX_VIEWS = 4096, FUSE_MAX_ROWS = 1 << 20;
constexpr int FUSE_SLOTS = 8;

// Row v of the camera table.  v is wave-uniform wherever this is called, so the seventeen loads are of a uniform address.
__device__ __forceinline__ ViewCamera fuse_camera(const float* __restrict__ cameras, int v, int W, int H) {
    const float* __restrict__ c = cameras + (int64_t)v * FUSE_CAMERA_WORDS;
    ViewCamera C;
#pragma unroll
    for (int a = 0; a < 12; ++a) C.P.m[a] = c[a];
    C.fx = c[12]; C.fy = c[13]; C.cx = c[14]; C.cy = c[15];
    C.width = (float)W; C.height = (float)H;
    C.znear = c[16];
    C.W = W; C.H = H;
    return C;
}

// The observation of a point in view v: whether it is visible, and the label at its centre pixel (undefined where it is not visible).
__device__ __forceinline__ bool fuse_observe(const ViewCamera& C, float x, float y, float z, const u64* __restrict__ keys, const int* __restrict__ labels,
                                             float tau, int& label) {
    int px, py;
    float depth;
    label = -1;
    if (!view_project(C, x, y, z, px, py, depth)) return false;
    const int64_t p = (int64_t)py * C.W + px;
    if (!view_visible(keys[p], depth, tau)) return false;
    label = labels[p];
    return true;
}

// The label's region row, -1 if the label is not one of the view's.  row_base [V + 1] is device memory that no entry point inspects: a row is used only
// if it lies in [0, R), whatever the table holds.
__device__ __forceinline__ int fuse_row(const int* __restrict__ row_base, int v, int R, int label) {
    const int base = row_base[v], count = row_base[v + 1] - base;
    const int64_t row = (int64_t)base + label;
    return label >= 0 && label < count && base >= 0 && row < R ? (int)row : -1;
}

// ------------------------------------------------------------------------------------------------ rows from labels
// The wave's 64 points carry a row each (-1: none).  Per distinct row in the wave: the ballot of the lanes that carry it is the wave's word of that row,
// and the first of those lanes stores it.  The word belongs to this wave alone (rows cleared beforehand, nobody else writes it): a plain store.
__device__ __forceinline__ void ballot_rows(int row, int lane, int64_t word, int64_t Wd, u64* __restrict__ bits) {
    bool pending = row >= 0;
    for (u64 left = __ballot(pending); left != 0; left = __ballot(pending)) {
        const int first = __builtin_ctzll(left);                                        // wave-uniform
        const int r = __builtin_amdgcn_readlane(row, __builtin_amdgcn_readfirstlane(first));
        const bool mine = pending && row == r;
        const u64 m = __ballot(mine);
        if (lane == first) bits[(int64_t)r * Wd + word] = m;
        pending = pending && !mine;
    }
}

__global__ __launch_bounds__(FUSE_THREADS) void fuse_clear_kernel(u64* __restrict__ bits, int64_t words) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += stride) bits[w] = 0;
}

// A wave owns the 64 consecutive points of one word, in one view (blockIdx.y).  The visible row R + v is written whole by this kernel.
__global__ __launch_bounds__(FUSE_THREADS) void fuse_region_kernel(const float* __restrict__ xyz, int N, const float* __restrict__ cameras, int W, int H,
                                                                  const u64* __restrict__ keys, const int* __restrict__ labels,
                                                                  const int* __restrict__ row_base, int R, float tau, u64* __restrict__ bits, int64_t Wd) {
    const int64_t word = (int64_t)blockIdx.x * (FUSE_THREADS / WAVE) + (threadIdx.x >> 6);
    if (word >= Wd) return;                                        // wave-uniform
    const int v = blockIdx.y, lane = threadIdx.x & 63;
    const int64_t i = word * 64 + lane, pixels = (int64_t)W * H;
    const ViewCamera C = fuse_camera(cameras, v, W, H);
    bool visible = false;
    int row = -1;
    if (i < N) {
        int label;
        visible = fuse_observe(C, xyz[i * 3 + 0], xyz[i * 3 + 1], xyz[i * 3 + 2], keys + v * pixels, labels + v * pixels, tau, label);
        if (visible) row = fuse_row(row_base, v, R, label);
    }
    const u64 seen = __ballot(visible);
    if (lane == 0) bits[((int64_t)R + v) * Wd + word] = seen;
    ballot_rows(row, lane, word, Wd, bits);
}

__global__ __launch_bounds__(FUSE_THREADS) void label_bits_kernel(const int* __restrict__ labels, int N, int K, u64* __restrict__ bits, int64_t Wd) {
    const int64_t word = (int64_t)blockIdx.x * (FUSE_THREADS / WAVE) + (threadIdx.x >> 6);
    if (word >= Wd) return;                                        // wave-uniform
    const int lane = threadIdx.x & 63;
    const int64_t i = word * 64 + lane;
    const int l = i < N ? labels[i] : -1;
    ballot_rows(l >= 0 && l < K ? l : -1, lane, word, Wd, bits);
}

// ------------------------------------------------------------------------------------------------ vote
// One thread per point; the loop over the views is wave-uniform.  The table of FUSE_SLOTS (label, count) pairs is indexed by unrolled loops only, so it
// stays in registers: `used` slots are filled in first-seen order, a label that finds the table full is counted in dropped.
__global__ __launch_bounds__(FUSE_THREADS) void fuse_vote_kernel(const float* __restrict__ xyz, int N, const float* __restrict__ cameras, int V, int W, int H,
                                                                const u64* __restrict__ keys, const int* __restrict__ labels,
                                                                const int* __restrict__ row_base, const int* __restrict__ remap, int R, float tau,
                                                                int min_votes, int* __restrict__ out_label, int* __restrict__ out_votes,
                                                                int* __restrict__ out_seen, int* __restrict__ out_labelled, int* __restrict__ out_dropped) {
    const int64_t i = (int64_t)blockIdx.x * FUSE_THREADS + threadIdx.x;
    if (i >= N) return;
    const float x = xyz[i * 3 + 0], y = xyz[i * 3 + 1], z = xyz[i * 3 + 2];
    const int64_t pixels = (int64_t)W * H;
    int lab[FUSE_SLOTS], cnt[FUSE_SLOTS];
#pragma unroll
    for (int s = 0; s < FUSE_SLOTS; ++s) { lab[s] = 0; cnt[s] = 0; }
    int used = 0, seen = 0, labelled = 0, dropped = 0;
    for (int v = 0; v < V; ++v) {
        const ViewCamera C = fuse_camera(cameras, v, W, H);
        int g;
        if (!fuse_observe(C, x, y, z, keys + v * pixels, labels + v * pixels, tau, g)) continue;
        ++seen;
        if (row_base) {
            const int row = fuse_row(row_base, v, R, g);
            if (row < 0) g = -1;
            else if (remap) g = remap[row];
        }
        if (g < 0) continue;                                       // visible but unlabelled
        ++labelled;
        bool found = false;
#pragma unroll
        for (int s = 0; s < FUSE_SLOTS; ++s) {
            const bool hit = s < used && lab[s] == g;
            cnt[s] += hit ? 1 : 0;
            found = found || hit;
        }
        if (found) continue;
        if (used == FUSE_SLOTS) { ++dropped; continue; }
#pragma unroll
        for (int s = 0; s < FUSE_SLOTS; ++s)
            if (s == used) { lab[s] = g; cnt[s] = 1; }
        ++used;
    }
    int best = -1, votes = 0;
#pragma unroll
    for (int s = 0; s < FUSE_SLOTS; ++s)
        if (s < used && (cnt[s] > votes || (cnt[s] == votes && lab[s] < best))) { best = lab[s]; votes = cnt[s]; }
    const bool won = votes >= min_votes;                           // min_votes >= 1: an empty table never wins
    out_label[i] = won ? best : -1;
    out_votes[i] = won ? votes : 0;
    out_seen[i] = seen;
    out_labelled[i] = labelled;
    out_dropped[i] = dropped;
}

// ------------------------------------------------------------------------------------------------ host
static inline bool fuse_views_ok(int32_t V, int32_t H, int32_t W) {
    return V >= 1 && V <= FUSE_MAX_VIEWS && W >= 1 && W <= VIEW_MAX_SIDE && H >= 1 && H <= VIEW_MAX_SIDE;
}

static inline unsigned fuse_clear_grid(int64_t words) { return (unsigned)(words < 4096 * (int64_t)FUSE_THREADS ? psam_cdiv(words, FUSE_THREADS) : 4096); }

PSAM_API int32_t psam_fuse_region_bits(const float* xyz, int32_t N, const float* cameras, int32_t V, int32_t H, int32_t W, const uint64_t* keys,
                                       const int32_t* labels, const int32_t* row_base, int32_t R, float tau, uint64_t* bits, int32_t* area,
                                       hipStream_t stream) {
    PSAM_REQUIRE(xyz && cameras && keys && labels && row_base && bits, PSAM_EINVAL, "psam_fuse_region_bits: null pointer");
    PSAM_REQUIRE(N > 0 && N <= VIEW_MAX_POINTS, PSAM_EINVAL, "psam_fuse_region_bits: need 0 < N <= 2^28");
    PSAM_REQUIRE(fuse_views_ok(V, H, W), PSAM_EINVAL, "psam_fuse_region_bits: need V in [1, 4096], width and height in [1, 8192]");
    PSAM_REQUIRE(R >= 0 && R <= FUSE_MAX_ROWS, PSAM_EINVAL, "psam_fuse_region_bits: need 0 <= R <= 2^20 region rows");
    PSAM_REQUIRE(tau >= 0.0f, PSAM_EINVAL, "psam_fuse_region_bits: tau must not be negative or NaN");
    PSAM_REQUIRE((((uintptr_t)keys | (uintptr_t)bits) & 7) == 0 &&
                 (((uintptr_t)xyz | (uintptr_t)cameras | (uintptr_t)labels | (uintptr_t)row_base | (uintptr_t)area) & 3) == 0, PSAM_EALIGN,
                 "psam_fuse_region_bits: keys and bits must be 8-byte aligned, xyz, cameras, labels, row_base and area 4-byte aligned");
    const int64_t Wd = psam_cdiv(N, 64);
    int32_t st;
    if (R > 0) {
        hipLaunchKernelGGL(fuse_clear_kernel, dim3(fuse_clear_grid(R * Wd)), dim3(FUSE_THREADS), 0, stream, (u64*)bits, R * Wd);
        if ((st = psam_launch_status("psam_fuse_region_bits: clear launch failed")) != PSAM_OK) return st;
    }
    hipLaunchKernelGGL(fuse_region_kernel, dim3((unsigned)psam_cdiv(Wd, FUSE_THREADS / WAVE), (unsigned)V), dim3(FUSE_THREADS), 0, stream, xyz, (int)N, cameras,
                       (int)W, (int)H, (const u64*)keys, (const int*)labels, (const int*)row_base, (int)R, tau, (u64*)bits, Wd);
    st = psam_launch_status("psam_fuse_region_bits: launch failed");
    if (st != PSAM_OK || !area) return st;
    hipLaunchKernelGGL(row_popcount_kernel<FUSE_THREADS>, dim3((unsigned)(R + V)), dim3(FUSE_THREADS), 0, stream, (const u64*)bits, Wd, (int*)area);
    return psam_launch_status("psam_fuse_region_bits: area launch failed");
}

PSAM_API int32_t psam_fuse_vote(const float* xyz, int32_t N, const float* cameras, int32_t V, int32_t H, int32_t W, const uint64_t* keys,
                                const int32_t* labels, const int32_t* row_base, const int32_t* remap, int32_t R, float tau, int32_t min_votes,
                                int32_t* label, int32_t* votes, int32_t* seen, int32_t* labelled, int32_t* dropped, hipStream_t stream) {
    PSAM_REQUIRE(xyz && cameras && keys && labels && label && votes && seen && labelled && dropped, PSAM_EINVAL, "psam_fuse_vote: null pointer");
    PSAM_REQUIRE(row_base || !remap, PSAM_EINVAL, "psam_fuse_vote: a remap needs the row_base that addresses it");
    PSAM_REQUIRE(N > 0 && N <= VIEW_MAX_POINTS, PSAM_EINVAL, "psam_fuse_vote: need 0 < N <= 2^28");
    PSAM_REQUIRE(fuse_views_ok(V, H, W), PSAM_EINVAL, "psam_fuse_vote: need V in [1, 4096], width and height in [1, 8192]");
    PSAM_REQUIRE(R >= 0 && R <= FUSE_MAX_ROWS, PSAM_EINVAL, "psam_fuse_vote: need 0 <= R <= 2^20 region rows");
    PSAM_REQUIRE(tau >= 0.0f, PSAM_EINVAL, "psam_fuse_vote: tau must not be negative or NaN");
    PSAM_REQUIRE(min_votes >= 1, PSAM_EINVAL, "psam_fuse_vote: min_votes must be at least 1");
    PSAM_REQUIRE(((uintptr_t)keys & 7) == 0 &&
                 (((uintptr_t)xyz | (uintptr_t)cameras | (uintptr_t)labels | (uintptr_t)row_base | (uintptr_t)remap | (uintptr_t)label | (uintptr_t)votes |
                   (uintptr_t)seen | (uintptr_t)labelled | (uintptr_t)dropped) & 3) == 0, PSAM_EALIGN,
                 "psam_fuse_vote: keys must be 8-byte aligned, every other pointer 4-byte aligned");
    hipLaunchKernelGGL(fuse_vote_kernel, dim3((unsigned)psam_cdiv(N, FUSE_THREADS)), dim3(FUSE_THREADS), 0, stream, xyz, (int)N, cameras, (int)V, (int)W, (int)H,
                       (const u64*)keys, (const int*)labels, (const int*)row_base, (const int*)remap, (int)R, tau, (int)min_votes, (int*)label, (int*)votes,
                       (int*)seen, (int*)labelled, (int*)dropped);
    return psam_launch_status("psam_fuse_vote: launch failed");
}

PSAM_API int32_t psam_label_bits(const int32_t* labels, int32_t N, int32_t K, uint64_t* bits, int32_t* area, hipStream_t stream) {
    PSAM_REQUIRE(labels && bits, PSAM_EINVAL, "psam_label_bits: null pointer");
    PSAM_REQUIRE(N > 0 && N <= VIEW_MAX_POINTS, PSAM_EINVAL, "psam_label_bits: need 0 < N <= 2^28");
    PSAM_REQUIRE(K >= 1 && K <= FUSE_MAX_ROWS, PSAM_EINVAL, "psam_label_bits: need 1 <= K <= 2^20 rows");
    PSAM_REQUIRE(((uintptr_t)bits & 7) == 0 && (((uintptr_t)labels | (uintptr_t)area) & 3) == 0, PSAM_EALIGN,
                 "psam_label_bits: bits must be 8-byte aligned, labels and area 4-byte aligned");
    const int64_t Wd = psam_cdiv(N, 64);
    hipLaunchKernelGGL(fuse_clear_kernel, dim3(fuse_clear_grid(K * Wd)), dim3(FUSE_THREADS), 0, stream, (u64*)bits, K * Wd);
    int32_t st = psam_launch_status("psam_label_bits: clear launch failed");
    if (st != PSAM_OK) return st;
    hipLaunchKernelGGL(label_bits_kernel, dim3((unsigned)psam_cdiv(Wd, FUSE_THREADS / WAVE)), dim3(FUSE_THREADS), 0, stream, (const int*)labels, (int)N, (int)K,
                       (u64*)bits, Wd);
    st = psam_launch_status("psam_label_bits: launch failed");
    if (st != PSAM_OK || !area) return st;
    hipLaunchKernelGGL(row_popcount_kernel<FUSE_THREADS>, dim3((unsigned)K), dim3(FUSE_THREADS), 0, stream, (const u64*)bits, Wd, (int*)area);
    return psam_launch_status("psam_label_bits: area launch failed");
}
