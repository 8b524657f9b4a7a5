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
// The table, the scan and the launch sequence of the downsample are voxel_table.h's, with the members' block counts in the workspace and three
// result words (count, members, flag).  What is the crop's own:
//   insert   membership (q <= r2), normalised coordinate, cell, key in ONE pass over xyz; only members are inserted, so a voxel's representative is a
//            member.  state[i] = slot, CROP_NO_CELL (a member that is its own representative: inv_h == 0, or a cell out of range with the flag
//            raised) or VOXEL_OUTSIDE
//   look-up  VOXEL_OUTSIDE stays; per block the representatives and the members
//   offsets  besides the scan, the sum of the blocks' members -> members
//   rank     besides keep_idx[rank] = i: wxyz[rank] = u(i), wrgb[rank] = rgb[i].  The gather rides on the rank pass: the representative's own thread
//            holds i and rank, so no pass reads keep_idx back
// The two expands are scene_expand.h's kernels.
#include "common.h"
#include "crop_coord.h"      // CropBall, crop_member: shared with scene_interp.hip
#include "scene_expand.h"
#include "voxel_table.h"

#include <cmath>

constexpr int CROP_THREADS = 256;
constexpr int CROP_NO_CELL = -1;                  // a member without a slot: its own representative

// ------------------------------------------------------------------------------------------------ insert
__global__ __launch_bounds__(CROP_THREADS) void crop_insert_kernel(const float* __restrict__ xyz, int M, CropBall ball, float inv_h, u64* __restrict__ keys,
                                                                  unsigned* __restrict__ low, int capacity, int* __restrict__ state, int* __restrict__ flag) {
    const int i = blockIdx.x * CROP_THREADS + threadIdx.x;       // whole waves stay in the kernel: voxel_claim_run needs every lane
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
    int slot = voxel_claim_run(keys, low, capacity, key, i);
    if (key == VOXEL_EMPTY) slot = member ? CROP_NO_CELL : VOXEL_OUTSIDE;  // a run of empty keys mixes members without a cell and points off the ball
    if (i < M) state[i] = slot;
}

// ------------------------------------------------------------------------------------------------ look-up, offsets, rank
__global__ __launch_bounds__(SCAN_THREADS) void crop_lookup_kernel(int* __restrict__ state, const unsigned* __restrict__ low, int M,
                                                                  int* __restrict__ block_count, int* __restrict__ block_members) {
    __shared__ int s_own[SCAN_WAVES];
    __shared__ int s_mem[SCAN_WAVES];
    const int i = blockIdx.x * SCAN_THREADS + threadIdx.x;
    bool own = false, member = false;
    if (i < M) {
        const int slot = state[i];
        member = slot != VOXEL_OUTSIDE;
        if (member) {
            const int r = slot >= 0 ? (int)low[slot] : i;
            state[i] = r;
            own = r == i;
        }
    }
    scan_note(own, s_own);
    scan_note(member, s_mem);
    __syncthreads();
    if (threadIdx.x == 0) {
        block_count[blockIdx.x] = scan_total(s_own);
        block_members[blockIdx.x] = scan_total(s_mem);
    }
}

// the members' counts are only summed (out3[1]), over the spans of the scan; the representatives' counts become their exclusive scan (out3[0])
__global__ __launch_bounds__(SCAN_THREADS) void crop_offsets_kernel(int* __restrict__ block, const int* __restrict__ block_members, int blocks,
                                                                   int* __restrict__ out3) {
    __shared__ int s_mem[SCAN_WAVES];
    int lo, hi, c = 0, m = 0;
    scan_span(blocks, threadIdx.x, lo, hi);
    for (int b = lo; b < hi; ++b) { c += block[b]; m += block_members[b]; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m += __shfl_xor(m, d, 64);
    if ((threadIdx.x & 63) == 0) s_mem[threadIdx.x >> 6] = m;
    scan_block_offsets(block, blocks, lo, hi, c, out3);            // its barriers are s_mem's too
    if (threadIdx.x == 0) out3[1] = scan_total(s_mem);
}

__global__ __launch_bounds__(SCAN_THREADS) void crop_rank_kernel(int* __restrict__ state, int M, const int* __restrict__ block_offset,
                                                                const float* __restrict__ xyz, const float* __restrict__ rgb, CropBall ball,
                                                                int64_t* __restrict__ keep_idx, float* __restrict__ wxyz, float* __restrict__ wrgb) {
    __shared__ int s_cnt[SCAN_WAVES];
    const int i = blockIdx.x * SCAN_THREADS + threadIdx.x;
    const bool own = i < M && state[i] == i;
    const u64 m = scan_note(own, s_cnt);
    __syncthreads();
    if (!own) return;
    const int rank = scan_rank(m, s_cnt, block_offset[blockIdx.x]);
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

PSAM_API size_t psam_crop_downsample_workspace_bytes(int32_t M) {
    if (M <= 0 || M > VOXEL_MAX_POINTS) return 0;
    return voxel_layout(nullptr, M, true, true).bytes;
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
    const VoxelWs w = voxel_layout(ws, M, true, true);
    const int capacity = (int)voxel_capacity(M);
    const unsigned point_blocks = (unsigned)psam_cdiv(M, CROP_THREADS), blocks = (unsigned)scan_blocks(M);
    const CropBall ball = {center[0], center[1], center[2], r2, inv_r};
    int32_t st = voxel_clear<3>(w, result, stream, "psam_crop_downsample: clear launch failed");
    if (st != PSAM_OK) return st;
    hipLaunchKernelGGL(crop_insert_kernel, dim3(point_blocks), dim3(CROP_THREADS), 0, stream, xyz, (int)M, ball, inv_h, w.keys, w.low, capacity, w.rep,
                       result + 2);
    if ((st = psam_launch_status("psam_crop_downsample: insert launch failed")) != PSAM_OK) return st;
    hipLaunchKernelGGL(crop_lookup_kernel, dim3(blocks), dim3(SCAN_THREADS), 0, stream, w.rep, (const unsigned*)w.low, (int)M, w.block, w.block_members);
    if ((st = psam_launch_status("psam_crop_downsample: look-up launch failed")) != PSAM_OK) return st;
    hipLaunchKernelGGL(crop_offsets_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, w.block, (const int*)w.block_members, (int)blocks, result);
    if ((st = psam_launch_status("psam_crop_downsample: offsets launch failed")) != PSAM_OK) return st;
    if (!full) return PSAM_OK;
    hipLaunchKernelGGL(crop_rank_kernel, dim3(blocks), dim3(SCAN_THREADS), 0, stream, w.rep, (int)M, (const int*)w.block, xyz, rgb, ball, keep_idx, wxyz, wrgb);
    if ((st = psam_launch_status("psam_crop_downsample: rank launch failed")) != PSAM_OK) return st;
    hipLaunchKernelGGL((voxel_inverse_kernel<TABLE_THREADS, true>), dim3((unsigned)psam_cdiv(M, TABLE_THREADS)), dim3(TABLE_THREADS), 0, stream, (const int*)w.rep,
                       (int)M, inv);
    return psam_launch_status("psam_crop_downsample: inverse launch failed");
}

// ------------------------------------------------------------------------------------------------ expand
PSAM_API int32_t psam_crop_expand_rows(const void* src, int64_t src_ld, const int64_t* inv, int32_t R, int32_t Nw, int32_t M, uint32_t fill, void* dst,
                                       int64_t dst_ld, hipStream_t stream) {
    PSAM_REQUIRE(src && inv && dst, PSAM_EINVAL, "psam_crop_expand_rows: null pointer");
    PSAM_REQUIRE(R > 0 && Nw > 0 && M > 0 && src_ld >= Nw && dst_ld >= M, PSAM_EINVAL,
                 "psam_crop_expand_rows: need R > 0, Nw > 0, M > 0, src_ld >= Nw, dst_ld >= M");
    PSAM_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 3) == 0, PSAM_EALIGN, "psam_crop_expand_rows: src and dst must be 4-byte aligned");
    return expand_rows_launch(src, src_ld, inv, R, Nw, M, fill, dst, dst_ld, stream, "psam_crop_expand_rows: launch failed");
}

PSAM_API int32_t psam_crop_expand_bits(const uint64_t* bits_w, const int64_t* inv, int32_t K, int32_t Nw, int32_t M, uint64_t* bits_f, int32_t* area_f,
                                       hipStream_t stream) {
    PSAM_REQUIRE(bits_w && inv && bits_f, PSAM_EINVAL, "psam_crop_expand_bits: null pointer");
    PSAM_REQUIRE(K > 0 && Nw > 0 && M > 0, PSAM_EINVAL, "psam_crop_expand_bits: need K > 0, Nw > 0, M > 0");
    return expand_bits_launch<true>(bits_w, inv, K, Nw, M, bits_f, area_f, stream, "psam_crop_expand_bits: launch failed", "psam_crop_expand_bits: area launch failed");
}
