// Full-resolution scenes (point_sam_amd/scene.py): a scan of M points is reduced to a working cloud of one real point per occupied voxel, the model runs on
// the working cloud, and every point of the scan receives the result of its voxel's representative.  Everything here is integer work or a bit-for-bit
// copy, so every output is exact and reproducible:
//   psam_voxel_downsample    xyz [M, 3] -> keep_idx [count] (the lowest index of every occupied voxel, increasing) and inv [M] (position in keep_idx
//                            of each point's representative); with both NULL only the count
//   psam_scene_expand_rows   dst[r, i] = src[r, inv[i]] for rows of 32-bit words (fp32 logits, int32 labels)
//   psam_scene_expand_bits   bit i of full row k = bit inv[i] of working row k (the packed masks of csrc/masks.hip), and the full rows' popcounts
//
// The table, the scan and the launch sequence of the downsample are voxel_table.h's; the kernels here say how a scan point becomes a key (cell from
// origin and inv_h) and what the look-up and rank passes keep.  The two expands are scene_expand.h's kernels with a zero fill.
#include "common.h"
#include "scene_expand.h"
#include "voxel_table.h"     // which includes voxel_cell.h: cells, keys, the hash, the table's capacity

#include <cmath>

constexpr int VOXEL_THREADS = 256;

// ------------------------------------------------------------------------------------------------ insert
__global__ __launch_bounds__(VOXEL_THREADS) void voxel_insert_kernel(const float* __restrict__ xyz, int M, float ox, float oy, float oz, float inv_h,
                                                                    u64* __restrict__ keys, unsigned* __restrict__ low, int capacity,
                                                                    int* __restrict__ slot_of, int* __restrict__ flag) {
    const int i = blockIdx.x * VOXEL_THREADS + threadIdx.x;      // whole waves stay in the kernel: voxel_claim_run needs every lane
    u64 key = VOXEL_EMPTY;
    if (i < M) {
        u64 cx, cy, cz;
        const bool ok = voxel_axis(xyz[(int64_t)i * 3 + 0], ox, inv_h, cx) & voxel_axis(xyz[(int64_t)i * 3 + 1], oy, inv_h, cy) &
                        voxel_axis(xyz[(int64_t)i * 3 + 2], oz, inv_h, cz);
        if (ok) key = voxel_key(cx, cy, cz);
        else *flag = 1;                                            // every writer stores the same value
    }
    const int slot = voxel_claim_run(keys, low, capacity, key, i);
    if (i < M) slot_of[i] = slot;
}

// ------------------------------------------------------------------------------------------------ look-up, offsets, rank
// A point without a cell (flag raised: the caller discards the outputs) counts as its own representative, so every index stays in range.
__global__ __launch_bounds__(SCAN_THREADS) void voxel_lookup_kernel(int* __restrict__ rep, const unsigned* __restrict__ low, int M,
                                                                   int* __restrict__ block_count) {
    __shared__ int s_cnt[SCAN_WAVES];
    const int i = blockIdx.x * SCAN_THREADS + threadIdx.x;
    bool own = false;
    if (i < M) {
        const int slot = rep[i];
        const int r = slot >= 0 ? (int)low[slot] : i;
        rep[i] = r;
        own = r == i;
    }
    scan_note(own, s_cnt);
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = scan_total(s_cnt);
}

__global__ __launch_bounds__(SCAN_THREADS) void voxel_offsets_kernel(int* __restrict__ block, int blocks, int* __restrict__ count) {
    int lo, hi, c = 0;
    scan_span(blocks, threadIdx.x, lo, hi);
    for (int b = lo; b < hi; ++b) c += block[b];
    scan_block_offsets(block, blocks, lo, hi, c, count);
}

__global__ __launch_bounds__(SCAN_THREADS) void voxel_rank_kernel(int* __restrict__ rep, int M, const int* __restrict__ block_offset,
                                                                 int64_t* __restrict__ keep_idx) {
    __shared__ int s_cnt[SCAN_WAVES];
    const int i = blockIdx.x * SCAN_THREADS + threadIdx.x;
    const bool own = i < M && rep[i] == i;
    const u64 m = scan_note(own, s_cnt);
    __syncthreads();
    if (!own) return;
    const int rank = scan_rank(m, s_cnt, block_offset[blockIdx.x]);
    keep_idx[rank] = i;
    rep[i] = ~rank;                                                // read by the inverse kernel; only this thread touches rep[i] here
}

PSAM_API size_t psam_voxel_downsample_workspace_bytes(int32_t M) {
    if (M <= 0 || M > VOXEL_MAX_POINTS) return 0;
    return voxel_layout(nullptr, M, true, false).bytes;
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
    const VoxelWs w = voxel_layout(ws, M, true, false);
    const int capacity = (int)voxel_capacity(M);
    const unsigned point_blocks = (unsigned)psam_cdiv(M, VOXEL_THREADS), blocks = (unsigned)scan_blocks(M);
    int32_t st = voxel_clear<1>(w, flag, stream, "psam_voxel_downsample: clear launch failed");
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
    hipLaunchKernelGGL((voxel_inverse_kernel<TABLE_THREADS, false>), dim3((unsigned)psam_cdiv(M, TABLE_THREADS)), dim3(TABLE_THREADS), 0, stream, (const int*)w.rep,
                       (int)M, inv);
    return psam_launch_status("psam_voxel_downsample: inverse launch failed");
}

// ------------------------------------------------------------------------------------------------ expand
PSAM_API int32_t psam_scene_expand_rows(const void* src, int64_t src_ld, const int64_t* inv, int32_t R, int32_t Nw, int32_t M, void* dst, int64_t dst_ld,
                                        hipStream_t stream) {
    PSAM_REQUIRE(src && inv && dst, PSAM_EINVAL, "psam_scene_expand_rows: null pointer");
    PSAM_REQUIRE(R > 0 && Nw > 0 && M > 0 && src_ld >= Nw && dst_ld >= M, PSAM_EINVAL,
                 "psam_scene_expand_rows: need R > 0, Nw > 0, M > 0, src_ld >= Nw, dst_ld >= M");
    PSAM_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 3) == 0, PSAM_EALIGN, "psam_scene_expand_rows: src and dst must be 4-byte aligned");
    return expand_rows_launch(src, src_ld, inv, R, Nw, M, 0u, dst, dst_ld, stream, "psam_scene_expand_rows: launch failed");
}

PSAM_API int32_t psam_scene_expand_bits(const uint64_t* bits_w, const int64_t* inv, int32_t K, int32_t Nw, int32_t M, uint64_t* bits_f, int32_t* area_f,
                                        hipStream_t stream) {
    PSAM_REQUIRE(bits_w && inv && bits_f, PSAM_EINVAL, "psam_scene_expand_bits: null pointer");
    PSAM_REQUIRE(K > 0 && Nw > 0 && M > 0, PSAM_EINVAL, "psam_scene_expand_bits: need K > 0, Nw > 0, M > 0");
    return expand_bits_launch<false>(bits_w, inv, K, Nw, M, bits_f, area_f, stream, "psam_scene_expand_bits: launch failed", "psam_scene_expand_bits: area launch failed");
}
