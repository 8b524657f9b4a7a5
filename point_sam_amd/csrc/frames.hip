// RGB-D frames (point_sam_amd/views.py: FrameSet): F depth images with colour and a camera each become one scan, and every frame a view of it whose
// keys point at each pixel's OWN point.
//   psam_frames_unproject  depth [F, H, W] + rgb [F, H, W, 3] + cameras [F, 18] -> world xyz [M, 3], rgb [M, 3], index [F, H, W], M: the kept pixels,
//                          compacted in ascending (f, y, x)
//   psam_frames_finish     xyz normalised in place, then keys [F, H, W] = (bits(depth in the normalised camera) << 32) | index: what psam_view_pick,
//                          the paints and psam_view_lift_bits take as the keys of a view
//
// Definition (include/pointsam_hip.h, "RGB-D frames"; tests/frames_reference.py follows it operation for operation).  Every fp32 operation is rounded
// on its own (-ffp-contract=off), division is IEEE.  No atomics: a kept pixel's place is (kept pixels in the blocks before) + (in the waves before,
// in its block) + (ballot bits below its lane), so every output bit is a function of the inputs alone.  The caller owns every buffer; no allocation,
// no host synchronisation.
//
// Launches of psam_frames_unproject, each a kernel boundary:
//   mark      a thread per pixel: the predicate (range, then the four neighbours of the edge filter); the wave's ballot word goes to the workspace,
//             the block's count to block[]
//   offsets   scan_block_offsets: exclusive scan of the block counts in place, the total behind the last block and in *count
//   emit      a thread per pixel reads its bit of the SAVED ballot word (the predicate, five loads and four compares, is evaluated once; the words
//             cost one bit per pixel each way), ranks itself and writes index, and for a kept pixel xyz and rgb
#include "common.h"
#include "rigid_pose.h"
#include "voxel_table.h"     // the ballot scan: scan_note / scan_total / scan_rank / scan_block_offsets, SCAN_THREADS; u64 (voxel_cell.h)

#include <cmath>

constexpr int FRAME_THREADS = 256;               // the two kernels of psam_frames_finish
constexpr int FRAME_MAX_SIDE = 8192;             // VIEW_MAX_SIDE of views.hip: a frame is a view
constexpr int64_t FRAME_MAX_PIXELS = 1 << 28;    // F * H * W, and so M: an index fits the low word of a key with room to spare
constexpr int FRAME_CAMERA_WORDS = 18;           // 12 pose words (world -> camera, row-major 3 x 4), fx, fy, cx, cy, near, far
constexpr u64 FRAME_EMPTY = ~0ull;

template <bool U16>
__device__ __forceinline__ float frame_depth(const void* __restrict__ depth, int p, float depth_scale) {
#pragma clang fp contract(off)
    if (U16) return (float)((const uint16_t*)depth)[p] * depth_scale;      // one rounded multiply
    return ((const float*)depth)[p];
}

// every compare is false for a NaN
__device__ __forceinline__ bool frame_in_range(float d, float znear, float zfar) { return d >= znear && d <= zfar && d < INFINITY; }

// p < total -> (f, y, x)
__device__ __forceinline__ void frame_pixel(int p, int W, int H, int& f, int& y, int& x) {
    const int hw = W * H;
    f = p / hw;
    const int r = p - f * hw;
    y = r / W;
    x = r - y * W;
}

// ------------------------------------------------------------------------------------------------ mark
// Blocks of SCAN_THREADS consecutive pixels; the workspace holds a ballot word for every wave of every block, also of the last one's tail.
template <bool U16>
__global__ __launch_bounds__(SCAN_THREADS) void frames_mark_kernel(const void* __restrict__ depth, float depth_scale, const float* __restrict__ cameras, int W,
                                                                  int H, int total, float edge, u64* __restrict__ ballots, int* __restrict__ block_count) {
#pragma clang fp contract(off)
    __shared__ int s_cnt[SCAN_WAVES];
    const int p = blockIdx.x * SCAN_THREADS + threadIdx.x;
    bool keep = false;
    if (p < total) {
        int f, y, x;
        frame_pixel(p, W, H, f, y, x);
        const float znear = cameras[(int64_t)f * FRAME_CAMERA_WORDS + 16], zfar = cameras[(int64_t)f * FRAME_CAMERA_WORDS + 17];
        const float d = frame_depth<U16>(depth, p, depth_scale);
        keep = frame_in_range(d, znear, zfar);
        if (keep && edge > 0.0f) {
            // a neighbour counts only inside the image (so inside this frame and this row / column) and in range; p - W >= 0 and p + W < total there
            const float limit = edge * d;
            bool jump = false;
            if (x > 0) { const float n = frame_depth<U16>(depth, p - 1, depth_scale); jump |= frame_in_range(n, znear, zfar) && fabsf(d - n) > limit; }
            if (x < W - 1) { const float n = frame_depth<U16>(depth, p + 1, depth_scale); jump |= frame_in_range(n, znear, zfar) && fabsf(d - n) > limit; }
            if (y > 0) { const float n = frame_depth<U16>(depth, p - W, depth_scale); jump |= frame_in_range(n, znear, zfar) && fabsf(d - n) > limit; }
            if (y < H - 1) { const float n = frame_depth<U16>(depth, p + W, depth_scale); jump |= frame_in_range(n, znear, zfar) && fabsf(d - n) > limit; }
            keep = !jump;
        }
    }
    const u64 m = scan_note(keep, s_cnt);
    if ((threadIdx.x & 63) == 0) ballots[p >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = scan_total(s_cnt);
}

__global__ __launch_bounds__(SCAN_THREADS) void frames_offsets_kernel(int* __restrict__ block, int blocks, int* __restrict__ count) {
    int lo, hi, c = 0;
    scan_span(blocks, threadIdx.x, lo, hi);
    for (int b = lo; b < hi; ++b) c += block[b];
    scan_block_offsets(block, blocks, lo, hi, c, count);
}

// ------------------------------------------------------------------------------------------------ emit
// The world point of pixel (x, y) at depth d: the camera-frame point, minus the translation, times the rotation's transpose.
__device__ __forceinline__ void frame_unproject(const float* __restrict__ cam, int x, int y, float d, float* __restrict__ out) {
#pragma clang fp contract(off)
    const float a = (((float)x + 0.5f) - cam[14]) / cam[12];
    const float b = (((float)y + 0.5f) - cam[15]) / cam[13];
    const float q0 = a * d - cam[3], q1 = b * d - cam[7], q2 = d - cam[11];
    out[0] = (cam[0] * q0 + cam[4] * q1) + cam[8] * q2;
    out[1] = (cam[1] * q0 + cam[5] * q1) + cam[9] * q2;
    out[2] = (cam[2] * q0 + cam[6] * q1) + cam[10] * q2;
}

template <bool U16, bool U8>
__global__ __launch_bounds__(SCAN_THREADS) void frames_emit_kernel(const void* __restrict__ depth, float depth_scale, const void* __restrict__ rgb,
                                                                  const float* __restrict__ cameras, int W, int H, int total,
                                                                  const u64* __restrict__ ballots, const int* __restrict__ block_offset,
                                                                  float* __restrict__ xyz, float* __restrict__ rgb_out, int* __restrict__ index) {
#pragma clang fp contract(off)
    __shared__ int s_cnt[SCAN_WAVES];
    const int p = blockIdx.x * SCAN_THREADS + threadIdx.x;
    const bool keep = (ballots[p >> 6] >> (threadIdx.x & 63)) & 1ull;      // one word per wave; bits of pixels past the end are 0
    const u64 m = scan_note(keep, s_cnt);
    int f, y, x;
    frame_pixel(min(p, total - 1), W, H, f, y, x);
    // A wave of 64 consecutive pixels nearly always lies in one frame: its camera is then addressed by a wave-uniform value and read once per
    // wave.  Decided while every lane is still here.
    const int f0 = __builtin_amdgcn_readfirstlane(f);
    const bool one_frame = __all(f == f0);
    __syncthreads();
    if (p >= total) return;
    if (!keep) { index[p] = -1; return; }
    const int rank = scan_rank(m, s_cnt, block_offset[blockIdx.x]);
    index[p] = rank;
    const float d = frame_depth<U16>(depth, p, depth_scale);
    float* __restrict__ out = xyz + (int64_t)rank * 3;
    if (one_frame) frame_unproject(cameras + (int64_t)f0 * FRAME_CAMERA_WORDS, x, y, d, out);
    else frame_unproject(cameras + (int64_t)f * FRAME_CAMERA_WORDS, x, y, d, out);
    float* __restrict__ col = rgb_out + (int64_t)rank * 3;
    if (U8) {
        const uint8_t* __restrict__ src = (const uint8_t*)rgb + (int64_t)p * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) col[c] = ((float)src[c] / 255.0f - 0.5f) / 0.5f;
    } else {
        const float* __restrict__ src = (const float*)rgb + (int64_t)p * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) col[c] = src[c];
    }
}

// ------------------------------------------------------------------------------------------------ finish
__global__ __launch_bounds__(FRAME_THREADS) void frames_normalise_kernel(float* __restrict__ xyz, int M, float mx, float my, float mz, float s) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * FRAME_THREADS + threadIdx.x;
    if (i >= M) return;
    float* __restrict__ q = xyz + (int64_t)i * 3;
    q[0] = (q[0] - mx) / s;
    q[1] = (q[1] - my) / s;
    q[2] = (q[2] - mz) / s;
}

__device__ __forceinline__ float frame_key_depth(const float* __restrict__ pose, float x, float y, float z) {
    RigidPose P;
#pragma unroll
    for (int a = 0; a < 12; ++a) P.m[a] = pose[a];
    float cx, cy, cz;
    pose_apply(P, x, y, z, cx, cy, cz);              // the arithmetic psam_view_lift_bits repeats for the same point; only cz is used
    return cz;
}

// One thread per pixel.  The pixel's point index is range-checked against M before a coordinate is read.
__global__ __launch_bounds__(FRAME_THREADS) void frames_keys_kernel(const float* __restrict__ xyz, int M, const int* __restrict__ index,
                                                                   const float* __restrict__ poses, int hw, int total, u64* __restrict__ keys) {
    const int p = blockIdx.x * FRAME_THREADS + threadIdx.x;
    const int f = min(p, total - 1) / hw;
    const int f0 = __builtin_amdgcn_readfirstlane(f);
    const bool one_frame = __all(f == f0);
    if (p >= total) return;
    const int i = index[p];
    u64 key = FRAME_EMPTY;
    if (i >= 0 && i < M) {
        const float* __restrict__ q = xyz + (int64_t)i * 3;
        const float z = one_frame ? frame_key_depth(poses + (int64_t)f0 * 12, q[0], q[1], q[2]) : frame_key_depth(poses + (int64_t)f * 12, q[0], q[1], q[2]);
        if (z > 0.0f && z < INFINITY) key = ((u64)__builtin_bit_cast(unsigned, z) << 32) | (u64)(unsigned)i;
    }
    keys[p] = key;
}

// ------------------------------------------------------------------------------------------------ host
struct FramesWs {
    u64* ballots;         // [blocks * SCAN_WAVES]
    int* block;           // [blocks + 1]: kept pixels per block, then their exclusive scan and the total
    size_t bytes;
};

static inline FramesWs frames_layout(void* ws, int64_t total) {
    FramesWs w = {};
    char* p = (char*)ws;
    size_t o = 0;
    w.ballots = (u64*)(p + o);     o += align16((size_t)scan_blocks(total) * SCAN_WAVES * sizeof(u64));
    w.block = (int*)(p + o);       o += align16(((size_t)scan_blocks(total) + 1) * sizeof(int));
    w.bytes = o;
    return w;
}

// 0 for a shape outside the limits
static inline int64_t frames_pixels(int32_t F, int32_t H, int32_t W) {
    if (F < 1 || H < 1 || H > FRAME_MAX_SIDE || W < 1 || W > FRAME_MAX_SIDE) return 0;
    const int64_t hw = (int64_t)H * W;
    return F <= FRAME_MAX_PIXELS / hw ? F * hw : 0;
}

PSAM_API size_t psam_frames_workspace_bytes(int32_t F, int32_t H, int32_t W) {
    const int64_t total = frames_pixels(F, H, W);
    return total ? frames_layout(nullptr, total).bytes : 0;
}

PSAM_API int32_t psam_frames_unproject(const void* depth, int32_t depth_u16, float depth_scale, const void* rgb, int32_t rgb_u8, const float* cameras,
                                       int32_t F, int32_t H, int32_t W, float edge, float* xyz, float* rgb_out, int32_t* index, int32_t* count,
                                       void* ws, size_t ws_bytes, hipStream_t stream) {
    PSAM_REQUIRE(depth && rgb && cameras && xyz && rgb_out && index && count && ws, PSAM_EINVAL, "psam_frames_unproject: null pointer");
    const int64_t total = frames_pixels(F, H, W);
    PSAM_REQUIRE(total > 0, PSAM_EINVAL, "psam_frames_unproject: need F >= 1, height and width in [1, 8192] and F * height * width <= 2^28");
    PSAM_REQUIRE((depth_u16 == 0 || depth_u16 == 1) && (rgb_u8 == 0 || rgb_u8 == 1), PSAM_EINVAL, "psam_frames_unproject: depth_u16 and rgb_u8 must be 0 or 1");
    PSAM_REQUIRE(!depth_u16 || (std::isfinite(depth_scale) && depth_scale > 0.0f), PSAM_EINVAL,
                 "psam_frames_unproject: depth_scale must be finite and positive for 16-bit depth");
    PSAM_REQUIRE(std::isfinite(edge) && edge >= 0.0f, PSAM_EINVAL, "psam_frames_unproject: edge must be finite and positive, or 0 for no edge filter");
    PSAM_REQUIRE(((uintptr_t)depth & (depth_u16 ? 1 : 3)) == 0 && ((uintptr_t)rgb & (rgb_u8 ? 0 : 3)) == 0 &&
                     (((uintptr_t)cameras | (uintptr_t)xyz | (uintptr_t)rgb_out | (uintptr_t)index | (uintptr_t)count) & 3) == 0 && ((uintptr_t)ws & 15) == 0,
                 PSAM_EALIGN, "psam_frames_unproject: the workspace must be 16-byte aligned, every other buffer aligned to its element");
    const FramesWs w = frames_layout(ws, total);
    PSAM_REQUIRE(ws_bytes >= w.bytes, PSAM_EWORKSPACE, "psam_frames_unproject: workspace too small (psam_frames_workspace_bytes)");
    const int blocks = (int)scan_blocks(total);
    const dim3 grid((unsigned)blocks), block(SCAN_THREADS);
    if (depth_u16) hipLaunchKernelGGL(frames_mark_kernel<true>, grid, block, 0, stream, depth, depth_scale, cameras, (int)W, (int)H, (int)total, edge, w.ballots, w.block);
    else hipLaunchKernelGGL(frames_mark_kernel<false>, grid, block, 0, stream, depth, depth_scale, cameras, (int)W, (int)H, (int)total, edge, w.ballots, w.block);
    int32_t st = psam_launch_status("psam_frames_unproject: mark launch failed");
    if (st != PSAM_OK) return st;
    hipLaunchKernelGGL(frames_offsets_kernel, dim3(1), block, 0, stream, w.block, blocks, (int*)count);
    if ((st = psam_launch_status("psam_frames_unproject: offsets launch failed")) != PSAM_OK) return st;
#define FRAMES_EMIT(U16, U8)                                                                                                                              \
    hipLaunchKernelGGL((frames_emit_kernel<U16, U8>), grid, block, 0, stream, depth, depth_scale, rgb, cameras, (int)W, (int)H, (int)total, (const u64*)w.ballots, \
                       (const int*)w.block, xyz, rgb_out, (int*)index)
    if (depth_u16 && rgb_u8) FRAMES_EMIT(true, true);
    else if (depth_u16) FRAMES_EMIT(true, false);
    else if (rgb_u8) FRAMES_EMIT(false, true);
    else FRAMES_EMIT(false, false);
#undef FRAMES_EMIT
    return psam_launch_status("psam_frames_unproject: emit launch failed");
}

PSAM_API int32_t psam_frames_finish(float* xyz, int32_t M, const int32_t* index, const float* poses, int32_t F, int32_t H, int32_t W, const float* center,
                                    float scale, uint64_t* keys, hipStream_t stream) {
    PSAM_REQUIRE(xyz && index && poses && center && keys, PSAM_EINVAL, "psam_frames_finish: null pointer");
    const int64_t total = frames_pixels(F, H, W);
    PSAM_REQUIRE(total > 0, PSAM_EINVAL, "psam_frames_finish: need F >= 1, height and width in [1, 8192] and F * height * width <= 2^28");
    PSAM_REQUIRE(M >= 1 && M <= total, PSAM_EINVAL, "psam_frames_finish: need 1 <= M <= F * height * width");
    PSAM_REQUIRE(std::isfinite(scale) && scale > 0.0f, PSAM_EINVAL, "psam_frames_finish: scale must be finite and positive");
    PSAM_REQUIRE(std::isfinite(center[0]) && std::isfinite(center[1]) && std::isfinite(center[2]), PSAM_EINVAL, "psam_frames_finish: center must be finite");
    PSAM_REQUIRE(((uintptr_t)keys & 7) == 0 && (((uintptr_t)xyz | (uintptr_t)index | (uintptr_t)poses) & 3) == 0, PSAM_EALIGN,
                 "psam_frames_finish: keys must be 8-byte aligned, xyz, index and poses 4-byte aligned");
    hipLaunchKernelGGL(frames_normalise_kernel, dim3((unsigned)psam_cdiv(M, FRAME_THREADS)), dim3(FRAME_THREADS), 0, stream, xyz, (int)M, center[0], center[1],
                       center[2], scale);
    const int32_t st = psam_launch_status("psam_frames_finish: normalise launch failed");
    if (st != PSAM_OK) return st;
    hipLaunchKernelGGL(frames_keys_kernel, dim3((unsigned)psam_cdiv(total, FRAME_THREADS)), dim3(FRAME_THREADS), 0, stream, (const float*)xyz, (int)M,
                       (const int*)index, poses, (int)(H * W), (int)total, (u64*)keys);
    return psam_launch_status("psam_frames_finish: keys launch failed");
}
