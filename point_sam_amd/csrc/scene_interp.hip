// Interpolated scene masks (point_sam_amd/scene.py: build_interp_plan): instead of its voxel representative's logit (scene.hip, crops.hip) a scan point
// receives the inverse-distance blend of up to three working points, chosen among the representatives of its own voxel and of the 26 voxels around
// it.  The arithmetic is the model's own feature upsampling (the reference's common.py:238-274, psam_three_nn / psam_interp3), the candidate set is
// the grid's: 27 distance evaluations per scan point where a search over the working cloud would take Nw.
//   psam_interp_scene_plan   xyz [M, 3], inv [M], wxyz [Nw, 3], nbr [Nw, 26] -> idx3 [M, 3] int32, w3 [M, 3] f32; geometry only, once per scene or crop
//   psam_interp_scene_rows   dst[r, i] = the blend of src[r, idx3[i]] with w3[i], fp32 rows; a lone source is copied bit for bit
//   psam_interp_scene_bits   the packed masks `blend > thr` of psam_mask_pack's layout and their popcounts, without the [K, M] floats in between
//
// This is NOT a true 3-NN: a working point two cells away can be nearer than the third candidate.  The definition is the 27-cell one.  Measured on
// the CPU (uniform clouds and sphere surfaces, 2 - 130 points per voxel, 20 000 sampled scan points per case): the 27 representatives contain the true
// nearest working point for 100 % of the sampled points and the true three nearest for 99.9 %; the voxel's own representative is the nearest for
// only 51 - 72 %.
//
// Every operation is fp32 and rounded on its own (-ffp-contract=off, IEEE division), candidates are ordered by (q, rank), so every output is a
// function of the inputs alone: no atomics, no hand-over between threads, no data-dependent loops.
#include "common.h"
#include "crop_coord.h"      // the crop's normalised coordinate: the same bits as the crop cloud's own points
#include "interp_select.h"   // the ascending triple of (q, rank) and the weights: transfer.hip's too
#include "row_popcount.h"    // the area pass of the packed masks
#include "voxel_cell.h"      // VOXEL_MAX_POINTS, u64

#include <climits>
#include <cmath>

constexpr int INTERP_THREADS = 256;
constexpr int INTERP_NBR = 26;                    // words of a voxel's row of nbr: 104 bytes, thirteen 8-byte loads

// A candidate rank outside [0, Nw) (-1: no occupied voxel there) reads the point's own representative again and is entered as unused.
__device__ __forceinline__ void interp_candidate(InterpBest& b, const float* __restrict__ wxyz, int r, int own, int Nw, float px, float py, float pz) {
#pragma clang fp contract(off)
    const bool ok = (unsigned)r < (unsigned)Nw;
    const float* __restrict__ c = wxyz + (int64_t)(ok ? r : own) * 3;
    const float dx = px - c[0], dy = py - c[1], dz = pz - c[2];
    const float q = (dx * dx + dy * dy) + dz * dz;
    interp_insert(b, ok ? q : __builtin_inff(), ok ? r : INT_MAX);
}

template <bool CROP>
__global__ __launch_bounds__(INTERP_THREADS) void interp_plan_kernel(const float* __restrict__ xyz, int M, const int64_t* __restrict__ inv,
                                                                    const float* __restrict__ wxyz, const int* __restrict__ nbr, int Nw, CropBall ball,
                                                                    float eps, int* __restrict__ idx3, float* __restrict__ w3) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * INTERP_THREADS + threadIdx.x;
    if (i >= M) return;
    int* __restrict__ oi = idx3 + (int64_t)i * 3;
    float* __restrict__ ow = w3 + (int64_t)i * 3;
    const int64_t v64 = inv[i];
    if ((u64)v64 >= (u64)Nw) {                                     // off the crop's ball (-1), or an index no downsample produces
        oi[0] = -1; oi[1] = -1; oi[2] = -1;
        ow[0] = 0.0f; ow[1] = 0.0f; ow[2] = 0.0f;
        return;
    }
    const int v = (int)v64;
    float p[3];
    if (CROP) crop_member(xyz + (int64_t)i * 3, ball, p);
    else { p[0] = xyz[(int64_t)i * 3 + 0]; p[1] = xyz[(int64_t)i * 3 + 1]; p[2] = xyz[(int64_t)i * 3 + 2]; }
    const int2* __restrict__ row = (const int2*)(nbr + (int64_t)v * INTERP_NBR);      // 104 v bytes: 8-byte aligned for every v
    int2 n[INTERP_NBR / 2];
#pragma unroll
    for (int o = 0; o < INTERP_NBR / 2; ++o) n[o] = row[o];
    InterpBest b = interp_none();
    interp_candidate(b, wxyz, v, v, Nw, p[0], p[1], p[2]);
#pragma unroll
    for (int o = 0; o < INTERP_NBR / 2; ++o) {
        interp_candidate(b, wxyz, n[o].x, v, Nw, p[0], p[1], p[2]);
        interp_candidate(b, wxyz, n[o].y, v, Nw, p[0], p[1], p[2]);
    }
    interp_finish(b, eps, oi, ow);
}

PSAM_API int32_t psam_interp_scene_plan(const float* xyz, int32_t M, const int64_t* inv, const float* wxyz, const int32_t* nbr, int32_t Nw,
                                        const float* center, float inv_r, float eps, int32_t* idx3, float* w3, hipStream_t stream) {
    PSAM_REQUIRE(xyz && inv && wxyz && nbr && idx3 && w3, PSAM_EINVAL, "psam_interp_scene_plan: null pointer");
    PSAM_REQUIRE(M > 0 && M <= VOXEL_MAX_POINTS, PSAM_EINVAL, "psam_interp_scene_plan: need 0 < M <= 2^28");
    PSAM_REQUIRE(Nw > 0 && Nw <= VOXEL_MAX_POINTS, PSAM_EINVAL, "psam_interp_scene_plan: need 0 < Nw <= 2^28");
    PSAM_REQUIRE(std::isfinite(eps) && eps >= 0.0f, PSAM_EINVAL, "psam_interp_scene_plan: eps must be finite and not negative");
    PSAM_REQUIRE(((uintptr_t)nbr & 7) == 0, PSAM_EALIGN, "psam_interp_scene_plan: nbr must be 8-byte aligned");
    PSAM_REQUIRE((((uintptr_t)xyz | (uintptr_t)wxyz | (uintptr_t)idx3 | (uintptr_t)w3) & 3) == 0 && ((uintptr_t)inv & 7) == 0, PSAM_EALIGN,
                 "psam_interp_scene_plan: xyz, wxyz, idx3 and w3 must be 4-byte aligned, inv 8-byte aligned");
    const dim3 grid((unsigned)psam_cdiv(M, INTERP_THREADS)), block(INTERP_THREADS);
    if (center) {
        PSAM_REQUIRE(std::isfinite(center[0]) && std::isfinite(center[1]) && std::isfinite(center[2]), PSAM_EINVAL,
                     "psam_interp_scene_plan: center must be finite");
        PSAM_REQUIRE(std::isfinite(inv_r) && inv_r > 0.0f, PSAM_EINVAL, "psam_interp_scene_plan: inv_r must be finite and positive");
        const CropBall ball = {center[0], center[1], center[2], 0.0f, inv_r};
        hipLaunchKernelGGL(interp_plan_kernel<true>, grid, block, 0, stream, xyz, (int)M, inv, wxyz, (const int*)nbr, (int)Nw, ball, eps, (int*)idx3, w3);
    } else {
        const CropBall none = {0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
        hipLaunchKernelGGL(interp_plan_kernel<false>, grid, block, 0, stream, xyz, (int)M, inv, wxyz, (const int*)nbr, (int)Nw, none, eps, (int*)idx3, w3);
    }
    return psam_launch_status("psam_interp_scene_plan: launch failed");
}

// ------------------------------------------------------------------------------------------------ apply
// A point's three taps, read once for all rows.  An index outside [0, Nw) is unused and never dereferenced: its load is redirected to the tap before
// it (to column 0 for the first) and its value dropped.  Taps are used in order: without the first the point is off, without the second the first
// is copied, the third joins only a blend.
struct InterpTaps {
    int j0, j1, j2;
    float w0, w1, w2;
    bool ok0, ok1, ok2;
};

__device__ __forceinline__ InterpTaps interp_taps(const int* __restrict__ idx3, const float* __restrict__ w3, int64_t i, int Nw) {
    InterpTaps t;
    const int a = idx3[i * 3 + 0], b = idx3[i * 3 + 1], c = idx3[i * 3 + 2];
    t.w0 = w3[i * 3 + 0]; t.w1 = w3[i * 3 + 1]; t.w2 = w3[i * 3 + 2];
    t.ok0 = (unsigned)a < (unsigned)Nw;
    t.ok1 = t.ok0 && (unsigned)b < (unsigned)Nw;
    t.ok2 = t.ok1 && (unsigned)c < (unsigned)Nw;
    t.j0 = t.ok0 ? a : 0;
    t.j1 = t.ok1 ? b : t.j0;
    t.j2 = t.ok2 ? c : t.j0;
    return t;
}

// The output word of one row: the fill, the first source's word untouched (NaN payloads and infinities survive), or the blend's bits.
__device__ __forceinline__ unsigned interp_word(const unsigned* __restrict__ row, const InterpTaps& t, unsigned fill) {
#pragma clang fp contract(off)
    const unsigned u0 = row[t.j0], u1 = row[t.j1], u2 = row[t.j2];
    float acc = t.w0 * __builtin_bit_cast(float, u0) + t.w1 * __builtin_bit_cast(float, u1);
    const float third = acc + t.w2 * __builtin_bit_cast(float, u2);
    acc = t.ok2 ? third : acc;
    return !t.ok0 ? fill : !t.ok1 ? u0 : __builtin_bit_cast(unsigned, acc);
}

// One thread per scan point, rows four at a time: twelve gathered words in flight, then four coalesced stores.
__global__ __launch_bounds__(INTERP_THREADS) void interp_rows_kernel(const unsigned* __restrict__ src, int64_t src_ld, const int* __restrict__ idx3,
                                                                    const float* __restrict__ w3, int R, int Nw, int M, unsigned fill,
                                                                    unsigned* __restrict__ dst, int64_t dst_ld) {
    const int i = blockIdx.x * INTERP_THREADS + threadIdx.x;
    if (i >= M) return;
    const InterpTaps t = interp_taps(idx3, w3, i, Nw);
    int r = 0;
    for (; r + 4 <= R; r += 4) {
        unsigned v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = interp_word(src + (int64_t)(r + u) * src_ld, t, fill);
#pragma unroll
        for (int u = 0; u < 4; ++u) dst[(int64_t)(r + u) * dst_ld + i] = v[u];
    }
    for (; r < R; ++r) dst[(int64_t)r * dst_ld + i] = interp_word(src + (int64_t)r * src_ld, t, fill);
}

PSAM_API int32_t psam_interp_scene_rows(const float* src, int64_t src_ld, const int32_t* idx3, const float* w3, int32_t R, int32_t Nw, int32_t M,
                                        float fill, float* dst, int64_t dst_ld, hipStream_t stream) {
    PSAM_REQUIRE(src && idx3 && w3 && dst, PSAM_EINVAL, "psam_interp_scene_rows: null pointer");
    PSAM_REQUIRE(R > 0 && Nw > 0 && Nw <= VOXEL_MAX_POINTS && M > 0 && M <= VOXEL_MAX_POINTS && src_ld >= Nw && dst_ld >= M, PSAM_EINVAL,
                 "psam_interp_scene_rows: need R > 0, 0 < Nw <= 2^28, 0 < M <= 2^28, src_ld >= Nw, dst_ld >= M");
    PSAM_REQUIRE((((uintptr_t)src | (uintptr_t)dst | (uintptr_t)idx3 | (uintptr_t)w3) & 3) == 0, PSAM_EALIGN,
                 "psam_interp_scene_rows: src, dst, idx3 and w3 must be 4-byte aligned");
    hipLaunchKernelGGL(interp_rows_kernel, dim3((unsigned)psam_cdiv(M, INTERP_THREADS)), dim3(INTERP_THREADS), 0, stream, (const unsigned*)src, src_ld,
                       (const int*)idx3, w3, (int)R, (int)Nw, (int)M, __builtin_bit_cast(unsigned, fill), (unsigned*)dst, dst_ld);
    return psam_launch_status("psam_interp_scene_rows: launch failed");
}

// ------------------------------------------------------------------------------------------------ bits
// The scheme of scene_expand.h's expand: a wave owns INTERP_BITS_WORDS consecutive output words, every lane loads the taps of its points once, and for
// every row the ballot of `value > thr` IS the output word (NaN compares false; an off point and a point past M give a zero bit); lanes
// 0 .. INTERP_BITS_WORDS - 1 store the wave's words of the row as one contiguous segment.  The areas are a pass of their own over the finished rows.
constexpr int INTERP_BITS_WORDS = 4;
constexpr int INTERP_BITS_THREADS = 256;
constexpr int INTERP_BITS_BLOCK_WORDS = INTERP_BITS_WORDS * INTERP_BITS_THREADS / WAVE;

__global__ __launch_bounds__(INTERP_BITS_THREADS) void interp_bits_kernel(const unsigned* __restrict__ src, int64_t src_ld, const int* __restrict__ idx3,
                                                                         const float* __restrict__ w3, int K, int Nw, int M, float thr,
                                                                         u64* __restrict__ bits_f, int64_t Wf) {
    const int lane = threadIdx.x & 63;
    const int64_t w0 = ((int64_t)blockIdx.x * (INTERP_BITS_THREADS / WAVE) + (threadIdx.x >> 6)) * INTERP_BITS_WORDS;
    if (w0 >= Wf) return;                                          // wave-uniform
    InterpTaps t[INTERP_BITS_WORDS];
#pragma unroll
    for (int u = 0; u < INTERP_BITS_WORDS; ++u) {
        const int64_t i = (w0 + u) * 64 + lane;
        t[u] = interp_taps(idx3, w3, i < M ? i : (int64_t)M - 1, Nw);      // past M: a valid address, the point is switched off below
        t[u].ok0 = t[u].ok0 && i < M;
    }
    const bool store = lane < INTERP_BITS_WORDS && w0 + lane < Wf;
    for (int k = 0; k < K; ++k) {
        const unsigned* __restrict__ row = src + (int64_t)k * src_ld;
        float val[INTERP_BITS_WORDS];
#pragma unroll
        for (int u = 0; u < INTERP_BITS_WORDS; ++u) val[u] = __builtin_bit_cast(float, interp_word(row, t[u], 0u));
        u64 mine = 0;
#pragma unroll
        for (int u = 0; u < INTERP_BITS_WORDS; ++u) {
            const u64 m = __ballot(t[u].ok0 && val[u] > thr);
            mine = lane == u ? m : mine;
        }
        if (store) bits_f[(int64_t)k * Wf + w0 + lane] = mine;
    }
}

PSAM_API int32_t psam_interp_scene_bits(const float* src, int64_t src_ld, const int32_t* idx3, const float* w3, int32_t K, int32_t Nw, int32_t M,
                                        float thr, uint64_t* bits_f, int32_t* area_f, hipStream_t stream) {
    PSAM_REQUIRE(src && idx3 && w3 && bits_f, PSAM_EINVAL, "psam_interp_scene_bits: null pointer");
    PSAM_REQUIRE(K > 0 && Nw > 0 && Nw <= VOXEL_MAX_POINTS && M > 0 && M <= VOXEL_MAX_POINTS && src_ld >= Nw, PSAM_EINVAL,
                 "psam_interp_scene_bits: need K > 0, 0 < Nw <= 2^28, 0 < M <= 2^28, src_ld >= Nw");
    PSAM_REQUIRE((((uintptr_t)src | (uintptr_t)idx3 | (uintptr_t)w3) & 3) == 0 && ((uintptr_t)bits_f & 7) == 0, PSAM_EALIGN,
                 "psam_interp_scene_bits: src, idx3 and w3 must be 4-byte aligned, bits_f 8-byte aligned");
    const int64_t Wf = psam_cdiv(M, 64);
    hipLaunchKernelGGL(interp_bits_kernel, dim3((unsigned)psam_cdiv(Wf, INTERP_BITS_BLOCK_WORDS)), dim3(INTERP_BITS_THREADS), 0, stream, (const unsigned*)src,
                       src_ld, (const int*)idx3, w3, (int)K, (int)Nw, (int)M, thr, (u64*)bits_f, Wf);
    int32_t st = psam_launch_status("psam_interp_scene_bits: launch failed");
    if (st != PSAM_OK || !area_f) return st;
    hipLaunchKernelGGL(row_popcount_kernel<INTERP_BITS_THREADS>, dim3((unsigned)K), dim3(INTERP_BITS_THREADS), 0, stream, (const u64*)bits_f, Wf, area_f);
    return psam_launch_status("psam_interp_scene_bits: area launch failed");
}
