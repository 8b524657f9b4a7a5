// Camera views of a cloud (point_sam_amd/views.py): the scan is drawn into a z-buffer of point splats, and the picture is the bridge between pixels
// and points -- which point is under a click, what a packed mask looks like in the image, which points an image mask covers.
//   psam_view_splat        xyz [N, 3] + camera -> keys [H, W]: per pixel the minimum (depth, index) key offered to it, all ones where none was
//   psam_view_pick         clicks [P, 2] -> the point index under each, searched in a window around the pixel
//   psam_view_paint_ids    packed masks [K, Wd] -> ids [H, W]: the lowest row that holds the pixel's point
//   psam_view_paint_rows   packed masks [K, Wd] -> rows [K, H, W] uint8: that row's bit of the pixel's point
//   psam_view_lift_bits    image masks [K, H, W] -> packed masks [K, ceil(N / 64)] of the points VISIBLE in the view, and their popcounts
//
// Definition (include/pointsam_hip.h, "camera views"; tests/view_reference.py follows it operation for operation).  Point i = (x, y, z):
//     c_a = ((P[a][0] x + P[a][1] y) + P[a][2] z) + P[a][3]                  rigid_pose.h
//     u = fx (c_x / c_z) + cx,  v = fy (c_y / c_z) + cy                      IEEE division
//     in view iff c_z >= near, c_z finite, 0 <= u < width, 0 <= v < height   fp32 compares BEFORE any conversion; a NaN is false everywhere
//     pixel (floorf(u), floorf(v));  key_i = (bits(c_z) << 32) | i           c_z > 0: the bit order is the value order
// A point offers its key to the (2 s + 1)^2 pixels around its own that lie inside the image; a pixel keeps the minimum.  The minimum of a set does not
// depend on the order its members arrive in, and no two points share a key (the index is part of it): the picture is a function of (points, camera, s)
// alone, ties in depth go to the lower index.
//
// Every fp32 operation is rounded on its own (-ffp-contract=off).  The caller owns every buffer; no allocation, no host synchronisation.
#include "common.h"
#include "rigid_pose.h"
#include "row_popcount.h"    // the area pass of the lifted masks; u64 (voxel_cell.h)
#include "view_camera.h"     // ViewCamera, view_project, view_visible: shared with fusion.hip

#include <climits>
#include <cmath>
#include <cstdio>

constexpr int VIEW_THREADS = 256;
constexpr int VIEW_MAX_SPLAT = 3, VIEW_MAX_WINDOW = 16;

// ------------------------------------------------------------------------------------------------ clear
__global__ __launch_bounds__(VIEW_THREADS) void view_clear_kernel(u64* __restrict__ keys, int64_t pixels) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pixels; p += stride) keys[p] = VIEW_EMPTY;
}

// ------------------------------------------------------------------------------------------------ splat
// One thread per point, at most (2 s + 1)^2 <= 49 pixels each.  A plain load of the pixel comes first and the atomic is skipped when the stored key is
// already <= ours.  The load may be stale (another CU's L1, an older L2 line) and that is safe: a pixel's key only ever DECREASES, so a stale value is
// larger than or equal to the truth.  A stale value can therefore only make us issue an atomic that loses -- never skip one that would have won.  The
// skip matters because an atomic drops its line from the XCD's L2 while a load keeps it there: in a dense picture most offers lose.
template <int S>
__global__ __launch_bounds__(VIEW_THREADS) void view_splat_kernel(const float* __restrict__ xyz, int N, ViewCamera C, u64* keys) {
    const int i = blockIdx.x * VIEW_THREADS + threadIdx.x;
    if (i >= N) return;
    int px, py;
    float depth;
    if (!view_project(C, xyz[(int64_t)i * 3 + 0], xyz[(int64_t)i * 3 + 1], xyz[(int64_t)i * 3 + 2], px, py, depth)) return;
    const u64 key = ((u64)__builtin_bit_cast(unsigned, depth) << 32) | (u64)(unsigned)i;
#pragma unroll
    for (int dy = -S; dy <= S; ++dy) {
        const int qy = py + dy;
        if (qy < 0 || qy >= C.H) continue;
#pragma unroll
        for (int dx = -S; dx <= S; ++dx) {
            const int qx = px + dx;
            if (qx < 0 || qx >= C.W) continue;
            u64* slot = keys + ((int64_t)qy * C.W + qx);
            if (key < *slot) atomicMin((unsigned long long*)slot, (unsigned long long)key);
        }
    }
}

// ------------------------------------------------------------------------------------------------ pick
// One thread per click: the non-empty pixel of the window with the smallest (dx^2 + dy^2, key).  At most (2 w + 1)^2 <= 1089 loads.
__global__ __launch_bounds__(VIEW_THREADS) void view_pick_kernel(const u64* __restrict__ keys, int W, int H, const int* __restrict__ pixels, int P, int w,
                                                                int* __restrict__ out) {
    const int c = blockIdx.x * VIEW_THREADS + threadIdx.x;
    if (c >= P) return;
    const int64_t qx = pixels[(int64_t)c * 2 + 0], qy = pixels[(int64_t)c * 2 + 1];
    int best_d = INT_MAX;
    u64 best = VIEW_EMPTY;
    for (int dy = -w; dy <= w; ++dy) {
        const int64_t y = qy + dy;
        if (y < 0 || y >= H) continue;
        for (int dx = -w; dx <= w; ++dx) {
            const int64_t x = qx + dx;
            if (x < 0 || x >= W) continue;
            const u64 k = keys[y * W + x];
            const int d = dx * dx + dy * dy;
            if (k != VIEW_EMPTY && (d < best_d || (d == best_d && k < best))) { best_d = d; best = k; }
        }
    }
    out[c] = best == VIEW_EMPTY ? -1 : (int)(unsigned)best;
}

// ------------------------------------------------------------------------------------------------ paint
// One thread per pixel.  The pixel's point index is range-checked against N before a bit word is read: keys of another cloud end as a wrong answer.
template <bool ROWS>
__global__ __launch_bounds__(VIEW_THREADS) void view_paint_kernel(const u64* __restrict__ keys, int64_t pixels, const u64* __restrict__ bits, int K, int N,
                                                                 int64_t Wd, int* __restrict__ ids, uint8_t* __restrict__ rows) {
    const int64_t p = (int64_t)blockIdx.x * VIEW_THREADS + threadIdx.x;
    if (p >= pixels) return;
    const u64 key = keys[p];
    const unsigned idx = (unsigned)key;
    const bool ok = key != VIEW_EMPTY && idx < (unsigned)N;
    const u64* __restrict__ word = bits + (idx >> 6);
    const int sh = (int)(idx & 63u);
    if (ROWS) {
        for (int k = 0; k < K; ++k) rows[(int64_t)k * pixels + p] = ok ? (uint8_t)((word[(int64_t)k * Wd] >> sh) & 1ull) : (uint8_t)0;
    } else {
        int id = -1;
        if (ok)
            for (int k = 0; k < K; ++k)
                if ((word[(int64_t)k * Wd] >> sh) & 1ull) { id = k; break; }
        ids[p] = id;
    }
}

// ------------------------------------------------------------------------------------------------ lift
// A wave owns the 64 consecutive points of one output word (whole waves stay in the kernel): the ballot of the predicate IS the word, the layout of
// psam_scene_expand_bits.  The projection and the visibility test run once per point, the K images are read at the point's centre pixel.
__global__ __launch_bounds__(VIEW_THREADS) void view_lift_kernel(const float* __restrict__ xyz, int N, ViewCamera C, const u64* __restrict__ keys, float tau,
                                                                const uint8_t* __restrict__ img, int K, u64* __restrict__ bits, int64_t Wd) {
#pragma clang fp contract(off)
    const int64_t word = (int64_t)blockIdx.x * (VIEW_THREADS / WAVE) + (threadIdx.x >> 6);
    if (word >= Wd) return;                                        // wave-uniform
    const int lane = threadIdx.x & 63;
    const int64_t i = word * 64 + lane;
    bool visible = false;
    int64_t p = 0;
    if (i < N) {
        int px, py;
        float depth;
        if (view_project(C, xyz[i * 3 + 0], xyz[i * 3 + 1], xyz[i * 3 + 2], px, py, depth)) {
            p = (int64_t)py * C.W + px;
            visible = view_visible(keys[p], depth, tau);
        }
    }
    const int64_t pixels = (int64_t)C.W * C.H;
    for (int k = 0; k < K; ++k) {
        const bool on = visible && (img == nullptr || img[(int64_t)k * pixels + p] != 0);
        const u64 m = __ballot(on);
        if (lane == 0) bits[(int64_t)k * Wd + word] = m;
    }
}

// ------------------------------------------------------------------------------------------------ host
// A refusal whose message names the entry point: the checks the entry points share are written once.
static inline int32_t view_refuse(const char* who, const char* what, int32_t code) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    psam_set_error(msg);                                           // copies
    return code;
}
#define VIEW_REQUIRE(cond, code, what)                          \
    do {                                                        \
        if (!(cond)) return view_refuse(who, (what), (code));   \
    } while (0)

static inline int32_t view_camera(const char* who, const float* pose, float fx, float fy, float cx, float cy, int32_t width, int32_t height, float znear,
                                  ViewCamera& C) {
    VIEW_REQUIRE(pose, PSAM_EINVAL, "null pointer");
    VIEW_REQUIRE(width >= 1 && width <= VIEW_MAX_SIDE && height >= 1 && height <= VIEW_MAX_SIDE, PSAM_EINVAL, "width and height must lie in [1, 8192]");
    VIEW_REQUIRE(std::isfinite(fx) && fx > 0.0f && std::isfinite(fy) && fy > 0.0f, PSAM_EINVAL, "fx and fy must be finite and positive");
    VIEW_REQUIRE(std::isfinite(cx) && std::isfinite(cy), PSAM_EINVAL, "cx and cy must be finite");
    VIEW_REQUIRE(std::isfinite(znear) && znear > 0.0f, PSAM_EINVAL, "near must be finite and positive");
    VIEW_REQUIRE(pose_load(pose, C.P), PSAM_EINVAL, "pose must be finite");
    C.fx = fx; C.fy = fy; C.cx = cx; C.cy = cy;
    C.width = (float)width; C.height = (float)height;
    C.znear = znear;
    C.W = width; C.H = height;
    return PSAM_OK;
}

static inline bool view_image_ok(int32_t width, int32_t height) {
    return width >= 1 && width <= VIEW_MAX_SIDE && height >= 1 && height <= VIEW_MAX_SIDE;
}

PSAM_API int32_t psam_view_splat(const float* xyz, int32_t N, const float* pose, float fx, float fy, float cx, float cy, int32_t width, int32_t height,
                                 float znear, int32_t s, uint64_t* keys, hipStream_t stream) {
    PSAM_REQUIRE(xyz && pose && keys, PSAM_EINVAL, "psam_view_splat: null pointer");
    PSAM_REQUIRE(N > 0 && N <= VIEW_MAX_POINTS, PSAM_EINVAL, "psam_view_splat: need 0 < N <= 2^28");
    PSAM_REQUIRE(s >= 0 && s <= VIEW_MAX_SPLAT, PSAM_EINVAL, "psam_view_splat: the footprint s must lie in 0 .. 3");
    ViewCamera C = {};
    int32_t st = view_camera("psam_view_splat", pose, fx, fy, cx, cy, width, height, znear, C);
    if (st != PSAM_OK) return st;
    PSAM_REQUIRE(((uintptr_t)keys & 7) == 0 && ((uintptr_t)xyz & 3) == 0, PSAM_EALIGN, "psam_view_splat: keys must be 8-byte aligned, xyz 4-byte aligned");
    const int64_t pixels = (int64_t)width * height;
    hipLaunchKernelGGL(view_clear_kernel, dim3((unsigned)(pixels < 4096 * (int64_t)VIEW_THREADS ? psam_cdiv(pixels, VIEW_THREADS) : 4096)), dim3(VIEW_THREADS), 0,
                       stream, (u64*)keys, pixels);
    if ((st = psam_launch_status("psam_view_splat: clear launch failed")) != PSAM_OK) return st;
    const dim3 grid((unsigned)psam_cdiv(N, VIEW_THREADS)), block(VIEW_THREADS);
    switch (s) {
        case 0: hipLaunchKernelGGL(view_splat_kernel<0>, grid, block, 0, stream, xyz, (int)N, C, (u64*)keys); break;
        case 1: hipLaunchKernelGGL(view_splat_kernel<1>, grid, block, 0, stream, xyz, (int)N, C, (u64*)keys); break;
        case 2: hipLaunchKernelGGL(view_splat_kernel<2>, grid, block, 0, stream, xyz, (int)N, C, (u64*)keys); break;
        default: hipLaunchKernelGGL(view_splat_kernel<3>, grid, block, 0, stream, xyz, (int)N, C, (u64*)keys); break;
    }
    return psam_launch_status("psam_view_splat: launch failed");
}

PSAM_API int32_t psam_view_pick(const uint64_t* keys, int32_t width, int32_t height, const int32_t* pixels, int32_t P, int32_t w, int32_t* point_index,
                                hipStream_t stream) {
    PSAM_REQUIRE(keys && pixels && point_index, PSAM_EINVAL, "psam_view_pick: null pointer");
    PSAM_REQUIRE(view_image_ok(width, height), PSAM_EINVAL, "psam_view_pick: width and height must lie in [1, 8192]");
    PSAM_REQUIRE(P > 0 && P <= VIEW_MAX_POINTS, PSAM_EINVAL, "psam_view_pick: need 0 < P <= 2^28 clicks");
    PSAM_REQUIRE(w >= 0 && w <= VIEW_MAX_WINDOW, PSAM_EINVAL, "psam_view_pick: the window w must lie in 0 .. 16");
    PSAM_REQUIRE(((uintptr_t)keys & 7) == 0 && (((uintptr_t)pixels | (uintptr_t)point_index) & 3) == 0, PSAM_EALIGN,
                 "psam_view_pick: keys must be 8-byte aligned, pixels and point_index 4-byte aligned");
    hipLaunchKernelGGL(view_pick_kernel, dim3((unsigned)psam_cdiv(P, VIEW_THREADS)), dim3(VIEW_THREADS), 0, stream, (const u64*)keys, (int)width, (int)height,
                       (const int*)pixels, (int)P, (int)w, (int*)point_index);
    return psam_launch_status("psam_view_pick: launch failed");
}

// ids or rows, the other NULL
static inline int32_t view_paint(const char* who, const uint64_t* keys, int32_t width, int32_t height, const uint64_t* bits, int32_t K, int32_t N, int32_t* ids,
                                 uint8_t* rows, hipStream_t stream) {
    VIEW_REQUIRE(keys && bits && (ids || rows), PSAM_EINVAL, "null pointer");
    VIEW_REQUIRE(view_image_ok(width, height), PSAM_EINVAL, "width and height must lie in [1, 8192]");
    VIEW_REQUIRE(K > 0 && N > 0 && N <= VIEW_MAX_POINTS, PSAM_EINVAL, "need K > 0 and 0 < N <= 2^28");
    VIEW_REQUIRE((((uintptr_t)keys | (uintptr_t)bits) & 7) == 0 && ((uintptr_t)ids & 3) == 0, PSAM_EALIGN, "keys and bits must be 8-byte aligned, ids 4-byte aligned");
    const int64_t pixels = (int64_t)width * height;
    const dim3 grid((unsigned)psam_cdiv(pixels, VIEW_THREADS)), block(VIEW_THREADS);
    if (rows) hipLaunchKernelGGL(view_paint_kernel<true>, grid, block, 0, stream, (const u64*)keys, pixels, (const u64*)bits, (int)K, (int)N, psam_cdiv(N, 64), ids, rows);
    else hipLaunchKernelGGL(view_paint_kernel<false>, grid, block, 0, stream, (const u64*)keys, pixels, (const u64*)bits, (int)K, (int)N, psam_cdiv(N, 64), ids, rows);
    return psam_launch_status(rows ? "psam_view_paint_rows: launch failed" : "psam_view_paint_ids: launch failed");
}

PSAM_API int32_t psam_view_paint_ids(const uint64_t* keys, int32_t width, int32_t height, const uint64_t* bits, int32_t K, int32_t N, int32_t* ids,
                                     hipStream_t stream) {
    return view_paint("psam_view_paint_ids", keys, width, height, bits, K, N, ids, nullptr, stream);
}

PSAM_API int32_t psam_view_paint_rows(const uint64_t* keys, int32_t width, int32_t height, const uint64_t* bits, int32_t K, int32_t N, uint8_t* rows,
                                      hipStream_t stream) {
    return view_paint("psam_view_paint_rows", keys, width, height, bits, K, N, nullptr, rows, stream);
}

PSAM_API int32_t psam_view_lift_bits(const float* xyz, int32_t N, const float* pose, float fx, float fy, float cx, float cy, int32_t width, int32_t height,
                                     float znear, const uint64_t* keys, const uint8_t* img, int32_t K, float tau, uint64_t* bits, int32_t* area,
                                     hipStream_t stream) {
    PSAM_REQUIRE(xyz && pose && keys && bits, PSAM_EINVAL, "psam_view_lift_bits: null pointer");
    PSAM_REQUIRE(N > 0 && N <= VIEW_MAX_POINTS, PSAM_EINVAL, "psam_view_lift_bits: need 0 < N <= 2^28");
    PSAM_REQUIRE(K > 0 && (img || K == 1), PSAM_EINVAL, "psam_view_lift_bits: need K > 0, and K == 1 without images (the visible set)");
    PSAM_REQUIRE(tau >= 0.0f, PSAM_EINVAL, "psam_view_lift_bits: tau must not be negative or NaN");
    ViewCamera C = {};
    int32_t st = view_camera("psam_view_lift_bits", pose, fx, fy, cx, cy, width, height, znear, C);
    if (st != PSAM_OK) return st;
    PSAM_REQUIRE((((uintptr_t)keys | (uintptr_t)bits) & 7) == 0 && (((uintptr_t)xyz | (uintptr_t)area) & 3) == 0, PSAM_EALIGN,
                 "psam_view_lift_bits: keys and bits must be 8-byte aligned, xyz and area 4-byte aligned");
    const int64_t Wd = psam_cdiv(N, 64);
    hipLaunchKernelGGL(view_lift_kernel, dim3((unsigned)psam_cdiv(Wd, VIEW_THREADS / WAVE)), dim3(VIEW_THREADS), 0, stream, xyz, (int)N, C, (const u64*)keys, tau,
                       img, (int)K, (u64*)bits, Wd);
    st = psam_launch_status("psam_view_lift_bits: launch failed");
    if (st != PSAM_OK || !area) return st;
    hipLaunchKernelGGL(row_popcount_kernel<VIEW_THREADS>, dim3((unsigned)K), dim3(VIEW_THREADS), 0, stream, (const u64*)bits, Wd, (int*)area);
    return psam_launch_status("psam_view_lift_bits: area launch failed");
}
