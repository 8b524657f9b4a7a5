// Instance geometry (point_sam_amd/geometry.py): where a packed mask is, how big it is and what colour it has, without unpacking it.
//   psam_instance_moments   per row of bits [K, W]: the point count, the fp32 bounding box and twelve fp64 sums (first and second moments, colour)
//   psam_instance_extents   per row: the fp32 box of the members in a given frame (origin, three axes) and the largest squared distance from the origin
//
// Work follows the set bits, not the width.  A wave owns GEOM_RANGE_WORDS consecutive words of one row (grid = ranges x rows, so one row of a large
// scan still spreads over the chip); each lane loads its GEOM_LANE_WORDS words up front (word j of lane l is base + 64 j + l: every load instruction
// of the wave is one contiguous 512-byte segment, and every word is read exactly once), drops the zero ones at once and walks the set bits of the
// others with ctz, gathering that point's coordinates and accumulating in registers.  A range without a set bit (the common case: an object is a
// few per cent of a scan) stores the identity and skips the reduction; any other range does ONE wave reduction and lane 0 stores the range's partial.
// A second kernel combines a row's partials in range order.  Nothing is accumulated across waves in flight, so there are no atomics, and:
//
//   the order of every fp64 addition is a function of (N, the row's bits) alone -- per lane: words j = 0 .. 3, bits ascending; per wave: the xor
//   butterfly 32, 16, 8, 4, 2, 1 (each step adds the same two values in both lanes, and IEEE addition commutes, so all lanes agree); per row: ranges
//   0, 1, 2, ... -- neither K, the row's position in the batch, nor the schedule enters it.  A row gives the same bits alone or among others, run to run.
//
// Min / max go through the order-preserving integer key of the fp32 pattern (-0 < +0, so the result does not depend on the order either).
// Every fp32 operation of the extents is rounded on its own (-ffp-contract=off); the fp64 terms of the moments are exact (a converted fp32 value, or
// the product of two: 48 significant bits), only their sums round.
#include "common.h"

typedef unsigned long long u64;

constexpr int GEOM_THREADS = 256;
constexpr int GEOM_LANE_WORDS = 4;
constexpr int GEOM_RANGE_WORDS = WAVE * GEOM_LANE_WORDS;       // 256 words = 16384 points per wave
constexpr int GEOM_MAX_POINTS = 1 << 28;
constexpr int GEOM_MAX_ROWS = 65535;                           // gridDim.y
constexpr int GEOM_SUMS = 12;
static_assert(GEOM_RANGE_WORDS == PSAM_INSTANCE_RANGE_WORDS, "the header documents the range a wave owns");

// fp32 -> unsigned, monotone over the whole number line (-inf < ... < -0 < +0 < ... < +inf); NaNs land at the two ends.
__device__ __forceinline__ unsigned geom_key(float f) {
    const unsigned u = __builtin_bit_cast(unsigned, f);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float geom_unkey(unsigned k) { return __builtin_bit_cast(float, k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }
constexpr unsigned GEOM_KEY_PINF = 0xff800000u, GEOM_KEY_NINF = 0x007fffffu;      // geom_key(+inf), geom_key(-inf): the identities of min and max

__device__ __forceinline__ unsigned geom_wave_min(unsigned v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, d, 64));
    return v;
}
__device__ __forceinline__ unsigned geom_wave_max(unsigned v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, d, 64));
    return v;
}

// The shared bit walk: the wave's range starts at word w0 of a row of W words; f(i) is called for every set bit i < N of the lane's words, in
// increasing i within a word and words in increasing j.  Bits at positions >= N are dropped before anything is indexed with them.  Returns whether
// ANY lane of the wave had a set bit (wave-uniform).
template <class F>
__device__ __forceinline__ bool geom_walk(const u64* __restrict__ row, int64_t W, int N, int64_t w0, int lane, F&& f) {
    u64 word[GEOM_LANE_WORDS];
#pragma unroll
    for (int j = 0; j < GEOM_LANE_WORDS; ++j) {
        const int64_t w = w0 + j * WAVE + lane;
        u64 m = w < W ? row[w] : 0ull;
        if (w == W - 1 && (N & 63)) m &= (1ull << (N & 63)) - 1ull;
        word[j] = m;
    }
    u64 any = 0;
#pragma unroll
    for (int j = 0; j < GEOM_LANE_WORDS; ++j) any |= word[j];
    if (__ballot(any != 0) == 0) return false;
#pragma unroll
    for (int j = 0; j < GEOM_LANE_WORDS; ++j) {
        const int base = (int)(w0 + j * WAVE + lane) * 64;      // < N <= 2^28 wherever a bit is set
        u64 m = word[j];
        while (m) {
            const int b = __builtin_ctzll(m);
            m &= m - 1;
            f(base + b);
        }
    }
    return true;
}

// ------------------------------------------------------------------------------------------------ moments
// Partials of (row k, range r) at slot k R + r: psum [K R, 12] f64, then pcnt [K R] int32, plo and phi [K R, 3] keys.
struct MomentsWs {
    double* psum;
    int* pcnt;
    unsigned* plo;
    unsigned* phi;
};
static inline size_t moments_ws_bytes(int64_t K, int64_t R) { return (size_t)(K * R) * (GEOM_SUMS * 8 + 4 + 12 + 12); }
static inline MomentsWs moments_ws(void* ws, int64_t K, int64_t R) {
    MomentsWs m;
    m.psum = (double*)ws;
    m.pcnt = (int*)(m.psum + K * R * GEOM_SUMS);
    m.plo = (unsigned*)(m.pcnt + K * R);
    m.phi = m.plo + K * R * 3;
    return m;
}

template <bool RGB>
__global__ __launch_bounds__(GEOM_THREADS) void moments_partial_kernel(const float* __restrict__ xyz, const float* __restrict__ rgb,
                                                                      const u64* __restrict__ bits, int64_t W, int N, int R, MomentsWs ws) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (GEOM_THREADS / WAVE) + (threadIdx.x >> 6);
    if (r >= R) return;                                            // wave-uniform
    const int k = blockIdx.y;
    int n = 0;
    double s[GEOM_SUMS];
#pragma unroll
    for (int c = 0; c < GEOM_SUMS; ++c) s[c] = 0.0;
    unsigned lo[3] = {GEOM_KEY_PINF, GEOM_KEY_PINF, GEOM_KEY_PINF}, hi[3] = {GEOM_KEY_NINF, GEOM_KEY_NINF, GEOM_KEY_NINF};
    const bool some = geom_walk(bits + (int64_t)k * W, W, N, (int64_t)r * GEOM_RANGE_WORDS, lane, [&](int i) {
        const float* __restrict__ p = xyz + (int64_t)i * 3;
        const float xf = p[0], yf = p[1], zf = p[2];
        const double x = (double)xf, y = (double)yf, z = (double)zf;
        ++n;
        s[0] = s[0] + x; s[1] = s[1] + y; s[2] = s[2] + z;
        s[3] = s[3] + x * x; s[4] = s[4] + x * y; s[5] = s[5] + x * z;
        s[6] = s[6] + y * y; s[7] = s[7] + y * z; s[8] = s[8] + z * z;
        if (RGB) {
            const float* __restrict__ q = rgb + (int64_t)i * 3;
            s[9] = s[9] + (double)q[0]; s[10] = s[10] + (double)q[1]; s[11] = s[11] + (double)q[2];
        }
        const unsigned kx = geom_key(xf), ky = geom_key(yf), kz = geom_key(zf);
        lo[0] = min(lo[0], kx); lo[1] = min(lo[1], ky); lo[2] = min(lo[2], kz);
        hi[0] = max(hi[0], kx); hi[1] = max(hi[1], ky); hi[2] = max(hi[2], kz);
    });
    const int64_t slot = (int64_t)k * R + r;
    if (some) {                                                    // wave-uniform: the whole wave takes part in the shuffles
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
#pragma unroll
        for (int c = 0; c < (RGB ? GEOM_SUMS : 9); ++c) s[c] = wave_sum_f64(s[c]);
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = geom_wave_min(lo[a]); hi[a] = geom_wave_max(hi[a]); }
    }
    if (lane == 0) {
        ws.pcnt[slot] = n;
#pragma unroll
        for (int c = 0; c < GEOM_SUMS; ++c) ws.psum[slot * GEOM_SUMS + c] = s[c];
#pragma unroll
        for (int a = 0; a < 3; ++a) { ws.plo[slot * 3 + a] = lo[a]; ws.phi[slot * 3 + a] = hi[a]; }
    }
}

// One wave per row; thread t < 12 adds column t of the row's partials in range order, 12 .. 17 take the box, 18 the count.
__global__ __launch_bounds__(WAVE) void moments_combine_kernel(MomentsWs ws, int R, int* __restrict__ count, double* __restrict__ sums,
                                                              float* __restrict__ lo, float* __restrict__ hi) {
    const int k = blockIdx.x, t = threadIdx.x;
    const int64_t s0 = (int64_t)k * R;
    if (t < GEOM_SUMS) {
        double acc = 0.0;
        for (int r = 0; r < R; ++r) acc = acc + ws.psum[(s0 + r) * GEOM_SUMS + t];
        sums[(int64_t)k * GEOM_SUMS + t] = acc;
    } else if (t < GEOM_SUMS + 3) {
        const int a = t - GEOM_SUMS;
        unsigned v = GEOM_KEY_PINF;
        for (int r = 0; r < R; ++r) v = min(v, ws.plo[(s0 + r) * 3 + a]);
        lo[(int64_t)k * 3 + a] = geom_unkey(v);
    } else if (t < GEOM_SUMS + 6) {
        const int a = t - GEOM_SUMS - 3;
        unsigned v = GEOM_KEY_NINF;
        for (int r = 0; r < R; ++r) v = max(v, ws.phi[(s0 + r) * 3 + a]);
        hi[(int64_t)k * 3 + a] = geom_unkey(v);
    } else if (t == GEOM_SUMS + 6) {
        int c = 0;
        for (int r = 0; r < R; ++r) c += ws.pcnt[s0 + r];
        count[k] = c;
    }
}

static inline bool geom_shape_ok(int64_t K, int64_t N) { return K > 0 && K <= GEOM_MAX_ROWS && N > 0 && N <= GEOM_MAX_POINTS; }
static inline int64_t geom_ranges(int64_t N) { return psam_cdiv(psam_cdiv(N, 64), GEOM_RANGE_WORDS); }

PSAM_API size_t psam_instance_moments_workspace_bytes(int32_t K, int32_t N) {
    return geom_shape_ok(K, N) ? moments_ws_bytes(K, geom_ranges(N)) : 0;
}

PSAM_API int32_t psam_instance_moments(const float* xyz, const float* rgb, const uint64_t* bits, int32_t K, int32_t N, int32_t* count, double* sums,
                                       float* lo, float* hi, void* ws, size_t ws_bytes, hipStream_t stream) {
    PSAM_REQUIRE(xyz && bits && count && sums && lo && hi && ws, PSAM_EINVAL, "psam_instance_moments: null pointer");
    PSAM_REQUIRE(geom_shape_ok(K, N), PSAM_EINVAL, "psam_instance_moments: need 0 < K <= 65535 and 0 < N <= 2^28");
    const int64_t W = psam_cdiv(N, 64), R = geom_ranges(N);
    PSAM_REQUIRE(ws_bytes >= moments_ws_bytes(K, R), PSAM_EINVAL, "psam_instance_moments: workspace too small (psam_instance_moments_workspace_bytes)");
    PSAM_REQUIRE((((uintptr_t)bits | (uintptr_t)sums | (uintptr_t)ws) & 7) == 0 &&
                     (((uintptr_t)xyz | (uintptr_t)rgb | (uintptr_t)count | (uintptr_t)lo | (uintptr_t)hi) & 3) == 0,
                 PSAM_EALIGN, "psam_instance_moments: bits, sums and ws must be 8-byte aligned, xyz, rgb, count, lo and hi 4-byte aligned");
    const MomentsWs m = moments_ws(ws, K, R);
    const dim3 grid((unsigned)psam_cdiv(R, GEOM_THREADS / WAVE), (unsigned)K), block(GEOM_THREADS);
    if (rgb) hipLaunchKernelGGL(moments_partial_kernel<true>, grid, block, 0, stream, xyz, rgb, (const u64*)bits, W, (int)N, (int)R, m);
    else hipLaunchKernelGGL(moments_partial_kernel<false>, grid, block, 0, stream, xyz, rgb, (const u64*)bits, W, (int)N, (int)R, m);
    const int32_t st = psam_launch_status("psam_instance_moments: launch failed");
    if (st != PSAM_OK) return st;
    hipLaunchKernelGGL(moments_combine_kernel, dim3((unsigned)K), dim3(WAVE), 0, stream, m, (int)R, (int*)count, sums, lo, hi);
    return psam_launch_status("psam_instance_moments: combine launch failed");
}

// ------------------------------------------------------------------------------------------------ extents
// Partials of (row k, range r): seven keys at slot (k R + r) * 7: lo[3], hi[3], r2max.
constexpr int GEOM_EXT = 7;

template <bool AXES>
__global__ __launch_bounds__(GEOM_THREADS) void extents_partial_kernel(const float* __restrict__ xyz, const u64* __restrict__ bits, int64_t W, int N,
                                                                      int R, const float* __restrict__ origin, const float* __restrict__ axes,
                                                                      unsigned* __restrict__ part) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (GEOM_THREADS / WAVE) + (threadIdx.x >> 6);
    if (r >= R) return;                                            // wave-uniform
    const int k = blockIdx.y;
    const float ox = origin[k * 3 + 0], oy = origin[k * 3 + 1], oz = origin[k * 3 + 2];
    float a[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    if (AXES) {
#pragma unroll
        for (int c = 0; c < 9; ++c) a[c] = axes[k * 9 + c];
    }
    unsigned lo[3] = {GEOM_KEY_PINF, GEOM_KEY_PINF, GEOM_KEY_PINF}, hi[3] = {GEOM_KEY_NINF, GEOM_KEY_NINF, GEOM_KEY_NINF}, far = GEOM_KEY_NINF;
    const bool some = geom_walk(bits + (int64_t)k * W, W, N, (int64_t)r * GEOM_RANGE_WORDS, lane, [&](int i) {
#pragma clang fp contract(off)
        const float* __restrict__ p = xyz + (int64_t)i * 3;
        const float dx = p[0] - ox, dy = p[1] - oy, dz = p[2] - oz;
        float q[3] = {dx, dy, dz};
        if (AXES) {
#pragma unroll
            for (int c = 0; c < 3; ++c) q[c] = (dx * a[c * 3 + 0] + dy * a[c * 3 + 1]) + dz * a[c * 3 + 2];
        }
        const float r2 = (dx * dx + dy * dy) + dz * dz;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned key = geom_key(q[c]);
            lo[c] = min(lo[c], key);
            hi[c] = max(hi[c], key);
        }
        far = max(far, geom_key(r2));
    });
    if (some) {                                                    // wave-uniform
#pragma unroll
        for (int c = 0; c < 3; ++c) { lo[c] = geom_wave_min(lo[c]); hi[c] = geom_wave_max(hi[c]); }
        far = geom_wave_max(far);
    }
    if (lane == 0) {
        unsigned* __restrict__ o = part + ((int64_t)k * R + r) * GEOM_EXT;
#pragma unroll
        for (int c = 0; c < 3; ++c) { o[c] = lo[c]; o[3 + c] = hi[c]; }
        o[6] = far;
    }
}

__global__ __launch_bounds__(WAVE) void extents_combine_kernel(const unsigned* __restrict__ part, int R, float* __restrict__ lo, float* __restrict__ hi,
                                                              float* __restrict__ r2max) {
    const int k = blockIdx.x, t = threadIdx.x;
    if (t >= GEOM_EXT) return;
    const bool is_min = t < 3;
    unsigned v = is_min ? GEOM_KEY_PINF : GEOM_KEY_NINF;
    for (int r = 0; r < R; ++r) {
        const unsigned u = part[((int64_t)k * R + r) * GEOM_EXT + t];
        v = is_min ? min(v, u) : max(v, u);
    }
    const float f = geom_unkey(v);
    if (t < 3) lo[(int64_t)k * 3 + t] = f;
    else if (t < 6) hi[(int64_t)k * 3 + t - 3] = f;
    else r2max[k] = f;
}

PSAM_API size_t psam_instance_extents_workspace_bytes(int32_t K, int32_t N) {
    return geom_shape_ok(K, N) ? (size_t)((int64_t)K * geom_ranges(N)) * GEOM_EXT * 4 : 0;
}

PSAM_API int32_t psam_instance_extents(const float* xyz, const uint64_t* bits, int32_t K, int32_t N, const float* origin, const float* axes, float* lo,
                                       float* hi, float* r2max, void* ws, size_t ws_bytes, hipStream_t stream) {
    PSAM_REQUIRE(xyz && bits && origin && lo && hi && r2max && ws, PSAM_EINVAL, "psam_instance_extents: null pointer");
    PSAM_REQUIRE(geom_shape_ok(K, N), PSAM_EINVAL, "psam_instance_extents: need 0 < K <= 65535 and 0 < N <= 2^28");
    const int64_t W = psam_cdiv(N, 64), R = geom_ranges(N);
    PSAM_REQUIRE(ws_bytes >= (size_t)(K * R) * GEOM_EXT * 4, PSAM_EINVAL, "psam_instance_extents: workspace too small (psam_instance_extents_workspace_bytes)");
    PSAM_REQUIRE(((uintptr_t)bits & 7) == 0 &&
                     (((uintptr_t)xyz | (uintptr_t)origin | (uintptr_t)axes | (uintptr_t)lo | (uintptr_t)hi | (uintptr_t)r2max | (uintptr_t)ws) & 3) == 0,
                 PSAM_EALIGN, "psam_instance_extents: bits must be 8-byte aligned, xyz, origin, axes, lo, hi, r2max and ws 4-byte aligned");
    const dim3 grid((unsigned)psam_cdiv(R, GEOM_THREADS / WAVE), (unsigned)K), block(GEOM_THREADS);
    if (axes) hipLaunchKernelGGL(extents_partial_kernel<true>, grid, block, 0, stream, xyz, (const u64*)bits, W, (int)N, (int)R, origin, axes, (unsigned*)ws);
    else hipLaunchKernelGGL(extents_partial_kernel<false>, grid, block, 0, stream, xyz, (const u64*)bits, W, (int)N, (int)R, origin, axes, (unsigned*)ws);
    const int32_t st = psam_launch_status("psam_instance_extents: launch failed");
    if (st != PSAM_OK) return st;
    hipLaunchKernelGGL(extents_combine_kernel, dim3((unsigned)K), dim3(WAVE), 0, stream, (const unsigned*)ws, (int)R, lo, hi, r2max);
    return psam_launch_status("psam_instance_extents: combine launch failed");
}
