// Surface normals and curvature per occupied voxel (point_sam_amd/superpoints.py): the eigenvector of the smallest eigenvalue of the scatter matrix of a
// voxel's neighbourhood -- every point whose voxel is v or one of nbr[v, 0 .. 25] (psam_region_neighbors).  All points of a voxel share its normal.
//
// The scatter matrix is EXACT.  A coordinate p in [-1, 1] has the fixed-point value q = floor((double)p * 2^20) + 2^20, an integer in [0, 2^21]
// (conversion, product with a power of two, floor and sum are all exact).  With n points, s = sum q and P = sum q q^T, S = n P - s s^T is an integer
// matrix: formed in 128-bit integer arithmetic and converted to fp64 once, it does not depend on the order of the points or on the launch schedule.
//   moments   one thread per point, integer atomic adds into table [V, 16] u64: count, s (3), then the six products xx, xy, xz, yy, yz, zz in two
//             limbs each -- the low 32 bits of q_a q_b into one word, the rest into another
//   eigen     one thread per voxel: adds up to 27 table rows, forms S in __int128, converts, solves in fp64 (cyclic Jacobi), writes the outputs
//
// No overflow, for EVERY accepted shape (0 < N <= 2^28, 0 < V <= N, any voxel size): a neighbourhood is a set of distinct points, so n <= N <= 2^28.
//   q <= 2^21                          s_a <= 2^28 * 2^21 = 2^49                               (one u64 word)
//   q_a q_b <= 2^42: low limb < 2^32   sum of low limbs < 2^28 * 2^32 = 2^60                   (one u64 word)
//                    high limb <= 2^10 sum of high limbs <= 2^28 * 2^10 = 2^38                 (one u64 word)
//   P_ab = high * 2^32 + low <= 2^70, n P_ab <= 2^98 and s_a s_b <= 2^98: both, and their difference, fit a signed 128-bit integer.
// A sum over 27 rows of the table is a sum over the neighbourhood's points, so the same bounds hold for it.  N above 2^28 is refused before launch.
//
// int128 -> fp64 is done here, not left to the compiler's run-time routine: the value's top 64 bits with a sticky bit for the rest, one correctly
// rounded u64 -> fp64 conversion (the sticky bit sits ten places below the rounding position), and an exact scaling.  Round to nearest even, like
// float(int) of the reference.
#include "common.h"

#include <cmath>

typedef unsigned long long u64;
typedef __int128 i128;
typedef unsigned __int128 u128;

constexpr int NORMAL_THREADS = 256;
constexpr int NORMAL_MAX_POINTS = 1 << 28;
constexpr int NORMAL_ROW = 16;                     // u64 words per voxel of the table: count, 3 sums, 6 low limbs, 6 high limbs
constexpr int NORMAL_SWEEPS = 24;                  // cyclic Jacobi converges quadratically: a 3 x 3 matrix is diagonal to the last bit after five or six

static inline unsigned normal_blocks(int64_t n) { return (unsigned)psam_cdiv(n, NORMAL_THREADS); }

// ------------------------------------------------------------------------------------------------ moments
__global__ __launch_bounds__(NORMAL_THREADS) void normal_clear_kernel(u64* __restrict__ table, int64_t words) {
    const int64_t stride = (int64_t)gridDim.x * NORMAL_THREADS;
    for (int64_t t = (int64_t)blockIdx.x * NORMAL_THREADS + threadIdx.x; t < words; t += stride) table[t] = 0ull;
}

// q of one coordinate; false for a value that is not finite or outside [-1, 1] (NaN compares false)
__device__ __forceinline__ bool normal_fixed(float p, u64& q) {
    if (!(p >= -1.0f && p <= 1.0f)) return false;
    q = (u64)((long long)floor((double)p * 1048576.0) + 1048576ll);
    return true;
}

__global__ __launch_bounds__(NORMAL_THREADS) void normal_moments_kernel(const float* __restrict__ xyz, const int64_t* __restrict__ inv, int N, int V,
                                                                      u64* __restrict__ table) {
    const int i = blockIdx.x * NORMAL_THREADS + threadIdx.x;
    if (i >= N) return;
    const int64_t v = inv[i];
    if ((u64)v >= (u64)V) return;
    u64 q[3];
    if (!(normal_fixed(xyz[(int64_t)i * 3 + 0], q[0]) & normal_fixed(xyz[(int64_t)i * 3 + 1], q[1]) & normal_fixed(xyz[(int64_t)i * 3 + 2], q[2]))) return;
    u64* __restrict__ row = table + v * NORMAL_ROW;
    atomicAdd(&row[0], 1ull);
    atomicAdd(&row[1], q[0]); atomicAdd(&row[2], q[1]); atomicAdd(&row[3], q[2]);
    const u64 p[6] = {q[0] * q[0], q[0] * q[1], q[0] * q[2], q[1] * q[1], q[1] * q[2], q[2] * q[2]};
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        atomicAdd(&row[4 + c], p[c] & 0xffffffffull);
        atomicAdd(&row[10 + c], p[c] >> 32);
    }
}

// ------------------------------------------------------------------------------------------------ eigen
__device__ __forceinline__ double normal_to_double(i128 v) {
    const bool neg = v < 0;
    const u128 m = neg ? (u128)0 - (u128)v : (u128)v;
    const u64 hi = (u64)(m >> 64), lo = (u64)m;
    double d;
    if (hi == 0) {
        d = (double)lo;                                            // one rounding: hi32 * 2^32 (exact) + lo32 (exact)
    } else {
        const int shift = 64 - __builtin_clzll(hi);               // 1 .. 64: the value has 64 + shift bits
        u64 top = (u64)(m >> shift);
        const u128 rest = m & (((u128)1 << shift) - 1);
        if (rest != 0) top |= 1ull;                                // sticky
        d = ldexp((double)top, shift);
    }
    return neg ? -d : d;
}

// One Jacobi rotation of the symmetric matrix a (full storage) in the plane (P, Q), R the third axis; the columns of e follow.
template <int P, int Q, int R>
__device__ __forceinline__ void normal_rotate(double (&a)[3][3], double (&e)[3][3]) {
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    if (fabs(apq) <= 0x1p-70 * (fabs(a[P][P]) + fabs(a[Q][Q]))) {      // below the last bit of both diagonal entries: it is zero
        a[P][Q] = a[Q][P] = 0.0;
        return;
    }
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    a[P][P] = a[P][P] - t * apq;
    a[Q][Q] = a[Q][Q] + t * apq;
    a[P][Q] = a[Q][P] = 0.0;
    const double arp = a[R][P], arq = a[R][Q];
    a[R][P] = a[P][R] = c * arp - s * arq;
    a[R][Q] = a[Q][R] = s * arp + c * arq;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double erp = e[r][P], erq = e[r][Q];
        e[r][P] = c * erp - s * erq;
        e[r][Q] = s * erp + c * erq;
    }
}

__global__ __launch_bounds__(NORMAL_THREADS) void normal_eigen_kernel(const u64* __restrict__ table, const int* __restrict__ nbr, int V, int min_points,
                                                                    int has_view, float wx, float wy, float wz, int* __restrict__ count,
                                                                    double* __restrict__ scatter, float* __restrict__ normal,
                                                                    float* __restrict__ curvature) {
    const int v = blockIdx.x * NORMAL_THREADS + threadIdx.x;
    if (v >= V) return;
    u64 acc[NORMAL_ROW];
#pragma unroll
    for (int c = 0; c < NORMAL_ROW; ++c) acc[c] = table[(int64_t)v * NORMAL_ROW + c];
    for (int o = 0; o < 26; ++o) {
        const int u = nbr[(int64_t)v * 26 + o];
        if ((unsigned)u >= (unsigned)V) continue;
#pragma unroll
        for (int c = 0; c < NORMAL_ROW; ++c) acc[c] += table[(int64_t)u * NORMAL_ROW + c];
    }
    const u64 n = acc[0];
    // S = n P - s s^T, exact
    const int ia[6] = {0, 0, 0, 1, 1, 2}, ib[6] = {0, 1, 2, 1, 2, 2};
    double S[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const u128 P = ((u128)acc[10 + c] << 32) + (u128)acc[4 + c];
        S[c] = normal_to_double((i128)((u128)n * P) - (i128)((u128)acc[1 + ia[c]] * (u128)acc[1 + ib[c]]));
    }
    count[v] = (int)n;
    if (scatter) {
#pragma unroll
        for (int c = 0; c < 6; ++c) scatter[(int64_t)v * 6 + c] = S[c];
    }
    float out[3] = {0.0f, 0.0f, 0.0f}, curv = 0.0f;
    if ((int64_t)n >= (int64_t)min_points && n > 0) {
        // scaled by a power of two (exact) so that the largest entry is near 1: eigenvectors and the curvature do not change
        double big = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) big = fmax(big, fabs(S[c]));
        int ex = 0;
        if (big > 0.0) frexp(big, &ex);
        double a[3][3], e[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
#pragma unroll
        for (int c = 0; c < 6; ++c) a[ia[c]][ib[c]] = a[ib[c]][ia[c]] = ldexp(S[c], -ex);
        for (int sweep = 0; sweep < NORMAL_SWEEPS; ++sweep) {
            if (a[0][1] == 0.0 && a[0][2] == 0.0 && a[1][2] == 0.0) break;
            normal_rotate<0, 1, 2>(a, e);
            normal_rotate<0, 2, 1>(a, e);
            normal_rotate<1, 2, 0>(a, e);
        }
        // the smallest eigenvalue; on a tie the lowest axis
        double l0 = a[0][0], nx = e[0][0], ny = e[1][0], nz = e[2][0];
        if (a[1][1] < l0) { l0 = a[1][1]; nx = e[0][1]; ny = e[1][1]; nz = e[2][1]; }
        if (a[2][2] < l0) { l0 = a[2][2]; nx = e[0][2]; ny = e[1][2]; nz = e[2][2]; }
        const double len = sqrt(nx * nx + ny * ny + nz * nz);
        out[0] = (float)(nx / len); out[1] = (float)(ny / len); out[2] = (float)(nz / len);
        const double sum = (a[0][0] + a[1][1]) + a[2][2];
        l0 = l0 < 0.0 ? 0.0 : l0;                                  // S is positive semi-definite: below zero is rounding
        curv = sum > 0.0 ? (float)(l0 / sum) : 0.0f;
        // the sign, decided on the stored fp32 values
        bool flip;
        if (has_view) {
            const double dn = (double)n;
            const double mx = ((double)acc[1] / dn - 1048576.0) * 0x1p-20, my = ((double)acc[2] / dn - 1048576.0) * 0x1p-20,
                         mz = ((double)acc[3] / dn - 1048576.0) * 0x1p-20;
            const double d = ((double)out[0] * ((double)wx - mx) + (double)out[1] * ((double)wy - my)) +
                             (double)out[2] * ((double)wz - mz);
            flip = d < 0.0;
        } else {
            const float ax = fabsf(out[0]), ay = fabsf(out[1]), az = fabsf(out[2]);
            const float lead = (ax >= ay && ax >= az) ? out[0] : (ay >= az ? out[1] : out[2]);
            flip = lead < 0.0f;
        }
        if (flip) { out[0] = -out[0]; out[1] = -out[1]; out[2] = -out[2]; }
    }
    normal[(int64_t)v * 3 + 0] = out[0]; normal[(int64_t)v * 3 + 1] = out[1]; normal[(int64_t)v * 3 + 2] = out[2];
    curvature[v] = curv;
}

// ------------------------------------------------------------------------------------------------ entry
static inline bool normal_shape_ok(int32_t N, int32_t V) { return N > 0 && N <= NORMAL_MAX_POINTS && V > 0 && V <= N; }

PSAM_API size_t psam_normals_voxel_workspace_bytes(int32_t N, int32_t V) {
    return normal_shape_ok(N, V) ? (size_t)V * NORMAL_ROW * sizeof(u64) : 0;
}

PSAM_API int32_t psam_normals_voxel(const float* xyz, const int64_t* inv, const int32_t* nbr, int32_t N, int32_t V, int32_t min_points,
                                    const float* viewpoint, int32_t* count, double* scatter, float* normal, float* curvature, void* ws, size_t ws_bytes,
                                    hipStream_t stream) {
    PSAM_REQUIRE(xyz && inv && nbr && count && normal && curvature && ws, PSAM_EINVAL, "psam_normals_voxel: null pointer");
    PSAM_REQUIRE(normal_shape_ok(N, V), PSAM_EINVAL, "psam_normals_voxel: need 0 < N <= 2^28 and 0 < V <= N");
    PSAM_REQUIRE(min_points >= 1, PSAM_EINVAL, "psam_normals_voxel: min_points must be at least 1");
    PSAM_REQUIRE(!viewpoint || (std::isfinite(viewpoint[0]) && std::isfinite(viewpoint[1]) && std::isfinite(viewpoint[2])), PSAM_EINVAL,
                 "psam_normals_voxel: viewpoint must be finite");
    PSAM_REQUIRE(ws_bytes >= psam_normals_voxel_workspace_bytes(N, V), PSAM_EWORKSPACE,
                 "psam_normals_voxel: workspace too small (psam_normals_voxel_workspace_bytes)");
    PSAM_REQUIRE(((uintptr_t)ws & 15) == 0 && ((uintptr_t)scatter & 7) == 0, PSAM_EALIGN,
                 "psam_normals_voxel: workspace must be 16-byte aligned, scatter 8-byte aligned");
    u64* table = (u64*)ws;
    const int64_t words = (int64_t)V * NORMAL_ROW;
    hipLaunchKernelGGL(normal_clear_kernel, dim3(words < 4096 * (int64_t)NORMAL_THREADS ? normal_blocks(words) : 4096u), dim3(NORMAL_THREADS), 0, stream, table,
                       words);
    int32_t st = psam_launch_status("psam_normals_voxel: clear launch failed");
    if (st != PSAM_OK) return st;
    hipLaunchKernelGGL(normal_moments_kernel, dim3(normal_blocks(N)), dim3(NORMAL_THREADS), 0, stream, xyz, inv, (int)N, (int)V, table);
    if ((st = psam_launch_status("psam_normals_voxel: moments launch failed")) != PSAM_OK) return st;
    hipLaunchKernelGGL(normal_eigen_kernel, dim3(normal_blocks(V)), dim3(NORMAL_THREADS), 0, stream, (const u64*)table, nbr, (int)V, (int)min_points,
                       viewpoint ? 1 : 0, viewpoint ? viewpoint[0] : 0.0f, viewpoint ? viewpoint[1] : 0.0f, viewpoint ? viewpoint[2] : 0.0f, (int*)count, scatter, normal, curvature);
    return psam_launch_status("psam_normals_voxel: eigen launch failed");
}
