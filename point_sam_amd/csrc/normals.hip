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
// int128 -> fp64 is done by hand (normal_eigen.h), not left to the compiler's run-time routine: the value's top 64 bits with a sticky bit for the rest, one correctly
// rounded u64 -> fp64 conversion (the sticky bit sits ten places below the rounding position), and an exact scaling.  Round to nearest even, like
// float(int) of the reference.
#include "normal_eigen.h"     // the int128 -> fp64 conversion and the eigen-solve, shared with map_normals.hip

constexpr int NORMAL_THREADS = 256;
constexpr int NORMAL_MAX_POINTS = 1 << 28;
constexpr int NORMAL_ROW = 16;                     // u64 words per voxel of the table: count, 3 sums, 6 low limbs, 6 high limbs

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

// ------------------------------------------------------------------------------------------------ eigen (the solve: normal_eigen.h)
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
        normal_solve(S, out, curv);
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
            flip = normal_flip_default(out);
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
