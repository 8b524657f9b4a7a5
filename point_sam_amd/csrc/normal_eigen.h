// What normals.hip (normals of a voxelised cloud) and map_normals.hip (normals of a scan map's voxels) share: the exact integer -> fp64 conversion of a
// scatter matrix, and everything after it -- the power-of-two scaling, the cyclic Jacobi solve, the choice of the smallest eigenvalue, the fp32 rounding,
// the curvature and the sign rule without a viewpoint -- are one decision and live here once.  Translation units that include this are compiled with
// -ffp-contract=off and -fno-slp-vectorize (point_sam_amd/build.py): every fp64 operation is rounded on its own.
#pragma once
#include "common.h"

#include <cmath>

typedef unsigned long long u64;
typedef __int128 i128;
typedef unsigned __int128 u128;

constexpr int NORMAL_SWEEPS = 24;                  // cyclic Jacobi converges quadratically: a 3 x 3 matrix is diagonal to the last bit after five or six

// int128 -> fp64, round to nearest even: the value's top 64 bits with a sticky bit for the rest, one correctly rounded u64 -> fp64 conversion (the
// sticky bit sits ten places below the rounding position), and an exact scaling.
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

// The eigenvector of the smallest eigenvalue of S (xx, xy, xz, yy, yz, zz; on a tie the lowest axis), normalised and rounded to fp32, and the
// curvature l0 / (l0 + l1 + l2).  The sign is the solve's: normal_flip_default decides it on the stored values.
__device__ __forceinline__ void normal_solve(const double (&S)[6], float (&out)[3], float& curv) {
    const int ia[6] = {0, 0, 0, 1, 1, 2}, ib[6] = {0, 1, 2, 1, 2, 2};
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
    l0 = l0 < 0.0 ? 0.0 : l0;                                      // S is positive semi-definite: below zero is rounding
    curv = sum > 0.0 ? (float)(l0 / sum) : 0.0f;
}

// The sign without a viewpoint, decided on the stored fp32 values: the component of largest magnitude (ties: the lowest axis) is positive.
__device__ __forceinline__ bool normal_flip_default(const float (&out)[3]) {
    const float ax = fabsf(out[0]), ay = fabsf(out[1]), az = fabsf(out[2]);
    const float lead = (ax >= ay && ax >= az) ? out[0] : (ay >= az ? out[1] : out[2]);
    return lead < 0.0f;
}
