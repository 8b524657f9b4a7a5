// A rigid pose as the kernels take it, shared by transfer.hip (query frame -> source frame) and views.hip (cloud frame -> camera frame): twelve fp32
// words, row-major 3 x 4, passed by value.  The arithmetic is one decision and lives here once:
//     p_a = ((P[a][0] x + P[a][1] y) + P[a][2] z) + P[a][3]
// every operation rounded on its own (the including translation units are built with -ffp-contract=off, and -fno-slp-vectorize: packed over two rows
// the products become v_pk_mul_f32 forms that broadcast one half of a register pair, which isa_lint.py refuses).
#pragma once
#include "common.h"

#include <cmath>

struct RigidPose {
    float m[12];
};

// pose: 12 floats in HOST memory.  False, and P untouched from the first bad entry on, if one is not finite.
static inline bool pose_load(const float* pose, RigidPose& P) {
    for (int a = 0; a < 12; ++a) {
        if (!std::isfinite(pose[a])) return false;
        P.m[a] = pose[a];
    }
    return true;
}

__device__ __forceinline__ void pose_apply(const RigidPose& P, float x, float y, float z, float& px, float& py, float& pz) {
#pragma clang fp contract(off)
    px = ((P.m[0] * x + P.m[1] * y) + P.m[2] * z) + P.m[3];
    py = ((P.m[4] * x + P.m[5] * y) + P.m[6] * z) + P.m[7];
    pz = ((P.m[8] * x + P.m[9] * y) + P.m[10] * z) + P.m[11];
}
