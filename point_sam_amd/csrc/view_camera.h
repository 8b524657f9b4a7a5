// The pinhole camera as the kernels take it and the projection of a point, shared by views.hip (splat, lift) and fusion.hip (label fusion): one copy of
// the rule "in view" and of the centre pixel.  Definition: include/pointsam_hip.h, "camera views".  The including translation units are built with
// -ffp-contract=off and -fno-slp-vectorize (rigid_pose.h says why).
#pragma once
#include "common.h"
#include "rigid_pose.h"
#include "voxel_cell.h"      // u64

#include <cmath>

constexpr u64 VIEW_EMPTY = ~0ull;
constexpr int VIEW_MAX_SIDE = 8192;
constexpr int VIEW_MAX_POINTS = 1 << 28;

struct ViewCamera {
    RigidPose P;              // cloud frame -> camera frame
    float fx, fy, cx, cy;
    float width, height;      // the image's sides as fp32 (<= 8192: exact)
    float znear;
    int W, H;
};

// The centre pixel and the depth of a point, false if it is not in view.
__device__ __forceinline__ bool view_project(const ViewCamera& C, float x, float y, float z, int& px, int& py, float& depth) {
#pragma clang fp contract(off)
    float a, b, c;
    pose_apply(C.P, x, y, z, a, b, c);
    const float u = C.fx * (a / c) + C.cx;
    const float v = C.fy * (b / c) + C.cy;
    // every compare is false for a NaN; c < +inf with c >= near > 0 is "finite"
    const bool in = c >= C.znear && c < INFINITY && u >= 0.0f && u < C.width && v >= 0.0f && v < C.height;
    px = in ? (int)floorf(u) : 0;                                  // the conversion only of a value known to lie in [0, 8192)
    py = in ? (int)floorf(v) : 0;
    depth = c;
    return in;
}

// Whether a point in view at depth `depth` is visible behind the key of its centre pixel: the pixel is not empty and the point is at most tau behind
// its winner.  One rounded add; a NaN front (keys of no splat) is false.
__device__ __forceinline__ bool view_visible(u64 key, float depth, float tau) {
#pragma clang fp contract(off)
    const float front = __builtin_bit_cast(float, (unsigned)(key >> 32));
    return key != VIEW_EMPTY && depth <= front + tau;
}
