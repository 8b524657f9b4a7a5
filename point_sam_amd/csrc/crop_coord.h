// The normalised coordinate of a scan point in a crop's ball (crops.hip: membership, cells and the gathered crop cloud; scene_interp.hip: the query
// coordinate of a scan point against the crop cloud).  One definition, so every user gets the same bits.  Translation units that include this are built
// with -ffp-contract=off.
#pragma once
#include "common.h"

struct CropBall {
    float cx, cy, cz, r2, inv_r;
};

// d = x - c per axis; q = (dx dx + dy dy) + dz dz; member iff q <= r2 (NaN: false).  u = clamp(d inv_r, -1, 1): one definition for the insert
// and the gather.
__device__ __forceinline__ bool crop_member(const float* __restrict__ p, const CropBall& b, float u[3]) {
#pragma clang fp contract(off)
    const float dx = p[0] - b.cx, dy = p[1] - b.cy, dz = p[2] - b.cz;
    const float q = (dx * dx + dy * dy) + dz * dz;
    u[0] = fminf(fmaxf(dx * b.inv_r, -1.0f), 1.0f);
    u[1] = fminf(fmaxf(dy * b.inv_r, -1.0f), 1.0f);
    u[2] = fminf(fmaxf(dz * b.inv_r, -1.0f), 1.0f);
    return q <= b.r2;
}
