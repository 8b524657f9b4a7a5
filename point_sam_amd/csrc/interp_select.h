// The selection and the weights of a 3-NN plan, shared by scene_interp.hip (candidates: the 27 voxel representatives) and transfer.hip (candidates:
// the sources of another cloud within a radius): the three lowest candidates in (q, rank) and their inverse-distance weights are one definition
// (include/pointsam_hip.h, psam_interp_scene_plan) and live here once.  Translation units that include this are compiled with -ffp-contract=off.
#pragma once
#include "common.h"

#include <climits>

struct InterpBest {
    float q0, q1, q2;
    int r0, r1, r2;
};

__device__ __forceinline__ InterpBest interp_none() { return {__builtin_inff(), __builtin_inff(), __builtin_inff(), INT_MAX, INT_MAX, INT_MAX}; }

// (q, r) enters the ascending triple where it belongs; lexicographic, so a distance tie goes to the lower rank.  The unused entries are
// (+inf, INT_MAX): nothing compares below them but a real candidate, and an unused candidate (the same pair) displaces nothing.
__device__ __forceinline__ void interp_insert(InterpBest& b, float q, int r) {
    const bool lt0 = q < b.q0 || (q == b.q0 && r < b.r0);
    const bool lt1 = q < b.q1 || (q == b.q1 && r < b.r1);
    const bool lt2 = q < b.q2 || (q == b.q2 && r < b.r2);
    b.q2 = lt1 ? b.q1 : lt2 ? q : b.q2;
    b.r2 = lt1 ? b.r1 : lt2 ? r : b.r2;
    b.q1 = lt0 ? b.q0 : lt1 ? q : b.q1;
    b.r1 = lt0 ? b.r0 : lt1 ? r : b.r1;
    b.q0 = lt0 ? q : b.q0;
    b.r0 = lt0 ? r : b.r0;
}

// The point's six plan words from its triple: the blend; an exact hit or a lone candidate is a copy instead; no candidate at all is (-1, 0).
__device__ __forceinline__ void interp_finish(const InterpBest& b, float eps, int* __restrict__ oi, float* __restrict__ ow) {
#pragma clang fp contract(off)
    const bool two = b.r1 != INT_MAX, three = b.r2 != INT_MAX;
    const float a0 = 1.0f / fmaxf(b.q0, eps), a1 = 1.0f / fmaxf(b.q1, eps), a2 = 1.0f / fmaxf(b.q2, eps);
    float s = a0 + a1;
    if (three) s = s + a2;
    const bool copy = !two || b.q0 == 0.0f || b.r0 == INT_MAX;     // r0 == INT_MAX: no candidate entered (none in reach, or q is NaN for every one)
    oi[0] = b.r0 == INT_MAX ? -1 : b.r0;
    oi[1] = copy ? -1 : b.r1;
    oi[2] = copy || !three ? -1 : b.r2;
    ow[0] = b.r0 == INT_MAX ? 0.0f : copy ? 1.0f : a0 / s;
    ow[1] = copy ? 0.0f : a1 / s;
    ow[2] = copy || !three ? 0.0f : a2 / s;
}
