// Voxel cells and their hash, shared by scene.hip (the working cloud), crops.hip (a ball's working cloud) and regions.hip (the neighbourhood graph):
// one definition, so all put a point into the same cell bit for bit.  The table keyed by these cells is voxel_table.h.  Translation units that
// include this are compiled with -ffp-contract=off (point_sam_amd/build.py).
#pragma once
#include "common.h"

typedef unsigned long long u64;

constexpr int VOXEL_AXIS_BITS = 21;
constexpr int VOXEL_MAX_POINTS = 1 << 28;        // the table then has 2^29 slots: slot numbers and ranks stay in int32
constexpr u64 VOXEL_EMPTY = ~0ull;                // also the key of a point that has no cell (non-finite / out of range)

// open addressing at load factor <= 0.5
static inline int64_t voxel_capacity(int64_t M) {
    int64_t c = 64;
    while (c < 2 * M) c <<= 1;
    return c;
}
static inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

__device__ __forceinline__ bool voxel_axis(float x, float origin, float inv_h, u64& cell) {
#pragma clang fp contract(off)
    const float d = x - origin;
    const float s = d * inv_h;
    const float c = floorf(s);
    if (!(c >= 0.0f && c < (float)(1 << VOXEL_AXIS_BITS))) return false;      // NaN compares false: never an out-of-range cast
    cell = (u64)(unsigned)(int)c;
    return true;
}

__device__ __forceinline__ u64 voxel_key(u64 cx, u64 cy, u64 cz) { return cx | (cy << VOXEL_AXIS_BITS) | (cz << (2 * VOXEL_AXIS_BITS)); }

__device__ __forceinline__ u64 voxel_hash(u64 k) {      // the 64-bit finaliser of MurmurHash3
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
    return k ^ (k >> 33);
}
