// The scan map's block and a point's way into it, shared by scanmap.hip (the map's own entries), carve.hip (free-space carving), track.hip (ICP steps
// on the map's voxels) and map_normals.hip (a normal per voxel): the block's layout, the header's words, the pose arithmetic, the acceptance test of a point and a voxel's mean are one decision and live here once.  The block is described
// at the top of scanmap.hip.  Translation units that include this are compiled with -ffp-contract=off and -fno-slp-vectorize (point_sam_amd/build.py).
#pragma once
#include "common.h"
#include "rigid_pose.h"
#include "voxel_table.h"     // which includes voxel_cell.h

constexpr int MAP_THREADS = 256;
constexpr int MAP_MAX_POINTS = 1 << 28;            // per add, and both capacities: ids, slots and ranks stay in int32
constexpr int MAP_ROW = 8;                         // u64 words per voxel
constexpr int MAP_HEADER_INTS = 16;
// header words (int32); PSAM_MAP_HEADER_INTS of include/pointsam_hip.h
constexpr int MAP_H_MAX_VOXELS = 0, MAP_H_MAX_PAIRS = 1, MAP_H_INV_H = 2, MAP_H_FLAGS = 3, MAP_H_V = 4, MAP_H_ADDS = 5, MAP_H_PAIRS = 6, MAP_H_NEW = 7,
              MAP_H_ACCEPTED = 8, MAP_H_REJECTED = 9, MAP_H_OBSERVED = 10;      // 10, 11: accepted observations of all adds, one u64
constexpr int MAP_FLAG_VOXELS = 1, MAP_FLAG_PAIRS = 2, MAP_FLAG_COUNTS = 4;
static_assert(MAP_HEADER_INTS == PSAM_MAP_HEADER_INTS, "header size");

struct MapBlock {
    int* header;
    u64* keys;           // [Cv]
    int* id;             // [Cv]
    u64* pair_keys;      // [Cp]
    unsigned* pair_count;// [Cp]
    u64* rows;           // [max_voxels, MAP_ROW]
    u64* best;           // [max_voxels]
    u64* key_of_id;      // [max_voxels]
    int cv, cp;
    size_t ones_at, ones_bytes, zero_at, bytes;      // the span cleared to all ones (keys, id, pair_keys) and the span cleared to zero (the rest)
};

static inline MapBlock map_layout(void* block, int64_t max_voxels, int64_t max_pairs) {
    MapBlock b = {};
    char* p = (char*)block;
    size_t o = 0;
    b.cv = (int)voxel_capacity(max_voxels);
    b.cp = (int)voxel_capacity(max_pairs);
    b.header = (int*)(p + o);              o += align16(MAP_HEADER_INTS * sizeof(int));
    b.ones_at = o;
    b.keys = (u64*)(p + o);                o += align16((size_t)b.cv * sizeof(u64));
    b.id = (int*)(p + o);                  o += align16((size_t)b.cv * sizeof(int));
    b.pair_keys = (u64*)(p + o);           o += align16((size_t)b.cp * sizeof(u64));
    b.ones_bytes = o - b.ones_at;
    b.zero_at = o;
    b.pair_count = (unsigned*)(p + o);     o += align16((size_t)b.cp * sizeof(unsigned));
    b.rows = (u64*)(p + o);                o += align16((size_t)max_voxels * MAP_ROW * sizeof(u64));
    b.best = (u64*)(p + o);                o += align16((size_t)max_voxels * sizeof(u64));
    b.key_of_id = (u64*)(p + o);           o += align16((size_t)max_voxels * sizeof(u64));
    b.bytes = o;
    return b;
}

static inline bool map_caps_ok(int64_t max_voxels, int64_t max_pairs) {
    return max_voxels > 0 && max_voxels <= MAP_MAX_POINTS && max_pairs > 0 && max_pairs <= MAP_MAX_POINTS;
}

// ------------------------------------------------------------------------------------------------ a point
// q of one value in [-1, 1] (normals.hip's fixed point); false for a value that is not finite or outside (NaN compares false)
__device__ __forceinline__ bool map_fixed(float p, u64& q) {
    if (!(p >= -1.0f && p <= 1.0f)) return false;
    q = (u64)((long long)floor((double)p * 1048576.0) + 1048576ll);
    return true;
}

// The posed position of point i, its fixed point and its key; false for a point the map does not accept.
template <bool POSED>
__device__ __forceinline__ bool map_point(const float* __restrict__ xyz, int64_t i, const RigidPose& P, float inv_h, u64 (&q)[3], u64& key) {
    float p[3] = {xyz[i * 3 + 0], xyz[i * 3 + 1], xyz[i * 3 + 2]};
    if (POSED) pose_apply(P, p[0], p[1], p[2], p[0], p[1], p[2]);
    u64 c[3];
    const bool ok = voxel_axis(p[0], -1.0f, inv_h, c[0]) & voxel_axis(p[1], -1.0f, inv_h, c[1]) & voxel_axis(p[2], -1.0f, inv_h, c[2]) &
                    map_fixed(p[0], q[0]) & map_fixed(p[1], q[1]) & map_fixed(p[2], q[2]);
    if (ok) key = voxel_key(c[0], c[1], c[2]);
    return ok;
}

__device__ __forceinline__ float map_inv_h(const int* __restrict__ header) { return __builtin_bit_cast(float, header[MAP_H_INV_H]); }

// ------------------------------------------------------------------------------------------------ a voxel's mean
// fl32(fl64(fl64(sum) / fl64(count)) * 2^-20 - 1): the quotient rounds once, the scaling is exact, the difference rounds once, then fp64 -> fp32
__device__ __forceinline__ float map_mean(u64 sum, u64 count) {
#pragma clang fp contract(off)
    const double m = (double)sum / (double)count;
    const double s = m * 0x1p-20;
    const double d = s - 1.0;
    return (float)d;
}

// ------------------------------------------------------------------------------------------------ a cell's slot, probed in stages
// voxel_find (voxel_table.h) from its second probe on: `cur` is what the first probe read at `pos`
__device__ __forceinline__ int map_find_rest(const u64* __restrict__ keys, int capacity, u64 key, unsigned pos, u64 cur) {
    const unsigned mask = (unsigned)capacity - 1u;
    for (int probe = 1; probe <= capacity; ++probe) {
        if (cur == VOXEL_EMPTY) break;
        if (cur == key) return (int)pos;
        if (probe == capacity) break;
        pos = (pos + 1u) & mask;
        cur = keys[pos];
    }
    return -1;
}
