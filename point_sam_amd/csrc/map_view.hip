// Scan map views (point_sam_amd/scanmap.py: ScanMap.view): the map as a camera inside it sees it, by casting one ray per pixel through the map's own
// hash grid.  The answer is views.hip's picture -- keys [H, W], (bits(depth) << 32) | index, all ones where a pixel is empty -- with the VOXEL ID in
// the index's place, so psam_view_pick, psam_view_paint_ids / _rows and everything built on the keys work on the map unchanged.
//   psam_mapview   map block + camera + eye -> keys [H, W]
//
// Definition (include/pointsam_hip.h, "scan map views"; tests/map_view_reference.py states it again in numpy and Python integers).  The eye's three
// fp32 words are the host's (-R^T t, rounded once); its cell o is a map point's (voxel_axis and the [-1, 1] test).  Pixel (px, py), every fp32
// operation rounded on its own:
//     a = ((float)px + 0.5f - cx) / fx,  b = ((float)py + 0.5f - cy) / fy
//     d_k = (R[0][k] a + R[1][k] b) + R[2][k]          the camera's direction (a, b, 1) taken back by R^T
//     m = max |d_k|; the pixel is empty unless every d_k is finite and m > 0
//     N_k = (int)rintf((d_k / m) * 2^21)               the longest axis is exactly +-2^21
// The ray is carve.hip's, between cell centres, from o towards the cell o + N, which lies outside every grid: carve_walk's difference form with
// n_a = |N_a|, tied axes stepping together.  The cells are SIGNED integers here, because the walk ends by leaving the grid 0 .. cmax,
// cmax = min((int)floorf(2 inv_h), 2^21 - 1): both the grid and the segment are convex, so a ray that has left never returns, and at most
// 3 (cmax + 1) trips are made.  |D_ab| < 2^44: every k_a stays <= cmax + 1 <= 2^21 and n_a <= 2^21.  The first crossed cell (the eye's own is none)
// that holds a pairable voxel v -- id below V, count >= min_count, its bit in `skip` clear: track.hip's rules -- whose mean (map_mean: psam_map_cloud's
// bits) has a depth c = pose_apply(P, mean).z with c >= near and c < inf ends the walk: key = (bits(c) << 32) | v.  Anything else is passed through.
// One thread owns one pixel and nothing is accumulated: the words are a function of the inputs alone.  The map block is only read.
//
// Layout.  A wave is an 8 x 8 tile of pixels, a workgroup 2 x 2 tiles: the lanes of a wave walk nearly the same cells and leave the loop together.
//
// Brick gate.  Most crossed cells are empty and each would cost a probe into the table.  A pre-pass over the V voxel ids (key_of_id, the row's count,
// `skip`) sets one bit per BRICK of (2^s)^3 cells that holds a pairable voxel, in the caller's workspace; the walk probes only cells whose brick
// bit is set.  A lookup is skipped, never a step: the visited cells and the result are the same by construction.  s = 3 (8^3 cells) for voxels down to
// 2^-10 and grows beyond, so that the bitmap never has more than 257 bricks per axis (2.1 MB: resident in L2).  A bitmap of at most
// MAP_VIEW_LDS_WORDS words (33^3 bits at voxel 2^-7 are 1124) is staged into LDS per workgroup.  psam_mapview's `flags` switch the gate and
// the staging off for measurement (profiles/map_view/README.md); no flag changes a word of the result.
//
// The walk is a second copy of carve_walk's arithmetic, not a shared header: carve_walk steps a packed key and ends on the distance to its end cell,
// this one steps signed coordinates and ends on the grid's bound, and what they share is the three selects per difference.  carve.hip is untouched.
#include "map_block.h"
#include "transfer_index.h"      // transfer_refuse
#include "view_camera.h"

#include <cmath>

constexpr int MAP_VIEW_TILE = 8;                                   // a wave: 8 x 8 pixels
constexpr int MAP_VIEW_SIDE = 16;                                  // a workgroup: 16 x 16 pixels, four waves
constexpr int MAP_VIEW_THREADS = MAP_VIEW_SIDE * MAP_VIEW_SIDE;
constexpr int MAP_VIEW_MAX_BRICKS = 257;                           // per axis
constexpr int MAP_VIEW_LDS_WORDS = 4096;                           // 16 KB: eight workgroups per CU keep their place
constexpr int MAP_VIEW_NO_GATE = PSAM_MAP_VIEW_NO_GATE, MAP_VIEW_NO_LDS = PSAM_MAP_VIEW_NO_LDS;
static_assert(MAP_VIEW_THREADS == 4 * WAVE, "four tiles per workgroup");

struct MapViewGrid {
    float inv_h;
    int cmax;            // the largest cell of an axis
    int shift;           // a brick is (1 << shift)^3 cells
    int nb;              // bricks per axis
    int words;           // u32 words of the bitmap
};

// The grid and the bitmap's shape of a map cleared with inv_h; false for an inv_h no map can have.
static inline bool map_view_grid(float inv_h, MapViewGrid& g) {
    if (!(std::isfinite(inv_h) && inv_h > 0.0f)) return false;
    const float top = floorf(2.0f * inv_h);                        // 2 inv_h is exact or +inf
    g.inv_h = inv_h;
    g.cmax = top < (float)(1 << VOXEL_AXIS_BITS) ? (int)top : (1 << VOXEL_AXIS_BITS) - 1;
    g.shift = 3;
    while ((g.cmax >> g.shift) + 1 > MAP_VIEW_MAX_BRICKS) ++g.shift;
    g.nb = (g.cmax >> g.shift) + 1;
    g.words = (int)(((int64_t)g.nb * g.nb * g.nb + 31) / 32);     // nb^3 <= 257^3 < 2^25
    return true;
}

struct MapViewEye {
    float v[3];
};

// ------------------------------------------------------------------------------------------------ the bricks
// One thread per voxel id; the bitmap was cleared on the stream before.  A key whose brick lies off the bitmap (no accepted point has one) sets nothing.
__global__ __launch_bounds__(MAP_THREADS) void map_view_bricks_kernel(const int* __restrict__ header, const u64* __restrict__ key_of_id,
                                                                     const u64* __restrict__ rows, int V, const u64* __restrict__ skip, int min_count,
                                                                     MapViewGrid g, unsigned* __restrict__ bricks) {
    const int v = blockIdx.x * MAP_THREADS + threadIdx.x;
    if (header[MAP_H_FLAGS] != 0) return;                          // uniform: whole waves stay for the shuffle below
    int bit = -1;
    if (v < V) {
        const u64 word = skip ? skip[v >> 6] : 0ull;
        constexpr u64 AXIS = (1ull << VOXEL_AXIS_BITS) - 1ull;
        const u64 key = key_of_id[v];
        const int b0 = (int)(key & AXIS) >> g.shift, b1 = (int)((key >> VOXEL_AXIS_BITS) & AXIS) >> g.shift,
                  b2 = (int)((key >> (2 * VOXEL_AXIS_BITS)) & AXIS) >> g.shift;
        const bool pairable = rows[(int64_t)v * MAP_ROW] >= (u64)min_count && !((word >> (v & 63)) & 1ull);
        // VOXEL_EMPTY, or no key at all, has bits above the three fields
        if (pairable && !(key >> (3 * VOXEL_AXIS_BITS)) && b0 < g.nb && b1 < g.nb && b2 < g.nb) bit = (b2 * g.nb + b1) * g.nb + b0;
    }
    // Voxel ids follow the scans' order, so neighbours in id are neighbours in space: 4 x 10^5 voxels of a room at voxel 2^-7 share 1124 words, and
    // with one atomic per voxel a gated view measured 0.2 to 0.3 ms MORE than one without the gate (profiles/map_view/README.md).  A lane whose neighbour below has the same bit leaves it to the neighbour, and a bit
    // that a load already shows set is not set again: bits are only ever set, so a stale load can only cost an atomic, never lose one.
    const int below = __shfl_up(bit, 1, 64);
    if (bit < 0 || ((threadIdx.x & 63) != 0 && below == bit)) return;
    unsigned* __restrict__ word = &bricks[bit >> 5];
    const unsigned mask = 1u << (bit & 31);
    if (!(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & mask)) atomicOr(word, mask);
}

// ------------------------------------------------------------------------------------------------ the rays
__device__ __forceinline__ int wave_sum_view(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// GATE: the bitmap is asked before a probe; LDS: it is staged into shared memory first; STATS: crossed cells and probes are counted into stats[0 .. 1].
template <bool GATE, bool LDS, bool STATS>
__global__ __launch_bounds__(MAP_VIEW_THREADS) void map_view_kernel(const int* __restrict__ header, const u64* __restrict__ keys, const int* __restrict__ id,
                                                                   int cv, const u64* __restrict__ rows, int V, const u64* __restrict__ skip, int min_count,
                                                                   ViewCamera C, MapViewEye eye, MapViewGrid g, const unsigned* __restrict__ bricks,
                                                                   u64* __restrict__ out, u64* __restrict__ stats) {
#pragma clang fp contract(off)
    __shared__ unsigned s_bricks[LDS ? MAP_VIEW_LDS_WORDS : 1];
    const unsigned* __restrict__ bm = bricks;
    if constexpr (GATE && LDS) {
        for (int w = threadIdx.x; w < g.words; w += MAP_VIEW_THREADS) s_bricks[w] = bricks[w];      // g.words <= MAP_VIEW_LDS_WORDS: the entry's choice
        __syncthreads();
        bm = s_bricks;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int px = blockIdx.x * MAP_VIEW_SIDE + (wave & 1) * MAP_VIEW_TILE + (lane & 7);
    const int py = blockIdx.y * MAP_VIEW_SIDE + (wave >> 1) * MAP_VIEW_TILE + (lane >> 3);
    const bool inside = px < C.W && py < C.H;
    u64 key = VIEW_EMPTY;
    int crossed = 0, probes = 0;
    // a dead map, or a block that was cleared with another voxel size than the grid was laid out for, shows nothing
    bool live = inside && header[MAP_H_FLAGS] == 0 && header[MAP_H_INV_H] == __builtin_bit_cast(int, g.inv_h);
    u64 o[3] = {0, 0, 0};
    if (live)
        live = voxel_axis(eye.v[0], -1.0f, g.inv_h, o[0]) & voxel_axis(eye.v[1], -1.0f, g.inv_h, o[1]) & voxel_axis(eye.v[2], -1.0f, g.inv_h, o[2]) &
               (eye.v[0] >= -1.0f && eye.v[0] <= 1.0f) & (eye.v[1] >= -1.0f && eye.v[1] <= 1.0f) & (eye.v[2] >= -1.0f && eye.v[2] <= 1.0f);
    int N0 = 0, N1 = 0, N2 = 0;
    if (live) {
        const float a = ((float)px + 0.5f - C.cx) / C.fx, b = ((float)py + 0.5f - C.cy) / C.fy;
        const float d0 = (C.P.m[0] * a + C.P.m[4] * b) + C.P.m[8], d1 = (C.P.m[1] * a + C.P.m[5] * b) + C.P.m[9],
                    d2 = (C.P.m[2] * a + C.P.m[6] * b) + C.P.m[10];
        const float m = fmaxf(fabsf(d0), fmaxf(fabsf(d1), fabsf(d2)));
        live = fabsf(d0) < INFINITY && fabsf(d1) < INFINITY && fabsf(d2) < INFINITY && m > 0.0f;      // a NaN compares false
        if (live) {                                                // |d_k / m| <= 1: the conversions are of values in [-2^21, 2^21]
            N0 = (int)rintf((d0 / m) * 2097152.0f);
            N1 = (int)rintf((d1 / m) * 2097152.0f);
            N2 = (int)rintf((d2 / m) * 2097152.0f);
        }
    }
    if (live) {
        const int n0 = N0 < 0 ? -N0 : N0, n1 = N1 < 0 ? -N1 : N1, n2 = N2 < 0 ? -N2 : N2;
        const int s0 = N0 < 0 ? -1 : 1, s1 = N1 < 0 ? -1 : 1, s2 = N2 < 0 ? -1 : 1;
        const long long e0 = 2ll * n0, e1 = 2ll * n1, e2 = 2ll * n2;
        long long D01 = (long long)n1 - n0, D02 = (long long)n2 - n0, D12 = (long long)n2 - n1;      // k = 0
        int c0 = (int)o[0], c1 = (int)o[1], c2 = (int)o[2];
        const int trips = 3 * (g.cmax + 1);                        // every trip steps an axis, and no axis steps more than cmax + 1 times inside the grid
        for (int trip = 0; trip < trips; ++trip) {
            const bool t0 = D01 <= 0 && D02 <= 0, t1 = D01 >= 0 && D12 <= 0, t2 = D02 >= 0 && D12 >= 0;
            c0 += t0 ? s0 : 0; c1 += t1 ? s1 : 0; c2 += t2 ? s2 : 0;
            D01 += (t0 ? e1 : 0ll) - (t1 ? e0 : 0ll);
            D02 += (t0 ? e2 : 0ll) - (t2 ? e0 : 0ll);
            D12 += (t1 ? e2 : 0ll) - (t2 ? e1 : 0ll);
            if ((unsigned)c0 > (unsigned)g.cmax || (unsigned)c1 > (unsigned)g.cmax || (unsigned)c2 > (unsigned)g.cmax) break;      // left the grid: empty
            if (STATS) ++crossed;
            if constexpr (GATE) {
                const int bit = (((c2 >> g.shift) * g.nb) + (c1 >> g.shift)) * g.nb + (c0 >> g.shift);      // c <= cmax: below nb^3
                if (!((bm[bit >> 5] >> (bit & 31)) & 1u)) continue;
            }
            if (STATS) ++probes;
            const int at = voxel_find(keys, cv, voxel_key((u64)c0, (u64)c1, (u64)c2));
            if (at < 0) continue;
            const int v = id[at];
            if (v < 0 || v >= V) continue;
            const ulonglong2* __restrict__ row = (const ulonglong2*)(rows + (int64_t)v * MAP_ROW);
            const ulonglong2 lo = row[0];                          // count, sum x
            const u64 word = skip ? skip[v >> 6] : 0ull;
            if (lo.x < (u64)min_count || ((word >> (v & 63)) & 1ull)) continue;
            const ulonglong2 hi = row[1];                          // sum y, sum z
            float ca, cb, cc;
            pose_apply(C.P, map_mean(lo.y, lo.x), map_mean(hi.x, lo.x), map_mean(hi.y, lo.x), ca, cb, cc);
            if (!(cc >= C.znear && cc < INFINITY)) continue;       // in front of near, or no depth at all: seen through
            key = ((u64)__builtin_bit_cast(unsigned, cc) << 32) | (u64)(unsigned)v;
            break;
        }
    }
    if (inside) out[(int64_t)py * C.W + px] = key;
    if constexpr (STATS) {                                         // a wave's rays cross fewer than 64 * 3 * 2^21 < 2^30 cells
        const int wave_crossed = wave_sum_view(crossed), wave_probes = wave_sum_view(probes);
        if (lane == 0 && wave_crossed) atomicAdd(&stats[0], (u64)wave_crossed);
        if (lane == 0 && wave_probes) atomicAdd(&stats[1], (u64)wave_probes);
    }
}

// ------------------------------------------------------------------------------------------------ entries
PSAM_API size_t psam_mapview_ws_bytes(float inv_h) {
    MapViewGrid g = {};
    return map_view_grid(inv_h, g) ? align16((size_t)g.words * sizeof(unsigned)) : 0;
}

template <bool GATE, bool LDS>
static inline void map_view_launch(bool counted, dim3 grid, hipStream_t stream, const MapBlock& b, int V, const u64* skip, int min_count, const ViewCamera& C,
                                   const MapViewEye& eye, const MapViewGrid& g, const unsigned* bricks, u64* keys, u64* stats) {
    if (counted)
        hipLaunchKernelGGL((map_view_kernel<GATE, LDS, true>), grid, dim3(MAP_VIEW_THREADS), 0, stream, (const int*)b.header, (const u64*)b.keys, (const int*)b.id,
                           b.cv, (const u64*)b.rows, V, skip, min_count, C, eye, g, bricks, keys, stats);
    else
        hipLaunchKernelGGL((map_view_kernel<GATE, LDS, false>), grid, dim3(MAP_VIEW_THREADS), 0, stream, (const int*)b.header, (const u64*)b.keys, (const int*)b.id,
                           b.cv, (const u64*)b.rows, V, skip, min_count, C, eye, g, bricks, keys, stats);
}

PSAM_API int32_t psam_mapview(const void* map, size_t map_bytes, int32_t max_voxels, int32_t max_pairs, int32_t V, float inv_h, const float* pose, float fx,
                               float fy, float cx, float cy, int32_t width, int32_t height, float znear, const float* eye, const uint64_t* skip,
                               int32_t min_count, int32_t flags, uint64_t* keys, uint64_t* stats, void* ws, size_t ws_bytes, hipStream_t stream) {
    static const char* const name = "psam_mapview";
    if (!(map && pose && eye && keys && ws)) return transfer_refuse(PSAM_EINVAL, name, "null pointer");
    if (!map_caps_ok(max_voxels, max_pairs)) return transfer_refuse(PSAM_EINVAL, name, "need 0 < max_voxels <= 2^28 and 0 < max_pairs <= 2^28");
    if (!(V > 0 && V <= max_voxels)) return transfer_refuse(PSAM_EINVAL, name, "need 0 < V <= max_voxels (an empty map has no view)");
    MapViewGrid g = {};
    if (!map_view_grid(inv_h, g)) return transfer_refuse(PSAM_EINVAL, name, "inv_h must be finite and positive");
    if (!(width >= 1 && width <= VIEW_MAX_SIDE && height >= 1 && height <= VIEW_MAX_SIDE))
        return transfer_refuse(PSAM_EINVAL, name, "width and height must lie in [1, 8192]");
    if (!(std::isfinite(fx) && fx > 0.0f && std::isfinite(fy) && fy > 0.0f)) return transfer_refuse(PSAM_EINVAL, name, "fx and fy must be finite and positive");
    if (!(std::isfinite(cx) && std::isfinite(cy))) return transfer_refuse(PSAM_EINVAL, name, "cx and cy must be finite");
    if (!(std::isfinite(znear) && znear > 0.0f)) return transfer_refuse(PSAM_EINVAL, name, "near must be finite and positive");
    ViewCamera C = {};
    if (!pose_load(pose, C.P)) return transfer_refuse(PSAM_EINVAL, name, "pose must be finite");
    MapViewEye e = {{eye[0], eye[1], eye[2]}};
    for (int a = 0; a < 3; ++a)
        if (!(e.v[a] >= -1.0f && e.v[a] <= 1.0f)) return transfer_refuse(PSAM_EINVAL, name, "the eye must lie in [-1, 1]^3");
    if (!(min_count >= 1)) return transfer_refuse(PSAM_EINVAL, name, "min_count must be at least 1");
    if (flags & ~(MAP_VIEW_NO_GATE | MAP_VIEW_NO_LDS)) return transfer_refuse(PSAM_EINVAL, name, "unknown flags");
    if (!((((uintptr_t)map | (uintptr_t)ws) & 15) == 0 && (((uintptr_t)skip | (uintptr_t)keys | (uintptr_t)stats) & 7) == 0))
        return transfer_refuse(PSAM_EALIGN, name, "map and ws must be 16-byte aligned, skip, keys and stats 8-byte aligned");
    if (map_bytes < map_layout(nullptr, max_voxels, max_pairs).bytes) return transfer_refuse(PSAM_EWORKSPACE, name, "map block too small (psam_map_bytes)");
    if (ws_bytes < psam_mapview_ws_bytes(inv_h)) return transfer_refuse(PSAM_EWORKSPACE, name, "workspace too small (psam_mapview_ws_bytes)");
    C.fx = fx; C.fy = fy; C.cx = cx; C.cy = cy;
    C.width = (float)width; C.height = (float)height;
    C.znear = znear;
    C.W = width; C.H = height;
    const MapBlock b = map_layout((void*)map, max_voxels, max_pairs);
    const bool gate = !(flags & MAP_VIEW_NO_GATE), lds = gate && !(flags & MAP_VIEW_NO_LDS) && g.words <= MAP_VIEW_LDS_WORDS;
    unsigned* bricks = (unsigned*)ws;
    if (gate) {
        if (hipMemsetAsync(bricks, 0, (size_t)g.words * sizeof(unsigned), stream) != hipSuccess) {
            (void)hipGetLastError();
            psam_set_error("psam_mapview: clearing the workspace failed");
            return PSAM_EINVAL;
        }
        hipLaunchKernelGGL(map_view_bricks_kernel, dim3((unsigned)psam_cdiv(V, MAP_THREADS)), dim3(MAP_THREADS), 0, stream, (const int*)b.header,
                           (const u64*)b.key_of_id, (const u64*)b.rows, (int)V, (const u64*)skip, (int)min_count, g, bricks);
        const int32_t st = psam_launch_status("psam_mapview: bricks launch failed");
        if (st != PSAM_OK) return st;
    }
    const dim3 grid((unsigned)psam_cdiv(width, MAP_VIEW_SIDE), (unsigned)psam_cdiv(height, MAP_VIEW_SIDE));
    if (!gate) map_view_launch<false, false>(stats != nullptr, grid, stream, b, V, (const u64*)skip, min_count, C, e, g, bricks, (u64*)keys, (u64*)stats);
    else if (lds) map_view_launch<true, true>(stats != nullptr, grid, stream, b, V, (const u64*)skip, min_count, C, e, g, bricks, (u64*)keys, (u64*)stats);
    else map_view_launch<true, false>(stats != nullptr, grid, stream, b, V, (const u64*)skip, min_count, C, e, g, bricks, (u64*)keys, (u64*)stats);
    return psam_launch_status("psam_mapview: launch failed");
}
