// The cell index of a source cloud, shared by transfer.hip (which builds it and plans the 3-NN transfer with it), align.hip and align_plane.hip (the
// nearest source of an ICP step) and align_score.hip (whether a posed query has a source in reach at all): the workspace layout, the cell of a
// point, the walk over a query's candidates (in two forms, see there) and the host's check of "an index, a query cloud, a radius" live here, so
// all of them put the same sources in front of a query bit for bit and refuse the same arguments in the same words.  The definition and the
// index's format: transfer.hip's header.  Translation units that include this are compiled with -ffp-contract=off -fno-slp-vectorize
// (point_sam_amd/build.py).
#pragma once
#include "common.h"
#include "voxel_table.h"

#include <cmath>
#include <cstdio>

constexpr int TRANSFER_THREADS = 256;
constexpr unsigned TRANSFER_END = ~0u;

struct TransferWs {
    VoxelWs table;        // keys [C], low [C] = the chain heads
    unsigned* next;       // [N]
    size_t bytes;
};

static inline TransferWs transfer_layout(void* ws, int64_t N) {
    TransferWs w = {};
    w.table = voxel_layout(ws, N, false, false);
    w.next = (unsigned*)((char*)ws + w.table.bytes);
    w.bytes = w.table.bytes + align16((size_t)N * sizeof(unsigned));
    return w;
}

static inline bool transfer_finite3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

__device__ __forceinline__ bool transfer_cell(float x, float y, float z, float ox, float oy, float oz, float inv_h, u64& cx, u64& cy, u64& cz) {
    return voxel_axis(x, ox, inv_h, cx) & voxel_axis(y, oy, inv_h, cy) & voxel_axis(z, oz, inv_h, cz);
}

// The finished index as a kernel reads it.
struct TransferIndexView {
    const float* __restrict__ src;        // [N, 3]
    const u64* __restrict__ keys;         // [capacity]
    const unsigned* __restrict__ head;    // [capacity]
    const unsigned* __restrict__ next;    // [N]
    int N, capacity;
};

static inline TransferIndexView transfer_view(const float* src, int64_t N, const void* ws) {
    const TransferWs w = transfer_layout(const_cast<void*>(ws), N);
    return {src, (const u64*)w.table.keys, (const unsigned*)w.table.low, (const unsigned*)w.next, (int)N, (int)voxel_capacity(N)};
}

// The candidates of the point p in cell (cx, cy, cz): 27 look-ups in the finished table, each followed by a walk along the cell's chain; f(q, j) for
// every indexed source j of those cells with q = (dx dx + dy dy) + dz dz <= r2 (NaN compares false), in chain order -- callers order by (q, j).
// Bounded: the chains of one query by N steps altogether, and an index outside [0, N) ends a chain.
template <class F>
__device__ __forceinline__ void transfer_candidates(const TransferIndexView& ix, float px, float py, float pz, u64 cx, u64 cy, u64 cz, float r2, F&& f) {
#pragma clang fp contract(off)
    const int64_t lim = (int64_t)1 << VOXEL_AXIS_BITS;
    int budget = ix.N;                                             // steps along all 27 chains together
    for (int o = 0; o < 27; ++o) {
        const int64_t nx = (int64_t)cx + (o % 3 - 1), ny = (int64_t)cy + (o / 3 % 3 - 1), nz = (int64_t)cz + (o / 9 - 1);
        if (nx < 0 || nx >= lim || ny < 0 || ny >= lim || nz < 0 || nz >= lim) continue;
        const int slot = voxel_find(ix.keys, ix.capacity, voxel_key((u64)nx, (u64)ny, (u64)nz));
        if (slot < 0) continue;
        unsigned j = ix.head[slot];
        while (j < (unsigned)ix.N && budget-- > 0) {               // TRANSFER_END is above every N
            const float* __restrict__ c = ix.src + (int64_t)j * 3;
            const float dx = px - c[0], dy = py - c[1], dz = pz - c[2];
            const float q = (dx * dx + dy * dy) + dz * dz;
            if (q <= r2) f(q, (int)j);
            j = ix.next[j];
        }
    }
}

// Whether the point p in cell (cx, cy, cz) has a candidate at all (align_score.hip): transfer_candidates' walk -- the same 27 cells in the same order,
// the same q, the same bound on the chain steps -- left at the first source with q <= r2.  True exactly where transfer_candidates would call f at
// least once: the steps the walk skips come after that call and cannot take it back.
__device__ __forceinline__ bool transfer_any_candidate(const TransferIndexView& ix, float px, float py, float pz, u64 cx, u64 cy, u64 cz, float r2) {
#pragma clang fp contract(off)
    const int64_t lim = (int64_t)1 << VOXEL_AXIS_BITS;
    int budget = ix.N;                                             // steps along all 27 chains together
    for (int o = 0; o < 27; ++o) {
        const int64_t nx = (int64_t)cx + (o % 3 - 1), ny = (int64_t)cy + (o / 3 % 3 - 1), nz = (int64_t)cz + (o / 9 - 1);
        if (nx < 0 || nx >= lim || ny < 0 || ny >= lim || nz < 0 || nz >= lim) continue;
        const int slot = voxel_find(ix.keys, ix.capacity, voxel_key((u64)nx, (u64)ny, (u64)nz));
        if (slot < 0) continue;
        unsigned j = ix.head[slot];
        while (j < (unsigned)ix.N && budget-- > 0) {               // TRANSFER_END is above every N
            const float* __restrict__ c = ix.src + (int64_t)j * 3;
            const float dx = px - c[0], dy = py - c[1], dz = pz - c[2];
            const float q = (dx * dx + dy * dy) + dz * dz;
            if (q <= r2) return true;
            j = ix.next[j];
        }
    }
    return false;
}
// The loop is written twice on purpose.  Written once (a visitor whose bool return ends the walk, with these two as one-line forms), it computes
// the same bits, but the step kernels that inline it compile to another block layout and ran 2.5 - 4 % slower on an MI355X where the chain walk
// dominates (profiles/align/README.md); so did every form of one loop that was tried.  Change the two together.

// ------------------------------------------------------------------------------------------------ the host's checks
// What an entry says when it refuses an index: its name, and the two texts in which the entries differ -- what it calls the index workspace, and which
// pointers it names when one of them is misaligned (one text for the workspace, one for the rest; an entry may use the same for both).
struct TransferEntry {
    const char* name;
    const char* ws_name;       // "workspace", "index workspace"
    const char* ws_aligned;
    const char* rest_aligned;
};

static inline int32_t transfer_refuse(int32_t code, const char* entry, const char* what, const char* more = "") {
    char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s%s", entry, what, more);
    psam_set_error(msg);
    return code;
}

// The values an index is built with (psam_transfer_index_build) and every later entry is given again.  `pointers`: none of the entry's is null.
static inline int32_t transfer_check_index(const TransferEntry& e, bool pointers, int64_t N, const float* origin, float inv_h) {
    if (!pointers) return transfer_refuse(PSAM_EINVAL, e.name, "null pointer");
    if (!(N > 0 && N <= VOXEL_MAX_POINTS)) return transfer_refuse(PSAM_EINVAL, e.name, "need 0 < N <= 2^28");
    if (!(std::isfinite(inv_h) && inv_h > 0.0f)) return transfer_refuse(PSAM_EINVAL, e.name, "inv_h must be finite and positive");
    if (!transfer_finite3(origin)) return transfer_refuse(PSAM_EINVAL, e.name, "origin must be finite");
    return PSAM_OK;
}

// The index workspace, after the values: its alignment, the alignment of the entry's other pointers (`rest`: whether all of them are aligned as
// the entry needs), its size.
static inline int32_t transfer_check_ws(const TransferEntry& e, const void* ws, size_t ws_bytes, int64_t N, bool rest) {
    if (((uintptr_t)ws & 15) != 0) return transfer_refuse(PSAM_EALIGN, e.name, e.ws_aligned);
    if (!rest) return transfer_refuse(PSAM_EALIGN, e.name, e.rest_aligned);
    if (ws_bytes < transfer_layout(nullptr, N).bytes) return transfer_refuse(PSAM_EWORKSPACE, e.name, e.ws_name, " too small (psam_transfer_index_workspace_bytes)");
    return PSAM_OK;
}

// "An index, a query cloud, a radius": what psam_transfer_plan, psam_align_step, psam_plane_step and psam_pose_score check alike, before anything of
// their own.  rest_given / rest_aligned: whether the entry's other pointers are non-null where they must be, and aligned as it needs.
static inline int32_t transfer_check_query(const TransferEntry& e, const float* src, int64_t N, const void* ws, size_t ws_bytes, const float* origin,
                                           float inv_h, float r2, const float* qry, int64_t M, bool rest_given, bool rest_aligned) {
    const int32_t st = transfer_check_index(e, src && ws && origin && qry && rest_given, N, origin, inv_h);
    if (st != PSAM_OK) return st;
    if (!(M > 0 && M <= VOXEL_MAX_POINTS)) return transfer_refuse(PSAM_EINVAL, e.name, "need 0 < M <= 2^28");
    if (!(std::isfinite(r2) && r2 > 0.0f)) return transfer_refuse(PSAM_EINVAL, e.name, "r2 must be finite and positive");
    return transfer_check_ws(e, ws, ws_bytes, N, (((uintptr_t)src | (uintptr_t)qry) & 3) == 0 && rest_aligned);
}
