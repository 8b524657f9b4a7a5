// Masks carried to the next scan (point_sam_amd/transfer.py): a radius-limited 3-NN search from the points of one cloud (the queries, optionally moved
// by a rigid pose) into another cloud (the sources), written as a plan (idx3, w3) in scene_interp.hip's format, so psam_interp_scene_rows and
// psam_interp_scene_bits apply it unchanged.  psam_interp_scene_plan cannot do this: its points are members of the grid they query (inv, nbr[inv]); a
// foreign point may fall into an empty cell, and with h = r a cell holds many sources.
//   psam_transfer_index_build   sources -> cell -> chain: the index, once per source cloud and radius
//   psam_transfer_plan          per query the up to three nearest sources within r among those of its own and the 26 surrounding cells
//
// Definition.  h = r, cells are voxel_cell.h's with (origin, inv_h).  The candidates of a query are the indexed sources j whose cell differs from the
// cell of p (the query, or P q with a pose) by at most 1 on every axis and whose q_j = (dx dx + dy dy) + dz dz <= r2, d = p - src[j]; NaN compares
// false.  A source without a cell is never a candidate, a query without a cell has none.  Selection and weights are interp_select.h's: the three
// lowest in (q, j), the copy rule, (-1, 0) for unused entries.  The 27-cell set IS the definition.  It equals the true radius-r search except where
// the fp32 rounding of (x - o) * inv_h moves a point across a cell face while it lies at distance ~ r from the other: a source in reach by q <= r2
// can then sit two cells away and is not seen.
//
// Index.  voxel_table.h's table over C = voxel_capacity(N) slots, the slot's u32 the HEAD of a chain of source indices, next [N] the links; all ones
// ends a chain.  A source claims its cell's slot (voxel_claim) and pushes itself by one atomic exchange of the head.  The order inside a chain is
// the arrival order and differs from run to run; the plan orders candidates by (q, j), so no output depends on it.  The layout is private to the
// workspace.  Every walk is bounded: a probe by the capacity, the chains of one query by N steps altogether (each source hangs in one chain), and an
// index outside [0, N) ends a chain, so a logic error ends as a wrong answer, not as a hang or a wild load.
//
// Every fp32 operation is rounded on its own (-ffp-contract=off).  Caller-owned workspace; no allocation, no host synchronisation.
#include "common.h"
#include "interp_select.h"
#include "rigid_pose.h"      // the pose and its arithmetic, shared with views.hip
#include "voxel_table.h"
#include "transfer_index.h" // the workspace on that table, the cell of a point and the walk over a query's candidates, shared with align.hip

// One thread per source.  next[j] is written by its own source only and read after the kernel boundary.
__global__ __launch_bounds__(TRANSFER_THREADS) void transfer_insert_kernel(const float* __restrict__ src, int N, float ox, float oy, float oz, float inv_h,
                                                                         u64* __restrict__ keys, unsigned* __restrict__ head, unsigned* __restrict__ next,
                                                                         int capacity) {
    const int j = blockIdx.x * TRANSFER_THREADS + threadIdx.x;
    if (j >= N) return;
    u64 cx, cy, cz;
    unsigned after = TRANSFER_END;
    if (transfer_cell(src[(int64_t)j * 3 + 0], src[(int64_t)j * 3 + 1], src[(int64_t)j * 3 + 2], ox, oy, oz, inv_h, cx, cy, cz)) {
        const int slot = voxel_claim(keys, capacity, voxel_key(cx, cy, cz));
        if (slot >= 0) after = atomicExch(&head[slot], (unsigned)j);
    }
    next[j] = after;
}

// One thread per query: transfer_candidates (27 look-ups in the finished table, each followed by a walk along the cell's chain).
template <bool POSE>
__global__ __launch_bounds__(TRANSFER_THREADS) void transfer_plan_kernel(const float* __restrict__ src, int N, const u64* __restrict__ keys,
                                                                       const unsigned* __restrict__ head, const unsigned* __restrict__ next, int capacity,
                                                                       float ox, float oy, float oz, float inv_h, float r2,
                                                                       const float* __restrict__ qry, int M, RigidPose P, float eps,
                                                                       int* __restrict__ idx3, float* __restrict__ w3) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * TRANSFER_THREADS + threadIdx.x;
    if (i >= M) return;
    const float x = qry[(int64_t)i * 3 + 0], y = qry[(int64_t)i * 3 + 1], z = qry[(int64_t)i * 3 + 2];
    float px = x, py = y, pz = z;
    if (POSE) pose_apply(P, x, y, z, px, py, pz);                  // query frame -> source frame
    InterpBest b = interp_none();
    u64 cx, cy, cz;
    if (transfer_cell(px, py, pz, ox, oy, oz, inv_h, cx, cy, cz)) {
        // built here from loose arguments: passed the view as one struct, the kernel measured 1.2 % slower
        const TransferIndexView ix = {src, keys, head, next, N, capacity};
        transfer_candidates(ix, px, py, pz, cx, cy, cz, r2, [&](float q, int j) { interp_insert(b, q, j); });
    }
    interp_finish(b, eps, idx3 + (int64_t)i * 3, w3 + (int64_t)i * 3);
}

PSAM_API size_t psam_transfer_index_workspace_bytes(int32_t N) {
    if (N <= 0 || N > VOXEL_MAX_POINTS) return 0;
    return transfer_layout(nullptr, N).bytes;
}

PSAM_API int32_t psam_transfer_index_build(const float* src, int32_t N, const float* origin, float inv_h, void* ws, size_t ws_bytes, hipStream_t stream) {
    static const char* const aligned = "workspace must be 16-byte aligned, src 4-byte aligned";
    static const TransferEntry entry = {"psam_transfer_index_build", "workspace", aligned, aligned};
    int32_t st = transfer_check_index(entry, src && origin && ws, N, origin, inv_h);
    if (st == PSAM_OK) st = transfer_check_ws(entry, ws, ws_bytes, N, ((uintptr_t)src & 3) == 0);
    if (st != PSAM_OK) return st;
    const TransferWs w = transfer_layout(ws, N);
    st = voxel_clear<0>(w.table, nullptr, stream, "psam_transfer_index_build: clear launch failed");
    if (st != PSAM_OK) return st;
    hipLaunchKernelGGL(transfer_insert_kernel, dim3((unsigned)psam_cdiv(N, TRANSFER_THREADS)), dim3(TRANSFER_THREADS), 0, stream, src, (int)N, origin[0],
                       origin[1], origin[2], inv_h, w.table.keys, w.table.low, w.next, (int)voxel_capacity(N));
    return psam_launch_status("psam_transfer_index_build: insert launch failed");
}

PSAM_API int32_t psam_transfer_plan(const float* src, int32_t N, const void* ws, size_t ws_bytes, const float* origin, float inv_h, float r2,
                                    const float* qry, int32_t M, const float* pose, float eps, int32_t* idx3, float* w3, hipStream_t stream) {
    static const TransferEntry entry = {"psam_transfer_plan", "workspace", "workspace must be 16-byte aligned", "src, qry, idx3 and w3 must be 4-byte aligned"};
    const int32_t st = transfer_check_query(entry, src, N, ws, ws_bytes, origin, inv_h, r2, qry, M, idx3 && w3, (((uintptr_t)idx3 | (uintptr_t)w3) & 3) == 0);
    if (st != PSAM_OK) return st;
    PSAM_REQUIRE(std::isfinite(eps) && eps > 0.0f, PSAM_EINVAL, "psam_transfer_plan: eps must be finite and positive");
    RigidPose P = {};
    PSAM_REQUIRE(!pose || pose_load(pose, P), PSAM_EINVAL, "psam_transfer_plan: pose must be finite");
    const TransferIndexView ix = transfer_view(src, N, ws);
    const dim3 grid((unsigned)psam_cdiv(M, TRANSFER_THREADS)), block(TRANSFER_THREADS);
    if (pose) {
        hipLaunchKernelGGL(transfer_plan_kernel<true>, grid, block, 0, stream, ix.src, ix.N, ix.keys, ix.head, ix.next, ix.capacity, origin[0],
                           origin[1], origin[2], inv_h, r2, qry, (int)M, P, eps, (int*)idx3, w3);
    } else {
        hipLaunchKernelGGL(transfer_plan_kernel<false>, grid, block, 0, stream, ix.src, ix.N, ix.keys, ix.head, ix.next, ix.capacity, origin[0],
                           origin[1], origin[2], inv_h, r2, qry, (int)M, P, eps, (int*)idx3, w3);
    }
    return psam_launch_status("psam_transfer_plan: launch failed");
}
