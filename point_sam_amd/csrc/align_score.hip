// A global pose search's inner question (point_sam_amd/align.py: search): under each of P candidate poses, how many queries land on the other cloud?
//   psam_pose_score   counts[p] = the number of queries that have AT LEAST ONE candidate under pose p -- all P poses in one launch
//
// Definition.  The posed coordinate, the cell and the candidates of a query are psam_align_step's, bit for bit: pose_apply (rigid_pose.h),
// transfer_cell and the candidate set of transfer_candidates (transfer_index.h) -- the indexed sources of the 27 cells around cell(p) with
// q = (dx dx + dy dy) + dz dz <= r2 in fp32, NaN false.  The 27-cell set IS the definition; no cell is pruned by a geometric bound (align.hip's
// header: the fp32 rounding of the cell can put a source in reach one cell further than geometry suggests).  A query without a cell, and with it
// every query that is not finite, hits nothing.  So counts[p] == psam_align_step's sums[0] under pose p and the same r2, for every p.
//
// Early exit.  align_step needs the candidate lowest in (q, j) and must see them all; existence is settled by the first one, so the walk
// (transfer_any_candidate: the same cells, order and step bound) stops there.  A query deep inside the other cloud costs a probe or two; only a
// query that hits nothing pays for all 27.
//
// Shape.  One thread per query, the query in registers; a workgroup takes SCORE_THREADS queries through the SCORE_POSES poses of one chunk
// (grid: query tiles x pose chunks; past 65535 chunks a workgroup strides over them).  A pose's twelve words are read at a wave-uniform address,
// so they arrive by scalar loads and stay in scalar registers.  Per pose a wave adds __popcll(__ballot(hit)) with ONE integer atomicAdd, and none
// when nobody hit; the entry zeroes counts on the stream first.  Integer addition commutes and the totals stay below 2^28, so the words are a
// function of the inputs alone -- not of the schedule.  The poses are in DEVICE memory: the entry cannot look at them, the Python host validates them
// before the upload (ops.align_score).  A pose that is not finite gives NaN coordinates, no cell and a count of 0.
// Every fp32 operation is rounded on its own (-ffp-contract=off).  No workspace; no allocation, no host synchronisation.
#include "common.h"
#include "rigid_pose.h"
#include "transfer_index.h"

constexpr int SCORE_THREADS = 256;
constexpr int SCORE_POSES = PSAM_ALIGN_SCORE_POSES;
constexpr int SCORE_MAX_POSES = 1 << 20;
constexpr int SCORE_MAX_GRID_Y = 65535;

__global__ __launch_bounds__(SCORE_THREADS) void align_score_kernel(TransferIndexView ix, float ox, float oy, float oz, float inv_h, float r2,
                                                                    const float* __restrict__ qry, int M, const float* __restrict__ poses, int P,
                                                                    int* __restrict__ counts) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * SCORE_THREADS + threadIdx.x;
    if ((i & ~(WAVE - 1)) >= M) return;                            // wave-uniform: the block's waves past the last query
    const bool live = i < M;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    if (live) { x = qry[(int64_t)i * 3 + 0]; y = qry[(int64_t)i * 3 + 1]; z = qry[(int64_t)i * 3 + 2]; }
    const int lane = threadIdx.x & 63;
    const int chunks = (P + SCORE_POSES - 1) / SCORE_POSES;
    for (int c = blockIdx.y; c < chunks; c += gridDim.y) {
        const int end = min((c + 1) * SCORE_POSES, P);
        for (int p = c * SCORE_POSES; p < end; ++p) {              // p is wave-uniform, and so is the address of the pose
            RigidPose T;
#pragma unroll
            for (int a = 0; a < 12; ++a) T.m[a] = poses[(int64_t)p * 12 + a];
            bool hit = false;
            if (live) {
                float px, py, pz;
                pose_apply(T, x, y, z, px, py, pz);                // query frame -> source frame
                u64 cx, cy, cz;
                if (transfer_cell(px, py, pz, ox, oy, oz, inv_h, cx, cy, cz)) hit = transfer_any_candidate(ix, px, py, pz, cx, cy, cz, r2);
            }
            const u64 hits = __ballot(hit);
            if (hits != 0 && lane == 0) atomicAdd(&counts[p], (int)__popcll(hits));
        }
    }
}

PSAM_API int32_t psam_pose_score(const float* src, int32_t N, const void* index_ws, size_t index_ws_bytes, const float* origin, float inv_h, float r2,
                                  const float* qry, int32_t M, const float* poses, int32_t P, int32_t* counts, hipStream_t stream) {
    static const char* const aligned = "index_ws must be 16-byte aligned, src, qry, poses and counts 4-byte aligned";
    static const TransferEntry entry = {"psam_pose_score", "index workspace", aligned, aligned};
    const int32_t st = transfer_check_query(entry, src, N, index_ws, index_ws_bytes, origin, inv_h, r2, qry, M, poses && counts,
                                            (((uintptr_t)poses | (uintptr_t)counts) & 3) == 0);
    if (st != PSAM_OK) return st;
    PSAM_REQUIRE(P > 0 && P <= SCORE_MAX_POSES, PSAM_EINVAL, "psam_pose_score: need 0 < P <= 2^20");
    if (hipMemsetAsync(counts, 0, (size_t)P * sizeof(int32_t), stream) != hipSuccess) {
        (void)hipGetLastError();
        psam_set_error("psam_pose_score: clearing counts failed");
        return PSAM_EINVAL;
    }
    const TransferIndexView ix = transfer_view(src, N, index_ws);
    const int64_t chunks = psam_cdiv(P, SCORE_POSES);
    const dim3 grid((unsigned)psam_cdiv(M, SCORE_THREADS), (unsigned)(chunks < SCORE_MAX_GRID_Y ? chunks : SCORE_MAX_GRID_Y)), block(SCORE_THREADS);
    hipLaunchKernelGGL(align_score_kernel, grid, block, 0, stream, ix, origin[0], origin[1], origin[2], inv_h, r2, qry, (int)M, poses, (int)P,
                       (int*)counts);
    return psam_launch_status("psam_pose_score: launch failed");
}
