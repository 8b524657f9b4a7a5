// Mask proposals ("segment everything"): what comes after the decoder's logits when a cloud is prompted with a grid of points -- threshold the
// candidate masks, score their overlaps, suppress the duplicates, label the points (point_sam_amd/proposals.py).
//
// A mask is a row of W = ceil(N / 64) 64-bit words: bit (n % 64) of word (n / 64) is point n, bits past N are zero.  One wave reads 64 consecutive
// logits coalesced and the ballot of `logit > thr` IS the word, so the fp32 logits are read once and 1 bit per point is kept.  Everything below the
// pack is integer arithmetic on those words (and + popcount), so every result is exact and reproducible:
//   psam_mask_pack           logits [K, N] -> bits [K, W] + the three areas (at thr, thr + off, thr - off: the stability score's counts)
//   psam_mask_valid          the per-candidate filter (area bounds, predicted IoU, stability) -> valid [K]
//   psam_mask_intersections  inter[i, j] = popcount(a_i & b_j), LDS-tiled over rows and over W
//   psam_mask_nms            greedy suppression in a given order: a suppression bit matrix built in parallel, then ONE wave walks it
//   psam_mask_paint          per point the rank of the best kept mask that contains it
// The IoU decision is `inter > thr * union` in fp64: thr has a 24-bit significand and the union is an integer below 2^25 (N <= 2^24), so the
// product has at most 49 significant bits and is exact; a host reference in numpy decides identically.
#include "common.h"

typedef unsigned long long u64;

// ------------------------------------------------------------------------------------------------ pack
constexpr int PACK_THREADS = 1024;      // 16 waves per row: a chunk of 192 rows still puts 3072 waves on the chip
constexpr int PACK_WAVES = PACK_THREADS / WAVE;
constexpr int PACK_UNROLL = 4;          // words in flight per wave

__global__ __launch_bounds__(PACK_THREADS) void mask_pack_kernel(const float* __restrict__ logits, int64_t ld, int N, int W, float thr, float thr_hi,
                                                                float thr_lo, u64* __restrict__ bits, int* __restrict__ area,
                                                                int* __restrict__ area_hi, int* __restrict__ area_lo) {
    __shared__ int s_cnt[3][PACK_WAVES];
    const int row = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* __restrict__ src = logits + (int64_t)row * ld;
    u64* __restrict__ dst = bits + (int64_t)row * W;
    int c = 0, chi = 0, clo = 0;        // wave-uniform: popcounts of ballots
    for (int w0 = wave * PACK_UNROLL; w0 < W; w0 += PACK_WAVES * PACK_UNROLL) {
        float v[PACK_UNROLL];
#pragma unroll
        for (int u = 0; u < PACK_UNROLL; ++u) {
            const int64_t n = (int64_t)(w0 + u) * 64 + lane;
            v[u] = n < N ? src[n] : -__builtin_inff();      // past the row's end: below every threshold (a NaN threshold compares false too)
        }
#pragma unroll
        for (int u = 0; u < PACK_UNROLL; ++u) {
            const int64_t n = (int64_t)(w0 + u) * 64 + lane;
            const bool in = n < N;
            const u64 m = __ballot(in && v[u] > thr), mh = __ballot(in && v[u] > thr_hi), ml = __ballot(in && v[u] > thr_lo);
            if (w0 + u < W) {
                if (lane == 0) dst[w0 + u] = m;
                c += __popcll(m); chi += __popcll(mh); clo += __popcll(ml);
            }
        }
    }
    if (lane == 0) { s_cnt[0][wave] = c; s_cnt[1][wave] = chi; s_cnt[2][wave] = clo; }
    __syncthreads();
    if (threadIdx.x < 3) {
        int s = 0;
        for (int i = 0; i < PACK_WAVES; ++i) s += s_cnt[threadIdx.x][i];
        (threadIdx.x == 0 ? area : threadIdx.x == 1 ? area_hi : area_lo)[row] = s;
    }
}

PSAM_API int32_t psam_mask_pack(const float* logits, int64_t ld, int32_t K, int32_t N, float thr, float off, int32_t dst_row, uint64_t* bits,
                                int32_t* area, int32_t* area_hi, int32_t* area_lo, hipStream_t stream) {
    PSAM_REQUIRE(logits && bits && area && area_hi && area_lo, PSAM_EINVAL, "psam_mask_pack: null pointer");
    PSAM_REQUIRE(K > 0 && N > 0 && ld >= N && dst_row >= 0, PSAM_EINVAL, "psam_mask_pack: need K > 0, N > 0, ld >= N, dst_row >= 0");
    PSAM_REQUIRE(N <= (1 << 24), PSAM_EINVAL, "psam_mask_pack: N above 2^24 (the areas must stay exact as fp32 / in the fp64 IoU test)");
    const int W = (int)psam_cdiv(N, 64);
    const float thr_hi = thr + off, thr_lo = thr - off;      // rounded to fp32, as the reference's np.float32 arithmetic
    hipLaunchKernelGGL(mask_pack_kernel, dim3((unsigned)K), dim3(PACK_THREADS), 0, stream, logits, ld, (int)N, W, thr, thr_hi, thr_lo,
                       (u64*)bits + (int64_t)dst_row * W, area + dst_row, area_hi + dst_row, area_lo + dst_row);
    return psam_launch_status("psam_mask_pack: launch failed");
}

// ------------------------------------------------------------------------------------------------ validity
__global__ void mask_valid_kernel(const int* __restrict__ area, const int* __restrict__ area_hi, const int* __restrict__ area_lo,
                                  const float* __restrict__ score, int K, double max_area, int min_points, float pred_iou_thr, double stab_thr,
                                  unsigned char* __restrict__ valid) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const int a = area[k], hi = area_hi[k], lo = area_lo[k];
    const bool ok = a >= min_points && (double)a < max_area && score[k] >= pred_iou_thr && lo > 0 && (double)hi >= stab_thr * (double)lo;
    valid[k] = ok ? 1 : 0;
}

PSAM_API int32_t psam_mask_valid(const int32_t* area, const int32_t* area_hi, const int32_t* area_lo, const float* score, int32_t K, int32_t N,
                                 int32_t min_points, float max_area_frac, float pred_iou_thr, float stab_thr, uint8_t* valid, hipStream_t stream) {
    PSAM_REQUIRE(area && area_hi && area_lo && score && valid, PSAM_EINVAL, "psam_mask_valid: null pointer");
    PSAM_REQUIRE(K > 0 && N > 0, PSAM_EINVAL, "psam_mask_valid: need K > 0 and N > 0");
    hipLaunchKernelGGL(mask_valid_kernel, dim3((unsigned)psam_cdiv(K, 256)), dim3(256), 0, stream, area, area_hi, area_lo, score, (int)K,
                       (double)max_area_frac * (double)N, (int)min_points, pred_iou_thr, (double)stab_thr, valid);
    return psam_launch_status("psam_mask_valid: launch failed");
}

// ------------------------------------------------------------------------------------------------ intersections
// inter[i, j] = popcount(a_i & b_j).  A workgroup of 256 threads owns a 64 x 64 tile of the output and walks W in steps of 32 words: the 64 rows
// of a and of b are staged in LDS as [row][32 + 1] words (the pad word spreads the b rows of a 16-lane group over all banks; the a rows are a
// broadcast), each thread keeps a 4 x 4 block of counters (a rows 4 ty .. 4 ty + 3, b rows tx + 16 j) and every staged word is used 64 times.
// Per 64-bit pair: two v_and and two accumulating v_bcnt.  `a == b`: only tiles on or above the diagonal are computed, a tile above it
// is also stored as its mirror.
constexpr int IT = 64, IW = 32, ILD = IW + 1;
// Measured (profiles/proposals/README.md): 8 x 4 counters per thread on a 128 x 64 tile need 161 VGPRs, 3 waves per SIMD, and are 25 % slower.  The
// mirrored path at K = 3072 runs 1176 tiles on 1024 resident workgroups (4 per CU): two rounds where 1.15 would do, which is why it takes 0.76 of
// the full matrix's time and not half.  Splitting W over workgroups would fix that at the price of integer atomics and a memset; not done.

__global__ __launch_bounds__(256) void mask_inter_kernel(const u64* __restrict__ a, const u64* __restrict__ b, int Ka, int Kb, int W,
                                                        int* __restrict__ inter, int symmetric) {
    __shared__ u64 sa[IT * ILD], sb[IT * ILD];
    const int bi = blockIdx.y, bj = blockIdx.x;
    const int i0 = bi * IT, j0 = bj * IT;
    if (symmetric && bj < bi) return;                      // under the diagonal: written as the mirror of tile (bj, bi)
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    int acc[4][4] = {};
    for (int w0 = 0; w0 < W; w0 += IW) {
        // stage: thread -> (row = tid / 32 + 8 r, word = tid % 32): 256 B contiguous per row
        const int lw = tid & 31, lr = tid >> 5;
        const bool wok = w0 + lw < W;
#pragma unroll
        for (int r = 0; r < IT / 8; ++r) {
            const int row = lr + 8 * r;
            sa[row * ILD + lw] = (wok && i0 + row < Ka) ? a[(int64_t)(i0 + row) * W + w0 + lw] : 0ull;
            sb[row * ILD + lw] = (wok && j0 + row < Kb) ? b[(int64_t)(j0 + row) * W + w0 + lw] : 0ull;
        }
        __syncthreads();
#pragma unroll 4
        for (int w = 0; w < IW; ++w) {
            u64 av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) av[i] = sa[(ty * 4 + i) * ILD + w];
#pragma unroll
            for (int j = 0; j < 4; ++j) bv[j] = sb[(tx + 16 * j) * ILD + w];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += __popcll(av[i] & bv[j]);
        }
        __syncthreads();
    }
    const bool mirror = symmetric && bj > bi;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gi = i0 + ty * 4 + i, gj = j0 + tx + 16 * j;
            if (gi < Ka && gj < Kb) {
                inter[(int64_t)gi * Kb + gj] = acc[i][j];
                // the mirror's stores are scattered (a column per lane); staging the tile through LDS to store rows measured the same
                // (0.528 against 0.532 ms at K = 3072, W = 512): the kernel's time is its and + popcount loop
                if (mirror) inter[(int64_t)gj * Kb + gi] = acc[i][j];
            }
        }
}

PSAM_API int32_t psam_mask_intersections(const uint64_t* a, const uint64_t* b, int32_t Ka, int32_t Kb, int32_t W, int32_t* inter, hipStream_t stream) {
    PSAM_REQUIRE(a && b && inter, PSAM_EINVAL, "psam_mask_intersections: null pointer");
    PSAM_REQUIRE(Ka > 0 && Kb > 0 && W > 0, PSAM_EINVAL, "psam_mask_intersections: need Ka > 0, Kb > 0, W > 0");
    PSAM_REQUIRE(psam_cdiv(Ka, IT) <= 65535, PSAM_EINVAL, "psam_mask_intersections: Ka above 65535 * 64");
    const int symmetric = (a == b && Ka == Kb) ? 1 : 0;
    hipLaunchKernelGGL(mask_inter_kernel, dim3((unsigned)psam_cdiv(Kb, IT), (unsigned)psam_cdiv(Ka, IT)), dim3(256), 0, stream, (const u64*)a,
                       (const u64*)b, (int)Ka, (int)Kb, (int)W, inter, symmetric);
    return psam_launch_status("psam_mask_intersections: launch failed");
}

// ------------------------------------------------------------------------------------------------ greedy NMS
// Positions are places in `order` (0 = best).  Step 1, parallel: S[p] = the set of positions q > p whose candidate overlaps candidate order[p]
// above the threshold, one bit per position (a wave's ballot is one word); row K of S = the positions whose candidate is invalid.  Step 2, one
// wave: `removed` starts as row K; walking p = 0, 1, ...: a position not removed is kept and ORs S[p] into `removed`.  The rows of S do not depend on the decisions, so the walk loads them
// NMS_PF positions ahead and its serial chain is one cross-lane read and a few ORs per position, with no trip to memory and none to the host.
constexpr int NMS_MAX_K = 16384;        // 4 words of `removed` per lane; inter [K, K] int32 is 1 GiB there
constexpr int NMS_PF = 8;

static inline int64_t nms_words(int K) { return psam_cdiv(K, 64); }

__global__ __launch_bounds__(256) void nms_matrix_kernel(const int* __restrict__ order, const unsigned char* __restrict__ valid,
                                                        const int* __restrict__ area, const int* __restrict__ inter, int K, int KW, double thr,
                                                        u64* __restrict__ S) {
    const int lane = threadIdx.x & 63;
    const int wq = blockIdx.x * 4 + (threadIdx.x >> 6), p = blockIdx.y;
    if (wq >= KW) return;                                  // wave-uniform
    const int q = wq * 64 + lane;
    if (p == K) {                                          // the walk's start: invalid (or out of range) candidates, and the positions past K
        bool bad = true;
        if (q < K) { const int c = order[q]; bad = (unsigned)c >= (unsigned)K || valid[c] == 0; }
        const u64 mb = __ballot(bad);
        if (lane == 0) S[(int64_t)K * KW + wq] = mb;
        return;
    }
    bool hit = false;
    const int i = order[p];
    if (q > p && q < K && (unsigned)i < (unsigned)K) {
        const int j = order[q];
        if ((unsigned)j < (unsigned)K) {
            const int in = inter[(int64_t)i * K + j];
            hit = (double)in > thr * (double)((int64_t)area[i] + area[j] - in);
        }
    }
    const u64 m = __ballot(hit);
    if (lane == 0) S[(int64_t)p * KW + wq] = m;
}

template <int NW>
__global__ __launch_bounds__(64) void nms_walk_kernel(const int* __restrict__ order, const u64* __restrict__ S, int K, int KW,
                                                     unsigned char* __restrict__ keep) {
    const int lane = threadIdx.x;
    u64 removed[NW];      // lane holds words s * 64 + lane
#pragma unroll
    for (int s = 0; s < NW; ++s) removed[s] = s * 64 + lane < KW ? S[(int64_t)K * KW + s * 64 + lane] : ~0ull;
    for (int p0 = 0; p0 < K; p0 += NMS_PF) {
        u64 rows[NMS_PF][NW];
        int cand[NMS_PF];
#pragma unroll
        for (int r = 0; r < NMS_PF; ++r) {
            const int p = p0 + r;
            cand[r] = p < K ? order[p] : -1;
#pragma unroll
            for (int s = 0; s < NW; ++s) {
                const int w = s * 64 + lane;
                rows[r][s] = (p < K && w < KW) ? S[(int64_t)p * KW + w] : 0ull;
            }
        }
#pragma unroll
        for (int r = 0; r < NMS_PF; ++r) {
            const int p = p0 + r;
            if (p >= K) break;                             // uniform
            const int wp = p >> 6;
            u64 mine = removed[0];
#pragma unroll
            for (int s = 1; s < NW; ++s) mine = (wp >> 6) == s ? removed[s] : mine;
            const u64 word = __shfl(mine, wp & 63, 64);
            const bool kept = ((word >> (p & 63)) & 1ull) == 0;      // uniform
            if (kept) {
#pragma unroll
                for (int s = 0; s < NW; ++s) removed[s] |= rows[r][s];
            }
            if (lane == 0 && (unsigned)cand[r] < (unsigned)K) keep[cand[r]] = kept ? 1 : 0;
        }
    }
}

PSAM_API size_t psam_mask_nms_workspace_bytes(int32_t K) {
    if (K <= 0 || K > NMS_MAX_K) return 0;
    return ((size_t)K + 1) * (size_t)nms_words(K) * sizeof(u64);
}

PSAM_API int32_t psam_mask_nms(const int32_t* order, const uint8_t* valid, const int32_t* area, const int32_t* inter, int32_t K, float iou_thr,
                               uint8_t* keep, void* ws, size_t ws_bytes, hipStream_t stream) {
    PSAM_REQUIRE(order && valid && area && inter && keep && ws, PSAM_EINVAL, "psam_mask_nms: null pointer");
    PSAM_REQUIRE(K > 0 && K <= NMS_MAX_K, PSAM_EINVAL, "psam_mask_nms: need 0 < K <= 16384");
    PSAM_REQUIRE(ws_bytes >= psam_mask_nms_workspace_bytes(K), PSAM_EWORKSPACE, "psam_mask_nms: workspace too small (psam_mask_nms_workspace_bytes)");
    PSAM_REQUIRE(((uintptr_t)ws & 7) == 0, PSAM_EALIGN, "psam_mask_nms: workspace must be 8-byte aligned");
    const int KW = (int)nms_words(K);
    u64* S = (u64*)ws;
    hipLaunchKernelGGL(nms_matrix_kernel, dim3((unsigned)psam_cdiv(KW, 4), (unsigned)K + 1), dim3(256), 0, stream, order, valid, area, inter, (int)K, KW,
                       (double)iou_thr, S);
    int32_t st = psam_launch_status("psam_mask_nms: matrix launch failed");
    if (st != PSAM_OK) return st;
    if (KW <= 64) hipLaunchKernelGGL(nms_walk_kernel<1>, dim3(1), dim3(64), 0, stream, order, (const u64*)S, (int)K, KW, keep);
    else if (KW <= 128) hipLaunchKernelGGL(nms_walk_kernel<2>, dim3(1), dim3(64), 0, stream, order, (const u64*)S, (int)K, KW, keep);
    else hipLaunchKernelGGL(nms_walk_kernel<4>, dim3(1), dim3(64), 0, stream, order, (const u64*)S, (int)K, KW, keep);
    return psam_launch_status("psam_mask_nms: walk launch failed");
}

// ------------------------------------------------------------------------------------------------ paint
// labels[n] = rank (0 = best) of the first kept mask, in `order`, that contains point n; -1 if none.  Step 1 (one workgroup): the kept candidates
// in order -> ws = [count, candidate of rank 0, of rank 1, ...].  Step 2: one wave per word of 64 points; the word of every kept mask is a
// wave-uniform load, four in flight, until every lane has its label.
constexpr int RANK_THREADS = 1024;

__global__ __launch_bounds__(RANK_THREADS) void paint_rank_kernel(const int* __restrict__ order, const unsigned char* __restrict__ keep, int K,
                                                                 int* __restrict__ ws) {
    __shared__ int s_cnt[RANK_THREADS];
    const int tid = threadIdx.x, per = (K + RANK_THREADS - 1) / RANK_THREADS;
    const int lo = min(tid * per, K), hi = min(lo + per, K);
    int c = 0;
    for (int p = lo; p < hi; ++p) { const int k = order[p]; c += ((unsigned)k < (unsigned)K && keep[k]) ? 1 : 0; }
    s_cnt[tid] = c;
    __syncthreads();
    if (tid == 0) {      // exclusive scan of 1024 small counts: a few microseconds, once per cloud
        int run = 0;
        for (int t = 0; t < RANK_THREADS; ++t) { const int v = s_cnt[t]; s_cnt[t] = run; run += v; }
        ws[0] = run;
    }
    __syncthreads();
    int r = s_cnt[tid];
    for (int p = lo; p < hi; ++p) { const int k = order[p]; if ((unsigned)k < (unsigned)K && keep[k]) ws[1 + r++] = k; }
}

__global__ __launch_bounds__(256) void paint_kernel(const u64* __restrict__ bits, const int* __restrict__ ws, int N, int W, int* __restrict__ labels) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= W) return;                                    // wave-uniform
    const int count = ws[0];
    const int* __restrict__ list = ws + 1;
    int label = -1;
    for (int r0 = 0; r0 < count; r0 += 4) {
        u64 word[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) word[u] = r0 + u < count ? bits[(int64_t)list[r0 + u] * W + w] : 0ull;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (label < 0 && ((word[u] >> lane) & 1ull)) label = r0 + u;
        if (__ballot(label < 0) == 0ull) break;
    }
    const int64_t n = (int64_t)w * 64 + lane;
    if (n < N) labels[n] = label;
}

PSAM_API size_t psam_mask_paint_workspace_bytes(int32_t K) { return K > 0 ? ((size_t)K + 1) * sizeof(int32_t) : 0; }

PSAM_API int32_t psam_mask_paint(const uint64_t* bits, const int32_t* order, const uint8_t* keep, int32_t K, int32_t N, int32_t* labels, void* ws,
                                 size_t ws_bytes, hipStream_t stream) {
    PSAM_REQUIRE(bits && order && keep && labels && ws, PSAM_EINVAL, "psam_mask_paint: null pointer");
    PSAM_REQUIRE(K > 0 && N > 0, PSAM_EINVAL, "psam_mask_paint: need K > 0 and N > 0");
    PSAM_REQUIRE(ws_bytes >= psam_mask_paint_workspace_bytes(K), PSAM_EWORKSPACE, "psam_mask_paint: workspace too small (psam_mask_paint_workspace_bytes)");
    PSAM_REQUIRE(((uintptr_t)ws & 3) == 0, PSAM_EALIGN, "psam_mask_paint: workspace must be 4-byte aligned");
    const int W = (int)psam_cdiv(N, 64);
    hipLaunchKernelGGL(paint_rank_kernel, dim3(1), dim3(RANK_THREADS), 0, stream, order, keep, (int)K, (int*)ws);
    int32_t st = psam_launch_status("psam_mask_paint: rank launch failed");
    if (st != PSAM_OK) return st;
    hipLaunchKernelGGL(paint_kernel, dim3((unsigned)psam_cdiv(W, 4)), dim3(256), 0, stream, (const u64*)bits, (const int*)ws, (int)N, W, labels);
    return psam_launch_status("psam_mask_paint: launch failed");
}
