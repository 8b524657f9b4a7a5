// Linear (K = 128 -> N = 512) -> LayerNorm -> GELU -> g8-packed rows in ONE kernel: the second half of the mini-PointNet (PatchEncoder's per-row half of
// conv2.0, conv2.1 and its GELU; common.py:493-496) without the [rows, 512] fp32 activation between a GEMM and a LayerNorm pass.
//
//   y[r, :]   = (X[r, :128] . W^T) / (sx[r] sw[:]) + rowbias[r / rowgroup, :]         f16x3: hi*lo + lo*hi + hi*hi on v_mfma_f32_32x32x16_f16, fp32 accumulation,
//                                                                                       the term and k order of gemm_f16x3p.hip, un-scaled as its epilogues do
//   out[r, :] = g8( gelu_erf( (y - mean_r) rstd_r gamma + beta ), s ),  rs[r] = s = f16_row_scale(bound)      bound >= max |gamma| sqrt(512) + max |beta|
//
// K = 128 makes the whole weight a register operand.  A workgroup of eight waves owns 64 rows x 512 columns; wave w owns columns 64 w .. 64 w + 63 of all 64 rows
// (2 x 2 accumulator tiles) and keeps its 64 x 128 slice of W, hi and lo planes, in 128 registers for the life of the workgroup: W never passes through LDS.
// The kernel is persistent: workgroup i takes the 64-row blocks i, i + grid, ...; there is no counter and no waiting on another workgroup.
//   * The 64 packed input rows (32 KiB) of a block arrive by LDS-DMA, in the slab layout and chunk swizzle of gemm_f16x3p.hip (four 32-k slabs of 64 rows x
//     128 B, chunk c of row r at position c ^ ((r >> 1) & 7)).  Two stages: the rows of the next block are requested before the MFMAs of this one and are
//     waited for (vmcnt(0)) before the block's second barrier, which publishes them; the stage they overwrite was last read before the previous block's barriers.
//   * The bias rows of a block (one per 32-row tile: rowgroup % 32 == 0) are fetched a block ahead, a column per thread, and published through LDS by the same
//     barrier; the column constants (1 / weight scale, gamma, beta) are put into LDS once.  The epilogue reads no global memory but the rows' scales.
//   * MFMA operands are swapped as in gemm_epilogue_t.h (D = W_frag x A_frag^T): a lane holds runs of four consecutive columns of ONE output row, so LayerNorm,
//     GELU, the hi / lo split and the g8 groups are register work with one v_permlane32_swap exchange per packed register.
//   * Row statistics are two-pass (mean, then centred squares): in-lane sums in column order, the lane pair, then the eight waves through 4 KiB of LDS in wave
//     order -- the order of gemm_store_tile_t_rowln, one exchange and one barrier per statistic, the same bits on every run.
#include "g8_pack.h"
#include "gemm_f16x3p_args.h"
#include "gemm_epilogue_t.h"

namespace {
struct RowLnArgs {
    const unsigned char* X; const unsigned char* W;      // g8-packed rows: [rows, ldx] and [512, ldw] containers
    const float* sx; const float* sw;                    // their row scales
    const float* rowbias; const float* gamma; const float* beta;
    unsigned* out; float* rs;
    int64_t ldx, ldw, ldrb, ldo;
    int rowgroup, nblocks;
    float eps, bound;
};

constexpr int RL_ROWS = 64, RL_K = 128, RL_N = 512, RL_WAVES = 8;
constexpr int RL_ROWB = 128;                             // bytes per row per 32-k slab
constexpr int RL_SLAB = RL_ROWS * RL_ROWB;               // 8 KiB
constexpr int RL_STAGE = (RL_K / 32) * RL_SLAB;          // 32 KiB: the packed rows of one block

__device__ __forceinline__ void rl_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__global__ __launch_bounds__(64 * RL_WAVES) void linear128_ln_gelu_pack_kernel(const RowLnArgs p) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) unsigned char stage_mem[2 * RL_STAGE];
    __shared__ float red[2 * RL_WAVES * RL_ROWS];        // the waves' partial sums, partial centred squares
    __shared__ __attribute__((aligned(16))) float cst[3 * RL_N];
    __shared__ __attribute__((aligned(16))) float rbs[2 * 2 * RL_N];      // [block parity][32-row tile]: the tile's bias row
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col_base = wave * 64;

    // ---- LDS-DMA of a block's rows: wave w moves rows 8 w .. 8 w + 7 of each of the four slabs (1 KiB pieces); lane -> (row 8 w + lane / 8, slot lane % 8),
    // which receives chunk slot ^ swz(row) (the DMA writes LDS linearly, so the swizzle is applied to the source address)
    const int drow = wave * 8 + (lane >> 3);
    const int dvoff = (int)(drow * p.ldx * 4) + (((lane & 7) ^ ((drow >> 1) & 7)) << 4);
    auto issue = [&](int blk, int st) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(p.X + (int64_t)blk * RL_ROWS * p.ldx * 4), 0, 0x7fffffff, 0x00020000);
#pragma unroll
        for (int s = 0; s < RL_K / 32; ++s) P_DMA16(rs, stage_mem + st * RL_STAGE + s * RL_SLAB + wave * 1024, dvoff, s * RL_ROWB);
    };
    int blk = blockIdx.x, st = 0;
    issue(blk, 0);

    // ---- this wave's slice of W: column tile j, k16 step ks, plane q (hi | lo) -> row col_base + 32 j + r32, group 2 ks + h
    pf16x8 fw[2][8][2];
    {
        const unsigned char* wl = p.W + (int64_t)(col_base + (lane & 31)) * p.ldw * 4 + (lane >> 5) * 32;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int ks = 0; ks < 8; ++ks)
#pragma unroll
                for (int q = 0; q < 2; ++q) fw[j][ks][q] = *reinterpret_cast<const pf16x8*>(wl + (int64_t)j * 32 * p.ldw * 4 + ks * 64 + q * 16);
    }
    const float so = f16_row_scale(p.bound);
    const float inv_n = 1.0f / (float)RL_N;
    float* red2 = red + RL_WAVES * RL_ROWS;
    // the column constants, read from LDS in every block: 1 / scale of the weight's rows | gamma | beta
    cst[tid] = inv_pow2(p.sw[tid]); cst[RL_N + tid] = p.gamma[tid]; cst[2 * RL_N + tid] = p.beta[tid];
    // bias rows of a block, one per 32-row tile (rowgroup % 32 == 0), a column per thread
    auto bias_fetch = [&](int b, float (&v)[2]) {
#pragma unroll
        for (int i = 0; i < 2; ++i) v[i] = p.rowbias[(int64_t)((b * RL_ROWS + i * 32) / p.rowgroup) * p.ldrb + tid];
    };
    {
        float v[2];
        bias_fetch(blk, v);
        rbs[tid] = v[0]; rbs[RL_N + tid] = v[1];
    }

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    rl_barrier();
    for (; blk < p.nblocks; blk += gridDim.x, st ^= 1) {
        const bool has_next = blk + (int)gridDim.x < p.nblocks;
        if (has_next) issue(blk + gridDim.x, st ^ 1);
        const int64_t row0 = (int64_t)blk * RL_ROWS;
        const unsigned char* sa = stage_mem + st * RL_STAGE;
        if (wave == 0) p.rs[row0 + lane] = so;      // the rows' common scale
        const float sxv = p.sx[row0 + lane];         // the scale of row `lane` of the block; the lane's own two rows are fetched from it after the MFMAs
        // Lane-dependent addresses are derived per block from a copy of the lane number the compiler cannot see through, here and after the MFMAs: hoisted
        // out of the loop they stay live through the whole block, beside 128 weight and 64 accumulator registers, and push weights into scratch.
        int lf = lane;
        asm volatile("" : "+v"(lf));
        // fragment offsets inside a slab: row r32 of a 32-row tile, chunk 4 s + 2 h + q (s = k16 step of the slab)
        int fa_off[2][2];
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int q = 0; q < 2; ++q) fa_off[s][q] = (lf & 31) * RL_ROWB + (((4 * s + 2 * (lf >> 5) + q) ^ ((lf >> 1) & 7)) << 4);
        // ---- the products: per k16 step the terms hi*lo, lo*hi, hi*hi
        pf32x16 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        // (one step's fragments at a time -- the fences keep the scheduler from hoisting later steps' reads over the 128 weight registers; the SIMD's other
        // wave has MFMAs to issue while this one waits for its reads)
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            pf16x8 fa[2][2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int q = 0; q < 2; ++q) fa[i][q] = *reinterpret_cast<const pf16x8*>(sa + (ks >> 1) * RL_SLAB + i * 32 * RL_ROWB + fa_off[ks & 1][q]);
            constexpr int PA[3] = {0, 1, 0}, PW[3] = {1, 0, 0};
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fw[j][ks][PW[t]], fa[i][PA[t]], acc[i][j], 0, 0, 0);
            ept_fence();
        }
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int r32 = ln & 31, h = ln >> 5;
        const int ccol = col_base + 4 * h;      // run n of this lane (tile n / 4, run n % 4) starts at column ccol + 8 n
        // ---- pass A: the pre-LayerNorm values in place, row sums.  acc[i][j][4 g + e] = y[row0 + 32 i + r32][col_base + 32 j + 8 g + 4 h + e]
        // (column constants and bias rows come from LDS, two runs per fence: unfenced, the scheduler requests all 24 vectors at once)
        float nb[2];
        bias_fetch(has_next ? blk + gridDim.x : blk, nb);      // the next block's bias rows: in flight under passes A and B, into LDS before the second barrier
        const float rsq[2] = {inv_pow2(__shfl(sxv, r32, 64)), inv_pow2(__shfl(sxv, 32 + r32, 64))};
        float sum[2] = {0.f, 0.f};
        const float* rbl = rbs + st * 2 * RL_N + ccol;
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            const int j = n >> 2, g = n & 3;
            if ((n & 1) == 0) ept_fence();
            const ep_f32x4 isw = ep_load4(cst + ccol + 8 * n), rb[2] = {ep_load4(rbl + 8 * n), ep_load4(rbl + RL_N + 8 * n)};
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float a = (acc[i][j][4 * g + e] * rsq[i]) * isw[e] + rb[i][e];      // both scales are powers of two: one rounding
                    acc[i][j][4 * g + e] = a;
                    sum[i] += a;
                }
        }
        float mean[2], rstd[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float a = sum[i], b = sum[i];
            ept_swap32f(a, b);
            sum[i] = h == 0 ? a + b : b + a;                     // lower half's partial + upper half's, in both halves
            // (both halves store the same bits: a store under `h == 0` would be a branch, and the compiler sinks the arithmetic of the second row tile
            // below the first one's branch, keeping every bias row and scale it loaded alive until then)
            red[wave * RL_ROWS + i * 32 + r32] = sum[i];
        }
        rl_barrier();
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < RL_WAVES; ++w) t += red[w * RL_ROWS + i * 32 + r32];
            mean[i] = t * inv_n;
        }
        // ---- pass B: centred squares
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float q = 0.f;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                ept_fence();      // (or the scheduler takes all 64 differences first)
#pragma unroll
                for (int r = 0; r < 16; ++r) { const float d = acc[i][j][r] - mean[i]; q = __builtin_fmaf(d, d, q); }
            }
            float a = q, b = q;
            ept_swap32f(a, b);
            q = h == 0 ? a + b : b + a;
            red2[wave * RL_ROWS + i * 32 + r32] = q;
        }
        rbs[(st ^ 1) * 2 * RL_N + tid] = nb[0]; rbs[(st ^ 1) * 2 * RL_N + RL_N + tid] = nb[1];      // (last read in the previous block's pass A)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // this wave's pieces of the next block's rows have landed; the barrier publishes everyone's
        rl_barrier();
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < RL_WAVES; ++w) t += red2[w * RL_ROWS + i * 32 + r32];
            rstd[i] = 1.0f / sqrtf(t * inv_n + p.eps);
        }
        // ---- pass C: normalise, GELU, pack, store.  Runs (2 gp, 2 gp + 1) of the two half-waves -> column group 2 gp + h of the tile in this lane
        unsigned* ob = p.out + row0 * p.ldo + col_base + 8 * h;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int gp = 0; gp < 2; ++gp) {
                const float* gb = cst + RL_N + ccol + j * 32 + 16 * gp;
                const ep_f32x4 gm0 = ep_load4(gb), gm1 = ep_load4(gb + 8), bt0 = ep_load4(gb + RL_N), bt1 = ep_load4(gb + RL_N + 8);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    ep_f32x4 v0, v1;
                    ept_fence();      // one run of four at a time: the erf temporaries of more do not fit beside the weight registers
#pragma unroll
                    for (int e = 0; e < 4; ++e) v0[e] = gelu_erf(__builtin_fmaf((acc[i][j][8 * gp + e] - mean[i]) * rstd[i], gm0[e], bt0[e]));
                    ept_fence();
#pragma unroll
                    for (int e = 0; e < 4; ++e) v1[e] = gelu_erf(__builtin_fmaf((acc[i][j][8 * gp + 4 + e] - mean[i]) * rstd[i], gm1[e], bt1[e]));
                    g8_store_halfwave_group(ob + (int64_t)(i * 32 + r32) * p.ldo + j * 32 + 16 * gp, v0, v1, so);
                }
            }
    }
}
}  // namespace

PSAM_API int32_t psam_linear128_ln_gelu_pack(const void* x, int64_t ldx, const float* x_scale, const void* w, int64_t ldw, const float* w_scale, const float* rowbias,
                                             int64_t ldrb, int32_t rowgroup, const float* gamma, const float* beta, float eps, float bound, int64_t rows, int32_t h1,
                                             void* out, int64_t ldo, float* out_scale, hipStream_t stream) {
#define WHO "psam_linear128_ln_gelu_pack"
    PSAM_REQUIRE(x && x_scale && w && w_scale && rowbias && gamma && beta && out && out_scale, PSAM_EINVAL, WHO ": null pointer");
    PSAM_REQUIRE(h1 == RL_N, PSAM_EINVAL, WHO ": the output rows must have 512 columns");
    PSAM_REQUIRE(rows > 0 && rows % RL_ROWS == 0 && rows < ((int64_t)1 << 31), PSAM_EINVAL, WHO ": rows must be a positive multiple of 64 below 2^31");
    PSAM_REQUIRE(rowgroup > 0 && rowgroup % 32 == 0 && ldx >= RL_K && ldw >= RL_K && ldrb >= RL_N && ldo >= RL_N && ldx * 4 * RL_ROWS < ((int64_t)1 << 31), PSAM_EINVAL,
                 WHO ": bad shape (packed inputs of 128 containers per row, bias and output rows of 512, a bias row per multiple of 32 rows)");
    PSAM_REQUIRE(((ldx | ldw | ldo) & 7) == 0 && (((uintptr_t)x | (uintptr_t)w | (uintptr_t)out) & 31) == 0, PSAM_EALIGN, WHO ": packed rows must be 32-byte aligned");
    PSAM_REQUIRE((ldrb & 3) == 0 && (((uintptr_t)rowbias | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)w_scale) & 15) == 0, PSAM_EALIGN,
                 WHO ": bias rows, gamma, beta and the weight's scales must be 16-byte aligned");
    RowLnArgs p;
    p.X = (const unsigned char*)x; p.W = (const unsigned char*)w; p.sx = x_scale; p.sw = w_scale; p.rowbias = rowbias; p.gamma = gamma; p.beta = beta;
    p.out = (unsigned*)out; p.rs = out_scale; p.ldx = ldx; p.ldw = ldw; p.ldrb = ldrb; p.ldo = ldo; p.rowgroup = rowgroup; p.nblocks = (int)(rows / RL_ROWS);
    p.eps = eps; p.bound = bound;
    // one 512-thread workgroup fits a CU at a time (256 registers per wave); two per CU in the grid halve what the last workgroups leave idle
    const int grid = p.nblocks < 2 * psam_cu_count() ? p.nblocks : 2 * psam_cu_count();
    hipLaunchKernelGGL(linear128_ln_gelu_pack_kernel, dim3((unsigned)grid), dim3(64 * RL_WAVES), 0, stream, p);
    return psam_launch_status(WHO ": launch failed");
#undef WHO
}
