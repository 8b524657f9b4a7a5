// The "g8" packed-row format of the f16x3 path, and every way a kernel writes it.  This is the only file that knows the layout.
//
// A row x[0 .. K) with its power-of-two scale s (f16_row_scale of the row maximum) is stored in 32-bit containers: for each group of 8
// consecutive columns, containers 8g .. 8g+3 hold hi = RNE_fp16(s * x) of the eight columns (two per container, the lower column in the
// low half-word) and containers 8g+4 .. 8g+7 hold lo = RNE_fp16(s * x - hi).  Columns K .. kpad32(K) - 1, the rest of the GEMM's 32-k
// slab, are zeros.  tests/g8_reference.py is the host's statement of the same format.
#pragma once
#include "common.h"

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// K rounded up to the 32-k slab of the packed GEMMs: the containers of a packed row
static inline __host__ __device__ int kpad32(int k) { return (k + 31) & ~31; }

#ifdef __HIPCC__
typedef float psam_f32x2 __attribute__((ext_vector_type(2)));
typedef float psam_f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 psam_f16x2 __attribute__((ext_vector_type(2)));

// Two already scaled values -> packed fp16 pairs hi = RNE(xs), lo = RNE(xs - hi); the residual is exact.
__device__ __forceinline__ void g8_split2_scaled(const psam_f32x2 xs, unsigned& hi, unsigned& lo) {
    const psam_f16x2 h = __builtin_convertvector(xs, psam_f16x2);
    const psam_f32x2 r = xs - __builtin_convertvector(h, psam_f32x2);
    hi = __builtin_bit_cast(unsigned, h);
    lo = __builtin_bit_cast(unsigned, __builtin_convertvector(r, psam_f16x2));
}
// (x0, x1) * s (s = power-of-two row scale): the f16x3 operand split
__device__ __forceinline__ void psam_split2_f16(float x0, float x1, float s, unsigned& hi, unsigned& lo) { g8_split2_scaled(psam_f32x2{x0, x1} * s, hi, lo); }

// Row scale of a row held as float4s per lane: g8_absmax4 folds a lane's values, g8_row_scale finishes over the wave (whole wave active).
__device__ __forceinline__ float g8_absmax4(const psam_f32x4 v) { return fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))); }
__device__ __forceinline__ float g8_absmax4(float amax, const psam_f32x4 v) { return fmaxf(fmaxf(amax, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3]))); }
__device__ __forceinline__ float g8_row_scale(float lane_max) { return f16_row_scale(wave_max(lane_max)); }

// The chunk: this lane holds 4 consecutive columns as (h0, l0) (h1, l1), its partner lane ^ DIST the other 4 of the group of 8.  Returns the
// 16-byte word this lane stores at ITS OWN container offset (4 * its float4 index): the lower / even lane (lane & DIST == 0) the hi chunk of
// the group, the upper / odd lane the lo chunk -- so consecutive lanes still write consecutive 16-byte chunks.  One exchange, whole wave active:
// DIST 1 on the DPP path (quad_perm), DIST 32 by v_permlane32_swap, which leaves each half-wave with exactly the words it stores.
// SHFL: the exchange through ds_bpermute (__shfl_xor) instead, for the kernels where the DPP form costs registers: scale_pack_rows_g8_kernel<4>, <8>
// (30 -> 31, 46 -> 47 VGPRs) and interp3_c256_kernel<4> (86 -> 90), whose R independent rows the compiler then schedules less tightly.
template <int DIST, bool SHFL = false>
__device__ __forceinline__ u32x4 g8_chunk_words(unsigned h0, unsigned l0, unsigned h1, unsigned l1, int lane) {
    static_assert(DIST == 1 || DIST == 32, "partner lane: ^ 1 or ^ 32");
    if constexpr (SHFL) {
        const bool upper = lane & DIST;
        const unsigned r0 = __shfl_xor(upper ? h0 : l0, DIST, 64), r1 = __shfl_xor(upper ? h1 : l1, DIST, 64);
        return upper ? u32x4{r0, r1, l0, l1} : u32x4{h0, h1, r0, r1};
    } else if constexpr (DIST == 1) {
        const bool upper = lane & 1;
        const unsigned r0 = (unsigned)dpp_i32<DPP_XOR1>((int)(upper ? h0 : l0)), r1 = (unsigned)dpp_i32<DPP_XOR1>((int)(upper ? h1 : l1));
        return upper ? u32x4{r0, r1, l0, l1} : u32x4{h0, h1, r0, r1};
    } else {
        psam_swap32(h0, l0); psam_swap32(h1, l1);      // lower: (own hi, partner's hi); upper: (partner's lo, own lo)
        return u32x4{h0, h1, l0, l1};
    }
}
template <int DIST, bool SHFL = false>
__device__ __forceinline__ u32x4 g8_chunk(const psam_f32x4 x, float s, int lane) {
    unsigned h0, l0, h1, l1;
    psam_split2_f16(x[0], x[1], s, h0, l0);
    psam_split2_f16(x[2], x[3], s, h1, l1);
    return g8_chunk_words<DIST, SHFL>(h0, l0, h1, l1, lane);
}
template <int DIST>
__device__ __forceinline__ u32x4 g8_chunk_scaled(const psam_f32x2 xs01, const psam_f32x2 xs23, int lane) {
    unsigned h0, l0, h1, l1;
    g8_split2_scaled(xs01, h0, l0);
    g8_split2_scaled(xs23, h1, l1);
    return g8_chunk_words<DIST>(h0, l0, h1, l1, lane);
}

// Half-wave regrouping (transposed GEMM epilogue): a lane of half-wave h holds runs x, y of four columns, 8 columns apart; lane ^ 32 holds the
// runs 4 columns further on.  After the exchange this lane owns one whole group, the (2 gp + h)-th of the 32-column tile: x of both halves is
// the lower half-wave's group, y the upper one's.  A whole group is [hi x 8 | lo x 8] = 32 contiguous bytes: g8_store_group.
struct g8_group { u32x4 hi, lo; };
__device__ __forceinline__ g8_group g8_halfwave_group(const psam_f32x4 x, const psam_f32x4 y, float s) {
    unsigned xh[2], xl[2], yh[2], yl[2];
    psam_split2_f16(x[0], x[1], s, xh[0], xl[0]);
    psam_split2_f16(x[2], x[3], s, xh[1], xl[1]);
    psam_split2_f16(y[0], y[1], s, yh[0], yl[0]);
    psam_split2_f16(y[2], y[3], s, yh[1], yl[1]);
    psam_swap32(xh[0], yh[0]); psam_swap32(xh[1], yh[1]); psam_swap32(xl[0], yl[0]); psam_swap32(xl[1], yl[1]);
    // x = columns 0-3, y = columns 4-7 of the group
    return {u32x4{xh[0], xh[1], yh[0], yh[1]}, u32x4{xl[0], xl[1], yl[0], yl[1]}};
}
// One thread holds the whole group v[0 .. 8): the format's definition.
__device__ __forceinline__ g8_group g8_whole_group(const float (&v)[8], float s) {
    unsigned hi[4], lo[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) psam_split2_f16(v[2 * e], v[2 * e + 1], s, hi[e], lo[e]);
    return {u32x4{hi[0], hi[1], hi[2], hi[3]}, u32x4{lo[0], lo[1], lo[2], lo[3]}};
}
// first: the group's first container
__device__ __forceinline__ void g8_store_group(unsigned* first, const g8_group& g) {
    *reinterpret_cast<u32x4*>(first) = g.hi;
    *reinterpret_cast<u32x4*>(first + 4) = g.lo;
}
// The regrouping and the store in one step, for a kernel whose lanes hold the runs as above (patch_rowln.hip)
__device__ __forceinline__ void g8_store_halfwave_group(unsigned* first, const psam_f32x4 x, const psam_f32x4 y, float s) { g8_store_group(first, g8_halfwave_group(x, y, s)); }

// This lane holds columns 2 * lane and 2 * lane + 1 of row `row` of P (ld containers per row; a group of 8 = 4 lanes): one hi and one lo container.
__device__ __forceinline__ void g8_store_pair(unsigned* P, int64_t row, int ld, int lane, float x0, float x1, float s) {
    unsigned hi, lo;
    psam_split2_f16(x0, x1, s, hi, lo);
    unsigned* o = P + row * ld + (lane >> 2) * 8 + (lane & 3);
    o[0] = hi;
    o[4] = lo;
}
#endif
