// Shared helpers for the gfx950 (CDNA4, wave64) kernels of libpointsam_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#define PSAM_OK 0
#define PSAM_EINVAL (-1)     // bad shape / null pointer / unsupported size
#define PSAM_EALIGN (-2)     // pointer or leading dimension not aligned as the kernel requires
#define PSAM_EWORKSPACE (-3) // workspace too small

#define PSAM_API extern "C" __attribute__((visibility("default")))

// The public header is part of every translation unit: a definition whose signature drifts from its declaration in include/pointsam_hip.h is a
// compile error (C linkage cannot be overloaded), and the structs that cross the ABI exist once.
#pragma GCC visibility push(default)
#include "../../include/pointsam_hip.h"
#pragma GCC visibility pop
#include "knob.h"

void psam_set_error(const char* msg);

#define PSAM_REQUIRE(cond, code, msg)                 \
    do {                                              \
        if (!(cond)) {                                \
            psam_set_error(msg);                      \
            return (code);                            \
        }                                             \
    } while (0)

// Returns 0 or the positive hipError_t of the launch just issued.
static inline int32_t psam_launch_status(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        psam_set_error(what);
        return (int32_t)e;
    }
    return PSAM_OK;
}

// What the calling thread's last call of an entry point launched, for its psam_*_last_* queries: one or two numbers (-1, or B0 for the second, before the
// first launch and after a refused call).  One `static thread_local` record per entry point; host-side bookkeeping only.
template <int32_t B0 = -1>
struct psam_launch_record {
    int32_t a = -1, b = B0;
    void reset() { a = -1; b = B0; }
    // rc: the status of the launch just issued; the numbers are stored only where it succeeded
    int32_t set(int32_t rc, int32_t a_, int32_t b_ = B0) {
        if (rc == PSAM_OK) { a = a_; b = b_; }
        return rc;
    }
    int32_t done(const char* what, int32_t a_, int32_t b_ = B0) { return set(psam_launch_status(what), a_, b_); }
};

// CUs of the current device; 256 (MI355X) where there is none to ask (host-side planning without a GPU).  Asked once per process and translation unit: every
// caller sees the cached count (the devices of one machine are of one type).
static inline int psam_cu_count() {
    static const int cached = [] {
        int ncu = 0, dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0) ncu = 256;
        return ncu;
    }();
    return cached;
}

// > 64 KiB of dynamic LDS must be opted into per kernel AND per device (the attribute lives with the device's code object).  done_mask: the caller's
// `static unsigned long long` (zero at first), one bit per device that has the attribute.  False: no device, or the attribute was refused.
template <typename K>
static inline bool psam_reserve_lds(K kernel, int lds, unsigned long long& done_mask) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    const unsigned long long bit = 1ull << (dev & 63);
    if (__atomic_load_n(&done_mask, __ATOMIC_ACQUIRE) & bit) return true;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) return false;
    __atomic_fetch_or(&done_mask, bit, __ATOMIC_RELEASE);
    return true;
}

static inline int64_t psam_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

#ifdef __HIPCC__
constexpr int WAVE = 64;

// Power-of-two row scale of the f16x3 GEMM: 2^(14 - e), e = floor(log2(row maximum)) clamped below at -112 (scale and its inverse stay
// normal fp32 numbers over the whole finite range: 2^-113 .. 2^126 and 2^-126 .. 2^113); 1 for an
// all-zero / non-finite row (gemm_f16x3.hip).
__device__ __forceinline__ float f16_row_scale(float amax) {
    const unsigned bits = __builtin_bit_cast(unsigned, amax);
    int e = (int)((bits >> 23) & 0xff) - 127;
    if (bits == 0 || e == 128) return 1.f;
    e = e < -112 ? -112 : e;
    return __builtin_bit_cast(float, (unsigned)(127 + 14 - e) << 23);
}

// 1/s for a power-of-two scale s in [2^-126, 2^126] (exact): exponent field 254 - E
__device__ __forceinline__ float inv_pow2(float s) { return __builtin_bit_cast(float, (254u << 23) - __builtin_bit_cast(unsigned, s)); }
// (the operand split and the packed-row format built on these scales: g8_pack.h)

// Reductions on the VALU's data-parallel-primitive path instead of ds_bpermute (an LDS round trip, ~100+ cycles per step, six steps for a
// wave): quad_perm xor 1 / xor 2, row_half_mirror, row_mirror leave every lane of a 16-lane row with the row's result in four
// few-cycle steps.  Whole wave must be active.
template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false); }
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) { return __builtin_bit_cast(float, dpp_i32<CTRL>(__builtin_bit_cast(int, v))); }
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_MIRROR = 0x140;
// Half-wave exchange (v_permlane32_swap): lanes 32-63 of a <-> lanes 0-31 of b.  Whole wave must be active.
__device__ __forceinline__ void psam_swap32(unsigned& a, unsigned& b) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned swap_u32x2 __attribute__((ext_vector_type(2)));
    const swap_u32x2 r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    a = r[0]; b = r[1];
#endif
}
__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, dpp_f32<DPP_XOR1>(v)); v = fmaxf(v, dpp_f32<DPP_XOR2>(v));
    v = fmaxf(v, dpp_f32<DPP_HALF_MIRROR>(v)); v = fmaxf(v, dpp_f32<DPP_MIRROR>(v));
    return v;
}
__device__ __forceinline__ int row16_min(int v) {
    v = min(v, dpp_i32<DPP_XOR1>(v)); v = min(v, dpp_i32<DPP_XOR2>(v));
    v = min(v, dpp_i32<DPP_HALF_MIRROR>(v)); v = min(v, dpp_i32<DPP_MIRROR>(v));
    return v;
}
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_f32<DPP_XOR1>(v); v += dpp_f32<DPP_XOR2>(v);
    v += dpp_f32<DPP_HALF_MIRROR>(v); v += dpp_f32<DPP_MIRROR>(v);
    return v;
}
// Wave reductions: four DPP steps inside the 16-lane rows, then two cross-row exchanges through ds_bpermute (xor 16, xor 32): every lane
// ends up with the result, in a fixed order.  (A variant that combined the rows with v_readlane of lanes 0/16/32/48 was faster still but
// gave run-to-run different LayerNorm statistics in one multi-stream test -- 9 failures in 10 runs against 0 in 10 for this form and for
// the plain six-step shuffle butterfly -- so SGPR read-back of DPP results is not used.)
__device__ __forceinline__ float wave_max(float v) {
    v = row16_max(v);
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float wave_sum(float v) {      // pairs, quads, 8s, 16s inside a row, then rows 16 apart, then 32 apart
    v = row16_sum(v);
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}
// fp64 wave sum by the xor butterfly 32, 16, 8, 4, 2, 1: each step adds the same two values in both lanes and IEEE addition commutes, so all lanes
// end up with the same bits, in an order that is a function of the lane numbers alone (geometry.hip, align.hip).  Whole wave must be active.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ int wave_min_dpp(int v) {
    v = row16_min(v);
    v = min(v, __shfl_xor(v, 16, 64));
    return min(v, __shfl_xor(v, 32, 64));
}
// exact (erf) GELU, as torch.nn.GELU() default
// (Round 4: a branch-free erf -- Abramowitz & Stegun 7.1.26, ~16 VALU instructions against the device library's ~45 with both branches taken --
// changed nothing in the benchmark: 796.6 / 797.6 against 796.7 / 795.9 clouds/s on one box; the GELUs sit in memory-bound passes.  Not kept.)
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }
__device__ __forceinline__ float silu(float x) { return x / (1.0f + __expf(-x)); }

// Squared distance with the oracle's operation order and NO fused multiply-add:
// ((dx*dx) + dy*dy) + dz*dz, every op rounded to fp32 (oracle/tokenizer_oracle.c: dist2).
// HIP's __fmul_rn/__fadd_rn are plain operators (contractable), so contraction is switched off by pragma
// here and by -ffp-contract=off for the whole tokenizer translation unit.
__device__ __forceinline__ float dist2_exact(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    float s = dx * dx;
    const float t = dy * dy;
    s = s + t;
    const float u = dz * dz;
    s = s + u;
    return s;
}

// Experiments builds only: PSAM_ABLATE_REPEAT (bit mask, environment) makes an idempotent kernel launch TWICE -- the throughput lost to the second
// launch is the kernel's exposed time in the pipeline (profiles/r06/r06_refill.txt): 1 = psam_attention_packed, 2 = psam_layernorm (out of place),
// 4 = psam_ln_stats_finalize.
static inline int psam_ablate_repeat() {
#ifdef PSAM_BUILD_EXPERIMENTS
    static psam_knob k_ablate_repeat("PSAM_ABLATE_REPEAT", 0);
    return k_ablate_repeat.get();
#else
    return 0;
#endif
}

// Layout of the caller's arrival-counter block (PSAM_COUNTER_BYTES = 16384 ints, include/pointsam_hip.h), in ints.  Launches that use one block are ordered,
// so the users could share words; they have ranges of their own anyway (a fault in one must not poison the others).
constexpr int PSAM_CNT_GEMM = 0, PSAM_CNT_GEMM_N = 4096;          // split-K GEMM: one word per output tile
constexpr int PSAM_CNT_ATTN = 4096, PSAM_CNT_ATTN_N = 4096;       // key-split attention: one word per (query block, head, batch)
constexpr int PSAM_CNT_ROW = 8192;                                // skinny Linear + LayerNorm: one word
static_assert((PSAM_CNT_ROW + 1) * 4 <= PSAM_COUNTER_BYTES, "counter block layout");
#endif
