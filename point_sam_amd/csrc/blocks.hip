// The coarse C-ABI entry points: psam_eva_block, psam_eva_gelu_block, psam_patch_encoder, psam_upscale_masks and psam_twoway_decoder, each with a
// *_prepare (packs the stage's weights ONCE into a device blob and fills a host plan) and the sizes of that blob and of a call's workspace.
// Host code only; every kernel is another entry point of this library.
//
// Every buffer layout is written ONCE, as a function that walks a Carve and fills a struct of pointers: *_prepared_bytes / *_ws_bytes walk it on a
// null base and report where it ends, *_prepare / the run walk it on the caller's buffer.  A size and its carve cannot disagree.
//
// psam_eva_block: ONE EVA02 (SwiGLU) transformer block of the patch encoder -- timm's block as the reference calls it
// (pc_sam/model/pc_encoder.py:138-139: x = block(x), no rope):  x += proj(SDPA(q, k, v)(LN1 x));  x += fc2(LN(SiLU(fc1_g h) * fc1_x h)), h = LN2 x.
//
// psam_eva_block_prepare packs a block's weights ONCE (what the Python host did in PointCloudSAM._pack): q|k|v concatenated, fc1_g / fc1_x
// interleaved in 32-row blocks, fc2 pre-multiplied by the inner LayerNorm's gamma (the LayerNorm folded into the GEMM), every matrix split
// into g8-packed hi|lo fp16 with power-of-two row scales, and the a-priori bounds of the packed hand-overs.  psam_eva_block then runs the
// block as eight launches with nothing in between -- LayerNorm (packed output + per-row bound) | qkv GEMM (packed q|k|v) | attention on
// packed operands | projection + residual | LayerNorm | fc1 (SwiGLU gate, packed output, LayerNorm partials) | partial merge | fc2 with the
// folded LayerNorm + residual -- so that a caller in any language drives the dominant 83 % of the path's FLOPs with one call per layer.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <initializer_list>
#ifdef PSAM_BUILD_EXPERIMENTS
#include <map>
#include <mutex>
#endif
#include <string>
#include <utility>
#include <vector>
#include "g8_pack.h"     // kpad32; brings in common.h and with it include/pointsam_hip.h

namespace {
constexpr int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

struct Carve {      // bump allocator over a caller-provided buffer; on a null base it only counts (`off` is then the size of the layout it walked)
    char* base; int64_t off = 0;
    explicit Carve(void* p) : base(static_cast<char*>(p)) {}
    template <typename T> T* take(int64_t count) { T* r = base ? reinterpret_cast<T*>(base + off) : nullptr; off += align256(count * (int64_t)sizeof(T)); return r; }
    int64_t offset_of(const void* p) const { return static_cast<const char*>(p) - base; }
};
template <typename F> size_t carved_bytes(F&& layout) { Carve cv(nullptr); layout(cv); return (size_t)cv.off; }      // the size of a layout

// A weight [rows, K] as the packed-operand GEMMs read it: g8-packed hi|lo fp16 rows (kpad32(K) floats each) and their power-of-two row scales
struct Packed { float* w; float* s; };
Packed take_packed(Carve& cv, int64_t rows, int K) { float* w = cv.take<float>(rows * kpad32(K)); return {w, cv.take<float>(rows)}; }
void put_offsets(const Carve& cv, const Packed& p, int64_t* o_w, int64_t* o_s) { *o_w = cv.offset_of(p.w); *o_s = cv.offset_of(p.s); }

int32_t fail(const char* who, const char* what) { psam_set_error((std::string(who) + ": " + what).c_str()); return PSAM_EINVAL; }

// Row scales, then the g8 pack, of one weight [rows, K] (row stride ldw, device) into `dst`; asynchronous on `stream`
int32_t pack_weight(const char* who, const float* w, int64_t ldw, int rows, int K, const Packed& dst, hipStream_t stream) {
    if (!w) return fail(who, "null weight pointer");
    int32_t rc = psam_row_scale_f16(w, ldw, rows, K, dst.s, stream);
    if (!rc) rc = psam_pack_rows_f16x2_g8(w, ldw, dst.s, rows, K, dst.w, kpad32(K), stream);
    return rc;
}
int32_t packing_done(const char* who, int32_t rc, hipStream_t stream) {      // the end of every _prepare: the blob is complete when it returns
    if (!rc && hipStreamSynchronize(stream) != hipSuccess) rc = fail(who, "packing failed");
    return rc;
}

// n floats of a device tensor on the host (empty when the copy fails)
std::vector<float> fetch(const float* dev, int64_t n) {
    std::vector<float> h((size_t)n);
    return hipMemcpy(h.data(), dev, (size_t)n * 4, hipMemcpyDeviceToHost) == hipSuccess ? h : std::vector<float>();
}
#define FETCH(who, name, dev, n) std::vector<float> name = fetch(dev, n); PSAM_REQUIRE((int64_t)name.size() == (int64_t)(n), PSAM_EINVAL, who ": cannot read a weight tensor")

double row_norm(const float* w, int k) {
    double s = 0.0;
    for (int i = 0; i < k; ++i) s += (double)w[i] * (double)w[i];
    return std::sqrt(s);
}

// One nn.Linear y [M, N] = act(x W^T + b), x [M, K] and y dense: the weight as the state dict holds it (row stride ldw) and, where a _prepare packed it,
// its packed form
struct Lin { const float* w; int64_t ldw; const float* b; const float* packed; const float* scales; int N, K; };

// Up to PSAM_SKINNY_MAX_JOBS Linears for ONE launch of psam_linear_skinny_multi / psam_linear_rows_multi (ldy 0: the rows of y are dense)
struct Job { const Lin* l; const float* x; const float* xadd; float* y; int64_t ldy = 0; };
psam_skinny_jobs_t skinny_jobs(std::initializer_list<Job> js) {
    psam_skinny_jobs_t jobs;
    std::memset(&jobs, 0, sizeof(jobs));
    for (const Job& j : js) {
        psam_skinny_job_t& o = jobs.job[jobs.n++];
        o.x = j.x; o.xadd = j.xadd; o.W = j.l->w; o.bias = j.l->b; o.y = j.y; o.ldy = j.ldy ? j.ldy : j.l->N; o.N = j.l->N;
    }
    return jobs;
}

// A Linear on a few hundred to ~2000 rows (one or two clouds' patch tokens): the exact-fp32 32 x 64-tile kernel (psam_linear_rows_multi) beats the
// packing pass + packed-operand GEMM there (5-6 us against 5 + 8-10 us: tiles of 128 rows leave a handful of workgroups, all latency).
// PSAM_ROWS_MULTI=0 switches it off (A/B).
// The choice is made from the rows of ONE cloud (its G patch tokens), never from the batch: a cloud's results must not depend on how many clouds share
// the launch (bit-exact batch independence, tests/test_gpu_e2e.py::test_batch_independence_across_the_row_kernel_threshold).
bool rows_multi_fits(int64_t rows_per_cloud, int K) {
    static psam_knob k_rows_multi("PSAM_ROWS_MULTI", 1);
    return k_rows_multi.get() != 0 && rows_per_cloud <= 2048 && (K & 15) == 0;
}

// The host's choice of kernel for one Linear (point_sam_amd/ops.py linear).  cloud_rows > 0: the M rows are the patch tokens of whole clouds, cloud_rows
// each, and the exact-fp32 row kernel takes them where it fits (without an activation: skinny_jobs sets none); 0: no row kernel (the two-way operator
// sequence).  Then: >= 256 rows and a packed weight -- scale + pack the rows into pack_buf / scale_buf, packed-operand "f16x3" GEMM; <= 64 rows --
// psam_linear_skinny; otherwise psam_linear.
int32_t host_linear(const Lin& l, const float* x, int64_t M, float* y, int act, int64_t cloud_rows, float* pack_buf, float* scale_buf, hipStream_t stream) {
    if (cloud_rows > 0 && act == 0 && rows_multi_fits(cloud_rows, l.K)) {
        const psam_skinny_jobs_t jobs = skinny_jobs({{&l, x, nullptr, y}});
        return psam_linear_rows_multi(&jobs, l.K, l.K, 1, 1, l.ldw, M, l.K, stream);
    }
    if (M >= 256 && l.packed) {
        const int kp = kpad32(l.K);
        int32_t rc = psam_scale_pack_rows_g8(x, l.K, (int32_t)M, l.K, pack_buf, kp, scale_buf, stream);
        if (rc) return rc;
        return psam_gemm_f16x3p_ex(pack_buf, kp, scale_buf, l.packed, kp, l.scales, y, l.N, l.b, nullptr, 0, nullptr, 0, 0, (int32_t)M, l.N, kp, 1.f, act, nullptr, stream);
    }
    if (M <= 64 && (l.K & 15) == 0) return psam_linear_skinny(x, l.K, l.w, l.ldw, l.b, nullptr, 0, y, l.N, (int32_t)M, l.N, l.K, act, stream);
    return psam_linear(x, l.K, l.w, l.ldw, l.b, nullptr, 0, y, l.N, (int32_t)M, l.N, l.K, act, stream);
}

inline const float* at(const void* prepared, int64_t off) { return reinterpret_cast<const float*>(static_cast<const char*>(prepared) + off); }
}  // namespace

// ---- psam_eva_block
namespace {
struct EvaPrepared { Packed qkv; float* bqkv; Packed proj; Packed w1; float* b1; Packed w2g; float *lnc, *lnd; };
EvaPrepared eva_prepared(Carve& cv, int dim, int hidden) {
    const int D = dim, Hp = kpad32(hidden);
    EvaPrepared p;
    p.qkv = take_packed(cv, 3 * D, D); p.bqkv = cv.take<float>(3 * D);      // q | k | v, their bias
    p.proj = take_packed(cv, D, D);
    p.w1 = take_packed(cv, 2 * Hp, D); p.b1 = cv.take<float>(2 * Hp);        // fc1 (g / x interleaved), its bias
    p.w2g = take_packed(cv, D, Hp); p.lnc = cv.take<float>(D); p.lnd = cv.take<float>(D);      // fc2 * gamma, ln_c, ln_d
    return p;
}

struct EvaWs { float *h, *rs, *ub, *so, *qkv, *sq, *o, *u, *su, *st, *mean, *rstd; };
EvaWs eva_ws(Carve& cv, int64_t M, int dim, int hidden) {
    const int64_t D = dim, Dp = kpad32(dim), Hp = kpad32(hidden), segs = psam_gemm_f16x3p_stat_segs((int32_t)(2 * Hp));
    EvaWs w;
    w.h = cv.take<float>(M * Dp);                                                    // LayerNorm output, packed
    w.rs = cv.take<float>(M); w.ub = cv.take<float>(M); w.so = cv.take<float>(M);    // its row scales, the gated rows' bound, attention output scales
    w.qkv = cv.take<float>(M * 3 * D); w.sq = cv.take<float>(M);                     // q | k | v packed, their scale
    w.o = cv.take<float>(M * Dp);                                                    // attention output, packed
    w.u = cv.take<float>(M * Hp); w.su = cv.take<float>(M);                          // gated hidden rows, packed, their scales
    w.st = cv.take<float>(M * segs * 2);                                             // LayerNorm partials
    w.mean = cv.take<float>(M); w.rstd = cv.take<float>(M);
    return w;
}
}  // namespace

// bytes of the device blob psam_eva_block_prepare fills
PSAM_API size_t psam_eva_block_prepared_bytes(int32_t dim, int32_t hidden) {
    if (dim <= 0 || hidden <= 0) return 0;
    return carved_bytes([&](Carve& cv) { eva_prepared(cv, dim, hidden); });
}

// Packs one block's weights into `prepared` (device, psam_eva_block_prepared_bytes) and fills `plan` (host).  Load-time call: it copies the
// weights to the host, builds the concatenated / interleaved / gamma-folded matrices and the bounds there in double precision, and uses a
// temporary device buffer for the fp32 staging of the largest matrix.  Synchronises `stream`.
PSAM_API int32_t psam_eva_block_prepare(const psam_eva_block_weights_t* wt, psam_eva_block_plan_t* plan, void* prepared, size_t prepared_bytes, hipStream_t stream) {
#define WHO "psam_eva_block_prepare"
    PSAM_REQUIRE(wt && plan && prepared, PSAM_EINVAL, WHO ": null pointer");
    const int D = wt->dim, H = wt->hidden, heads = wt->heads;
    PSAM_REQUIRE(D > 0 && H > 0 && heads > 0 && D % heads == 0 && D / heads == 64, PSAM_EINVAL, WHO ": head dim must be 64 (the packed-operand attention)");
    // the packed LayerNorm takes 256..4096 columns; the q|k|v GEMM (N = 3 dim, packed output) and fc2 (N = dim, folded LayerNorm) run fused epilogues,
    // which exist for whole 128-column tiles only
    PSAM_REQUIRE(D >= 256 && D <= 4096 && D % 128 == 0, PSAM_EINVAL, WHO ": need 256 <= dim <= 4096 and dim % 128 == 0 (packed LayerNorm, fused GEMM epilogues)");
    const int Hp = kpad32(H);
    PSAM_REQUIRE(Hp % 64 == 0 && Hp >= 128, PSAM_EINVAL,
                 WHO ": hidden rounded up to 32 must be a multiple of 64 (fused SwiGLU epilogue) and at least 128 (the K of a packed-operand GEMM)");
    PSAM_REQUIRE(prepared_bytes >= psam_eva_block_prepared_bytes(D, H), PSAM_EWORKSPACE, WHO ": prepared buffer too small");
    const float* ptrs[] = {wt->norm1_w, wt->norm1_b, wt->q_w, wt->q_b, wt->k_w, wt->v_w, wt->v_b, wt->proj_w, wt->proj_b, wt->norm2_w, wt->norm2_b,
                           wt->fc1_g_w, wt->fc1_g_b, wt->fc1_x_w, wt->fc1_x_b, wt->mlp_norm_w, wt->mlp_norm_b, wt->fc2_w, wt->fc2_b};
    for (const float* p : ptrs) PSAM_REQUIRE(p, PSAM_EINVAL, WHO ": null weight pointer");
    PSAM_REQUIRE(hipStreamSynchronize(stream) == hipSuccess, PSAM_EINVAL, WHO ": stream error");      // the weights may still be arriving on `stream`

    FETCH(WHO, qw, wt->q_w, (int64_t)D * D); FETCH(WHO, kw, wt->k_w, (int64_t)D * D); FETCH(WHO, vw, wt->v_w, (int64_t)D * D);
    FETCH(WHO, qb, wt->q_b, D); FETCH(WHO, vb, wt->v_b, D);
    FETCH(WHO, g1, wt->norm1_w, D); FETCH(WHO, b1n, wt->norm1_b, D);
    FETCH(WHO, gw, wt->fc1_g_w, (int64_t)H * D); FETCH(WHO, xw, wt->fc1_x_w, (int64_t)H * D); FETCH(WHO, gb, wt->fc1_g_b, H); FETCH(WHO, xb, wt->fc1_x_b, H);
    FETCH(WHO, mg, wt->mlp_norm_w, H); FETCH(WHO, mb, wt->mlp_norm_b, H);
    FETCH(WHO, w2, wt->fc2_w, (int64_t)D * H); FETCH(WHO, b2, wt->fc2_b, D);

    // ---- host-side matrices
    std::vector<float> wqkv((size_t)3 * D * D), bqkv((size_t)3 * D, 0.f);
    std::memcpy(wqkv.data(), qw.data(), (size_t)D * D * 4);
    std::memcpy(wqkv.data() + (size_t)D * D, kw.data(), (size_t)D * D * 4);
    std::memcpy(wqkv.data() + (size_t)2 * D * D, vw.data(), (size_t)D * D * 4);
    for (int i = 0; i < D; ++i) { bqkv[i] = qb[i]; bqkv[2 * D + i] = vb[i]; }      // k_proj has no bias (timm EvaAttention)
    // fc1: alternating 32-row blocks of fc1_g / fc1_x, hidden padded to Hp with zero rows (PSAM_ACT_SWIGLU)
    std::vector<float> w1((size_t)2 * Hp * D, 0.f), bias1((size_t)2 * Hp, 0.f);
    for (int n = 0; n < H; ++n) {
        const int64_t blk = n / 32, r = n % 32;
        std::memcpy(&w1[(size_t)((blk * 2) * 32 + r) * D], &gw[(size_t)n * D], (size_t)D * 4);
        std::memcpy(&w1[(size_t)((blk * 2 + 1) * 32 + r) * D], &xw[(size_t)n * D], (size_t)D * 4);
        bias1[(size_t)(blk * 2) * 32 + r] = gb[n];
        bias1[(size_t)(blk * 2 + 1) * 32 + r] = xb[n];
    }
    // fc2 with the inner LayerNorm folded in: fc2(LN(u)) = rstd (u (W2 gamma)^T - mean c) + d,  c = (W2 gamma) 1,  d = W2 beta + b2
    std::vector<float> w2g((size_t)D * Hp, 0.f), lnc(D), lnd(D);
    for (int n = 0; n < D; ++n) {
        double c = 0.0, d = (double)b2[n];
        for (int k = 0; k < H; ++k) {
            const double wg = (double)w2[(size_t)n * H + k] * (double)mg[k];
            w2g[(size_t)n * Hp + k] = (float)wg;
            c += wg;
            d += (double)w2[(size_t)n * H + k] * (double)mb[k];
        }
        lnc[n] = (float)c; lnd[n] = (float)d;
    }
    // ---- bounds: |W_n . h + b_n| <= ||W_n|| ||h|| + |b_n|;  a LayerNorm output has ||h|| <= max|gamma| sqrt(D) + ||beta||
    double gmax = 0.0, bnorm = 0.0;
    for (int i = 0; i < D; ++i) { gmax = std::fmax(gmax, std::fabs((double)g1[i])); bnorm += (double)b1n[i] * (double)b1n[i]; }
    const double hnorm = gmax * std::sqrt((double)D) + std::sqrt(bnorm);
    double nmax_all = 0.0, nmax_v = 0.0, bmax_all = 0.0, bmax_v = 0.0;
    for (int n = 0; n < 3 * D; ++n) {
        const double nn = row_norm(&wqkv[(size_t)n * D], D);
        nmax_all = std::fmax(nmax_all, nn); bmax_all = std::fmax(bmax_all, std::fabs((double)bqkv[n]));
        if (n >= 2 * D) { nmax_v = std::fmax(nmax_v, nn); bmax_v = std::fmax(bmax_v, std::fabs((double)bqkv[n])); }
    }
    // gated rows: |silu(g_n) x_n| <= (a_n t + b_n)(c_n t + d_n), t = ||h||_2 per row; coefficient-wise maxima over the hidden units
    double k2 = 0.0, k1 = 0.0, k0 = 0.0;
    for (int n = 0; n < H; ++n) {
        const double a = row_norm(&gw[(size_t)n * D], D), c = row_norm(&xw[(size_t)n * D], D), b = std::fabs((double)gb[n]), d = std::fabs((double)xb[n]);
        k2 = std::fmax(k2, a * c); k1 = std::fmax(k1, a * d + b * c); k0 = std::fmax(k0, b * d);
    }
    std::memset(plan, 0, sizeof(*plan));
    plan->dim = D; plan->heads = heads; plan->hidden = H; plan->hidden_pad = Hp; plan->eps = wt->eps;
    plan->qkv_bound = (float)(1.001 * (nmax_all * hnorm + bmax_all) + 1e-30);
    plan->v_bound = (float)(1.001 * (nmax_v * hnorm + bmax_v) + 1e-30);
    plan->u_c2 = (float)(1.002 * k2); plan->u_c1 = (float)(1.002 * k1); plan->u_c0 = (float)(1.002 * k0 + 1e-30);
    plan->norm1_w = wt->norm1_w; plan->norm1_b = wt->norm1_b; plan->norm2_w = wt->norm2_w; plan->norm2_b = wt->norm2_b; plan->proj_b = wt->proj_b;

    // ---- device blob: upload the fp32 matrix to a temporary, row scales + g8 packing by the library's own kernels
    Carve cv(prepared);
    const EvaPrepared p = eva_prepared(cv, D, H);
    put_offsets(cv, p.qkv, &plan->o_wqkv, &plan->o_sqkv); plan->o_bqkv = cv.offset_of(p.bqkv);
    put_offsets(cv, p.proj, &plan->o_wproj, &plan->o_sproj);
    put_offsets(cv, p.w1, &plan->o_w1, &plan->o_s1); plan->o_b1 = cv.offset_of(p.b1);
    put_offsets(cv, p.w2g, &plan->o_w2g, &plan->o_s2g); plan->o_lnc = cv.offset_of(p.lnc); plan->o_lnd = cv.offset_of(p.lnd);

    float* tmp = nullptr;      // ONE staging buffer for every host-built matrix: each pack is synchronised before the next upload overwrites it
    const int64_t tmp_floats = std::max<int64_t>({(int64_t)3 * D * D, (int64_t)2 * Hp * D, (int64_t)D * Hp});
    PSAM_REQUIRE(hipMalloc(&tmp, (size_t)tmp_floats * 4) == hipSuccess, PSAM_EINVAL, WHO ": cannot allocate the staging buffer");
    int32_t rc = PSAM_OK;
    auto pack = [&](const std::vector<float>& host, int rows, int K, const Packed& dst) {
        if (!rc && hipMemcpyAsync(tmp, host.data(), (size_t)rows * K * 4, hipMemcpyHostToDevice, stream) != hipSuccess) rc = fail(WHO, "upload failed");
        if (!rc) rc = packing_done(WHO, pack_weight(WHO, tmp, K, rows, K, dst, stream), stream);
    };
    auto up = [&](float* dst, const std::vector<float>& src) {
        if (!rc && hipMemcpy(dst, src.data(), src.size() * 4, hipMemcpyHostToDevice) != hipSuccess) rc = fail(WHO, "upload failed");
    };
    pack(wqkv, 3 * D, D, p.qkv);
    if (!rc) rc = packing_done(WHO, pack_weight(WHO, wt->proj_w, D, D, D, p.proj, stream), stream);
    pack(w1, 2 * Hp, D, p.w1);
    pack(w2g, D, Hp, p.w2g);
    up(p.bqkv, bqkv); up(p.b1, bias1); up(p.lnc, lnc); up(p.lnd, lnd);
    (void)hipFree(tmp);
    return rc;
#undef WHO
}

// workspace of one psam_eva_block call on M token rows
PSAM_API size_t psam_eva_block_ws_bytes(int64_t M, int32_t dim, int32_t hidden) {
    if (M <= 0 || dim <= 0 || hidden <= 0) return 0;
    return carved_bytes([&](Carve& cv) { eva_ws(cv, M, dim, hidden); });
}

// x [B*L, dim] (fp32, updated in place) <- block(x).  M = B * L must be a multiple of 256 (the fused GEMM epilogues work on whole tiles).
PSAM_API int32_t psam_eva_block(const psam_eva_block_plan_t* plan, const void* prepared, float* x, int32_t B, int32_t L, void* ws, size_t ws_bytes, hipStream_t stream) {
    PSAM_REQUIRE(plan && prepared && x && ws, PSAM_EINVAL, "psam_eva_block: null pointer");
    const int D = plan->dim, H = plan->hidden, Hp = plan->hidden_pad, heads = plan->heads, Dp = kpad32(D);
    const int64_t M = (int64_t)B * L;
    PSAM_REQUIRE(B > 0 && L > 0 && M % 256 == 0 && M < ((int64_t)1 << 31), PSAM_EINVAL, "psam_eva_block: B * L must be a positive multiple of 256");
    PSAM_REQUIRE(ws_bytes >= psam_eva_block_ws_bytes(M, D, H), PSAM_EWORKSPACE, "psam_eva_block: workspace too small");
    auto P = [&](int64_t off) { return at(prepared, off); };
    const int segs = psam_gemm_f16x3p_stat_segs(2 * Hp);
    Carve cv(ws);
    const EvaWs w = eva_ws(cv, M, D, H);
    int32_t rc;
    // attention half
    rc = psam_layernorm_ex(x, D, nullptr, 0, plan->norm1_w, plan->norm1_b, w.h, Dp, M, D, plan->eps, 0, w.rs, 1, stream);
    if (rc) return rc;
    psam_gemm_fuse_t f;
    std::memset(&f, 0, sizeof(f));
    f.pack_out = 1; f.out_scale = w.sq; f.out_k1 = 0.f; f.out_k2 = plan->qkv_bound;
    rc = psam_gemm_f16x3p_ex(w.h, Dp, w.rs, P(plan->o_wqkv), Dp, P(plan->o_sqkv), w.qkv, 3 * D, P(plan->o_bqkv), nullptr, 0, nullptr, 0, 0, (int32_t)M, 3 * D, Dp, 1.f, 0, &f, stream);
    if (rc) return rc;
    rc = psam_attention_packed(w.qkv, 3 * D, w.sq, w.o, Dp, w.so, B, heads, L, D / heads, 1.0f / std::sqrt((float)(D / heads)), plan->v_bound, stream);
    if (rc) return rc;
    rc = psam_gemm_f16x3p_ex(w.o, Dp, w.so, P(plan->o_wproj), Dp, P(plan->o_sproj), x, D, plan->proj_b, x, D, nullptr, 0, 0, (int32_t)M, D, Dp, 1.f, 0, nullptr, stream);
    if (rc) return rc;
    // MLP half
    rc = psam_layernorm_ex2(x, D, nullptr, 0, plan->norm2_w, plan->norm2_b, w.h, Dp, M, D, plan->eps, 0, w.rs, 1, w.ub, plan->u_c2, plan->u_c1, plan->u_c0, stream);
    if (rc) return rc;
    std::memset(&f, 0, sizeof(f));
    f.pack_out = 1; f.out_scale = w.su; f.out_bound = w.ub; f.stats = w.st; f.stat_cols = H;
    rc = psam_gemm_f16x3p_ex(w.h, Dp, w.rs, P(plan->o_w1), Dp, P(plan->o_s1), w.u, Hp, P(plan->o_b1), nullptr, 0, nullptr, 0, 0, (int32_t)M, 2 * Hp, Dp, 1.f, PSAM_ACT_SWIGLU, &f, stream);
    if (rc) return rc;
    rc = psam_ln_stats_finalize(w.st, (int32_t)M, segs, H, plan->eps, w.mean, w.rstd, stream);
    if (rc) return rc;
    std::memset(&f, 0, sizeof(f));
    f.ln_mean = w.mean; f.ln_rstd = w.rstd; f.ln_c = P(plan->o_lnc);
    return psam_gemm_f16x3p_ex(w.u, Hp, w.su, P(plan->o_w2g), Hp, P(plan->o_s2g), x, D, P(plan->o_lnd), x, D, nullptr, 0, 0, (int32_t)M, D, Hp, 1.f, 0, &f, stream);
}

// ================================================================================================================================
// psam_eva_gelu_block: one block of the giant encoder (timm eva_giant_patch14_560: fused qkv with q / v bias, GELU MLP, head dim 88) -- the launch
// sequence of PointCloudSAM._block for `not vit.swiglu` (point_sam_amd/model.py), decisions included: the same split-K factors (the library's own
// psam_gemm_f16x3p_splitk), the same packed hand-overs, hence the same bits.
// ================================================================================================================================
namespace {
struct GeluPrepared { Packed qkv; float* bqkv; Packed proj, w1, w2; };
GeluPrepared gelu_prepared(Carve& cv, int dim, int hidden) {
    return {take_packed(cv, 3 * dim, dim), cv.take<float>(3 * dim), take_packed(cv, dim, dim), take_packed(cv, hidden, dim), take_packed(cv, dim, hidden)};
}

// scratch of the key-split attention inside psam_eva_gelu_block: the largest single-cloud case (4 splits x 64 units x 66 KiB = 16.5 MiB) with room to spare;
// a shape that would need more runs with a smaller split factor (psam_attention_f16x3_ex2 caps it to the scratch it is given)
constexpr int64_t GELU_KS_WS_BYTES = (int64_t)32 << 20;
struct GeluWs { float *h, *rs, *ub, *so, *sg, *qkv, *o, *g, *gp, *planes; char* ks_ws; };
GeluWs gelu_ws(Carve& cv, int64_t M, int dim, int hidden) {
    const int64_t D = dim, Dp = kpad32(dim), Hp = kpad32(hidden), widest = std::max(3 * D, Hp);
    GeluWs w;
    w.h = cv.take<float>(M * Dp);                                  // packed LayerNorm rows
    w.rs = cv.take<float>(M); w.ub = cv.take<float>(M); w.so = cv.take<float>(M); w.sg = cv.take<float>(M);      // its scales, the fc1 bound, attention-output scales, fc2-input scales
    w.qkv = cv.take<float>(M * 3 * D);                             // fp32
    w.o = cv.take<float>(M * Dp);                                  // attention output, packed
    w.g = cv.take<float>(M * Hp); w.gp = cv.take<float>(M * Hp);   // GELU(fc1) rows (fp32 or packed) and their packed copy
    w.planes = cv.take<float>(4 * M * widest);                     // split-K partial planes (<= 4 per launch)
    w.ks_ws = cv.take<char>(GELU_KS_WS_BYTES);                     // key-split attention: partial softmax states (used by single-cloud shapes only)
    return w;
}
}  // namespace

PSAM_API size_t psam_eva_gelu_block_prepared_bytes(int32_t dim, int32_t hidden) {
    if (dim <= 0 || hidden <= 0) return 0;
    return carved_bytes([&](Carve& cv) { gelu_prepared(cv, dim, hidden); });
}

PSAM_API int32_t psam_eva_gelu_block_prepare(const psam_eva_gelu_block_weights_t* wt, psam_eva_gelu_block_plan_t* plan, void* prepared, size_t prepared_bytes,
                                             hipStream_t stream) {
#define WHO "psam_eva_gelu_block_prepare"
    PSAM_REQUIRE(wt && plan && prepared, PSAM_EINVAL, WHO ": null pointer");
    const int D = wt->dim, H = wt->hidden, heads = wt->heads;
    PSAM_REQUIRE(wt->precision == PSAM_PRECISION_F16X3, PSAM_EINVAL, WHO ": the coarse entry is built for PSAM_PRECISION_F16X3");
    PSAM_REQUIRE(D >= 256 && D <= 4096 && D % 32 == 0 && H >= 128 && H % 32 == 0 && heads > 0 && D % heads == 0, PSAM_EINVAL,
                 WHO ": need 256 <= dim <= 4096, dim % 32 == 0, hidden % 32 == 0, hidden >= 128 (the K of a packed-operand GEMM)");
    const int hd = D / heads;
    PSAM_REQUIRE(hd == 64 || (hd > 64 && hd <= 128 && hd % 8 == 0), PSAM_EINVAL, WHO ": head dim must be 64 or a multiple of 8 in (64, 128]");
    PSAM_REQUIRE(prepared_bytes >= psam_eva_gelu_block_prepared_bytes(D, H), PSAM_EWORKSPACE, WHO ": prepared buffer too small");
    const float* ptrs[] = {wt->norm1_w, wt->norm1_b, wt->qkv_w, wt->q_bias, wt->v_bias, wt->proj_w, wt->proj_b, wt->norm2_w, wt->norm2_b, wt->fc1_w, wt->fc1_b, wt->fc2_w, wt->fc2_b};
    for (const float* q : ptrs) PSAM_REQUIRE(q, PSAM_EINVAL, WHO ": null weight pointer");
    PSAM_REQUIRE(hipStreamSynchronize(stream) == hipSuccess, PSAM_EINVAL, WHO ": stream error");
    FETCH(WHO, vw, wt->qkv_w + (int64_t)2 * D * D, (int64_t)D * D); FETCH(WHO, qb, wt->q_bias, D); FETCH(WHO, vb, wt->v_bias, D);
    FETCH(WHO, w1, wt->fc1_w, (int64_t)H * D); FETCH(WHO, b1, wt->fc1_b, H);
    std::vector<float> bqkv((size_t)3 * D, 0.f);
    for (int i = 0; i < D; ++i) { bqkv[i] = qb[i]; bqkv[2 * D + i] = vb[i]; }
    // bound of |V| from the scale of the LayerNorm row that produced it (psam_attention_f16x3_ex): k1 = 2^15 sqrt(D) max ||W_v[n]||, k2 = max |b_v|
    double nv = 0.0, bv = 0.0, n1 = 0.0, bm1 = 0.0;
    for (int n = 0; n < D; ++n) { nv = std::fmax(nv, row_norm(&vw[(size_t)n * D], D)); bv = std::fmax(bv, std::fabs((double)vb[n])); }
    for (int n = 0; n < H; ++n) { n1 = std::fmax(n1, row_norm(&w1[(size_t)n * D], D)); bm1 = std::fmax(bm1, std::fabs((double)b1[n])); }
    std::memset(plan, 0, sizeof(*plan));
    plan->dim = D; plan->heads = heads; plan->hidden = H; plan->precision = wt->precision; plan->eps = wt->eps;
    plan->attn_keysplit = 4;
    plan->vk1 = (float)(32768.0 * std::sqrt((double)D) * nv); plan->vk2 = (float)bv;
    plan->u_c1 = (float)(1.002 * n1); plan->u_c0 = (float)(1.002 * bm1 + 1e-30);      // |GELU(W_n . h + b_n)| <= ||W_n|| t + |b_n|, t = ||h||_2
    plan->norm1_w = wt->norm1_w; plan->norm1_b = wt->norm1_b; plan->norm2_w = wt->norm2_w; plan->norm2_b = wt->norm2_b; plan->proj_b = wt->proj_b;
    plan->fc1_b = wt->fc1_b; plan->fc2_b = wt->fc2_b;
    Carve cv(prepared);
    const GeluPrepared p = gelu_prepared(cv, D, H);
    put_offsets(cv, p.qkv, &plan->o_wqkv, &plan->o_sqkv); plan->o_bqkv = cv.offset_of(p.bqkv);
    put_offsets(cv, p.proj, &plan->o_wproj, &plan->o_sproj);
    put_offsets(cv, p.w1, &plan->o_w1, &plan->o_s1);
    put_offsets(cv, p.w2, &plan->o_w2, &plan->o_s2);
    int32_t rc = pack_weight(WHO, wt->qkv_w, D, 3 * D, D, p.qkv, stream);
    if (!rc) rc = pack_weight(WHO, wt->proj_w, D, D, D, p.proj, stream);
    if (!rc) rc = pack_weight(WHO, wt->fc1_w, D, H, D, p.w1, stream);
    if (!rc) rc = pack_weight(WHO, wt->fc2_w, H, D, H, p.w2, stream);
    if (!rc && hipMemcpy(p.bqkv, bqkv.data(), bqkv.size() * 4, hipMemcpyHostToDevice) != hipSuccess) rc = fail(WHO, "upload failed");
    return packing_done(WHO, rc, stream);
#undef WHO
}

PSAM_API size_t psam_eva_gelu_block_ws_bytes(int64_t M, int32_t dim, int32_t hidden) {
    if (M <= 0 || dim <= 0 || hidden <= 0) return 0;
    return carved_bytes([&](Carve& cv) { gelu_ws(cv, M, dim, hidden); });
}

PSAM_API int32_t psam_eva_gelu_block(const psam_eva_gelu_block_plan_t* plan, const void* prepared, float* x, int32_t B, int32_t L, void* ws, size_t ws_bytes,
                                     int32_t* counters, hipStream_t stream) {
    PSAM_REQUIRE(plan && prepared && x && ws, PSAM_EINVAL, "psam_eva_gelu_block: null pointer");
    const int D = plan->dim, H = plan->hidden, heads = plan->heads, Dp = kpad32(D), Hp = kpad32(H), hd = D / heads;
    const int64_t M = (int64_t)B * L;
    PSAM_REQUIRE(B > 0 && L > 0 && M >= 256 && M < ((int64_t)1 << 31), PSAM_EINVAL, "psam_eva_gelu_block: B * L must be at least 256 (the packed-operand GEMMs)");
    PSAM_REQUIRE(ws_bytes >= psam_eva_gelu_block_ws_bytes(M, D, H), PSAM_EWORKSPACE, "psam_eva_gelu_block: workspace too small");
    auto P = [&](int64_t off) { return at(prepared, off); };
    Carve cv(ws);
    const GeluWs w = gelu_ws(cv, M, D, H);
    // a plain GEMM as the host's ops.linear issues it: the library's split-K factor, partial planes in the workspace
    auto gemm = [&](const float* A, int64_t lda, const float* sA, int64_t ow, int64_t os, int N, int K, float* C, int64_t ldc, const float* bias, const float* res, int act) -> int32_t {
        psam_gemm_fuse_t f;
        std::memset(&f, 0, sizeof(f));
        const int ks = ((N & 3) == 0 && (ldc & 3) == 0) ? psam_gemm_f16x3p_splitk((int32_t)M, N, K, act) : 1;
        if (ks > 1) { f.splitk = ks; f.splitk_ws = w.planes; f.splitk_plane = M * (int64_t)N; f.counters = counters; }
        return psam_gemm_f16x3p_ex(A, lda, sA, P(ow), K, P(os), C, ldc, bias, res, res ? ldc : 0, nullptr, 0, 0, (int32_t)M, N, K, 1.f, act, ks > 1 ? &f : nullptr, stream);
    };
    int32_t rc;
    // attention half
    rc = psam_layernorm_ex(x, D, nullptr, 0, plan->norm1_w, plan->norm1_b, w.h, Dp, M, D, plan->eps, 0, w.rs, 1, stream);
    if (rc) return rc;
    rc = gemm(w.h, Dp, w.rs, plan->o_wqkv, plan->o_sqkv, 3 * D, Dp, w.qkv, 3 * D, P(plan->o_bqkv), nullptr, 0);
    if (rc) return rc;
    rc = psam_attention_f16x3_ex2(w.qkv, 3 * D, (int64_t)L * 3 * D, w.qkv + D, 3 * D, (int64_t)L * 3 * D, w.qkv + 2 * D, 3 * D, (int64_t)L * 3 * D, w.o, Dp, (int64_t)L * Dp, B, heads, L, L,
                                  hd, (float)std::pow((double)hd, -0.5), w.rs, plan->vk1, plan->vk2, w.so, plan->attn_keysplit > 0 ? plan->attn_keysplit : 1, w.ks_ws, (size_t)GELU_KS_WS_BYTES, counters, stream);      // float(hd ** -0.5), as the host computes it
    if (rc) return rc;
    rc = gemm(w.o, Dp, w.so, plan->o_wproj, plan->o_sproj, D, Dp, x, D, plan->proj_b, x, 0);
    if (rc) return rc;
    // MLP half
    const bool fused_gelu = (M % 256 == 0) && (H % 128 == 0) && psam_gemm_f16x3p_splitk((int32_t)M, H, Dp, PSAM_ACT_GELU) == 1;
    if (fused_gelu) {
        rc = psam_layernorm_ex2(x, D, nullptr, 0, plan->norm2_w, plan->norm2_b, w.h, Dp, M, D, plan->eps, 0, w.rs, 1, w.ub, 0.f, plan->u_c1, plan->u_c0, stream);
        if (rc) return rc;
        psam_gemm_fuse_t f;
        std::memset(&f, 0, sizeof(f));
        f.pack_out = 1; f.out_scale = w.sg; f.out_bound = w.ub;
        rc = psam_gemm_f16x3p_ex(w.h, Dp, w.rs, P(plan->o_w1), Dp, P(plan->o_s1), w.g, Hp, plan->fc1_b, nullptr, 0, nullptr, 0, 0, (int32_t)M, H, Dp, 1.f, PSAM_ACT_GELU, &f, stream);
        if (rc) return rc;
        return gemm(w.g, Hp, w.sg, plan->o_w2, plan->o_s2, D, Hp, x, D, plan->fc2_b, x, 0);
    }
    rc = psam_layernorm_ex(x, D, nullptr, 0, plan->norm2_w, plan->norm2_b, w.h, Dp, M, D, plan->eps, 0, w.rs, 1, stream);
    if (rc) return rc;
    rc = gemm(w.h, Dp, w.rs, plan->o_w1, plan->o_s1, H, Dp, w.g, H, plan->fc1_b, nullptr, PSAM_ACT_GELU);
    if (rc) return rc;
    rc = psam_scale_pack_rows_g8(w.g, H, (int32_t)M, H, w.gp, Hp, w.sg, stream);
    if (rc) return rc;
    return gemm(w.gp, Hp, w.sg, plan->o_w2, plan->o_s2, D, Hp, x, D, plan->fc2_b, x, 0);
}

// ================================================================================================================================
// psam_patch_encoder: PatchEncoder.forward on kNN groups (pc_sam/model/common.py:477-506 after KNNGrouper / group_with_centers_and_knn,
// :99-120 / :126-187) -- the mini-PointNet of the patch embedding (features = rgb) and of the mask encoder (features = mask logits) -- as the
// Python host runs it in "f16x3": gather + Linear + LayerNorm + GELU in one kernel (packed rows) | conv1.3 GEMM with the group maximum and a
// packed output in its epilogue | the pooled half of conv2.0 once per group | conv2.0 on the rows with that as a row bias | LayerNorm + GELU
// (packed) | conv2.3 GEMM whose epilogue keeps only the group maximum.  hidden_dims[0] == 128, group size 32 or a multiple of 64
// (above 64: the epilogues pool 64-row parts, psam_group_max pools the parts), rows % 256 == 0.
// ================================================================================================================================
namespace {
// conv2.0 [h1, 2 h0] = [pooled half | per-row half]: cat([max, x]) W^T = max W[:, :h0]^T + x W[:, h0:]^T, each half packed with its own row scales
struct PatchPrepared { Packed c13, c20m, c20x, c23; };
PatchPrepared patch_prepared(Carve& cv, int h0, int h1, int cout) {
    return {take_packed(cv, h0, h0), take_packed(cv, h1, h0), take_packed(cv, h1, h0), take_packed(cv, cout, h1)};
}

struct PatchWs { float *x1, *x2, *s1, *s2, *rs, *y1, *y1p, *sy, *g1, *x3; };
PatchWs patch_ws(Carve& cv, int64_t rows, int64_t groups, int h0, int h1) {
    const int64_t a = kpad32(h0), b = kpad32(h1);
    PatchWs w;
    w.x1 = cv.take<float>(rows * a); w.x2 = cv.take<float>(rows * a);                                    // conv1.1 and conv1.3 rows, packed
    w.s1 = cv.take<float>(rows); w.s2 = cv.take<float>(rows); w.rs = cv.take<float>(rows);               // their scales, conv2.1's
    w.y1 = cv.take<float>(groups * a); w.y1p = cv.take<float>(groups * a); w.sy = cv.take<float>(groups);      // group maxima of conv1.3, fp32 and packed
    w.g1 = cv.take<float>(groups * h1);                                                                  // the pooled half of conv2.0
    w.x3 = cv.take<float>(rows * b);                                                                     // conv2.0 / conv2.1 rows
    return w;
}
}  // namespace

PSAM_API size_t psam_patch_encoder_prepared_bytes(int32_t h0, int32_t h1, int32_t cout) {
    if (h0 <= 0 || h1 <= 0 || cout <= 0) return 0;
    return carved_bytes([&](Carve& cv) { patch_prepared(cv, h0, h1, cout); });
}

PSAM_API int32_t psam_patch_encoder_prepare(const psam_patch_encoder_weights_t* wt, psam_patch_encoder_plan_t* plan, void* prepared, size_t prepared_bytes,
                                            hipStream_t stream) {
#define WHO "psam_patch_encoder_prepare"
    PSAM_REQUIRE(wt && plan && prepared, PSAM_EINVAL, WHO ": null pointer");
    const int h0 = wt->h0, h1 = wt->h1, cout = wt->cout, cin = wt->cin;
    PSAM_REQUIRE(h0 == 128 && h1 >= 256 && h1 % 128 == 0 && h1 <= 4096 && cout >= 128 && cout % 128 == 0 && cin >= 4, PSAM_EINVAL,
                 WHO ": hidden_dims[0] must be 128, hidden_dims[1] a multiple of 128 in [256, 4096], out_channels a multiple of 128");
    PSAM_REQUIRE(wt->c10_w && wt->c10_b && wt->c11_w && wt->c11_b && wt->c13_w && wt->c13_b && wt->c20_w && wt->c20_b && wt->c21_w && wt->c21_b && wt->c23_w && wt->c23_b,
                 PSAM_EINVAL, WHO ": null weight pointer");
    PSAM_REQUIRE(prepared_bytes >= psam_patch_encoder_prepared_bytes(h0, h1, cout), PSAM_EWORKSPACE, WHO ": prepared buffer too small");
    PSAM_REQUIRE(hipStreamSynchronize(stream) == hipSuccess, PSAM_EINVAL, WHO ": stream error");      // the weights may still be arriving on `stream`
    FETCH(WHO, w13, wt->c13_w, (int64_t)h0 * h0); FETCH(WHO, b13, wt->c13_b, h0); FETCH(WHO, g21, wt->c21_w, h1); FETCH(WHO, b21, wt->c21_b, h1);
    double nmax = 0.0, bmax = 0.0, gm = 0.0, bm = 0.0;
    for (int n = 0; n < h0; ++n) { nmax = std::fmax(nmax, row_norm(&w13[(size_t)n * h0], h0)); bmax = std::fmax(bmax, std::fabs((double)b13[n])); }
    for (int n = 0; n < h1; ++n) { gm = std::fmax(gm, std::fabs((double)g21[n])); bm = std::fmax(bm, std::fabs((double)b21[n])); }
    std::memset(plan, 0, sizeof(*plan));
    plan->cin = cin; plan->h0 = h0; plan->h1 = h1; plan->cout = cout; plan->eps = wt->eps;
    plan->k1 = (float)(32768.0 * std::sqrt((double)h0) * nmax);      // |conv1.3 row| <= k1 / scale(input row) + k2 (psam_gemm_fuse_t)
    plan->k2 = (float)bmax;
    // conv2.1's LayerNorm output: |(x - mean) rstd gamma + beta| <= max |gamma| sqrt(h1) + max |beta| (GELU only shrinks it)
    plan->ln21_bound = (float)(1.001 * (gm * std::sqrt((double)h1) + bm) + 1e-30);
    plan->c10_w = wt->c10_w; plan->c10_b = wt->c10_b; plan->c11_w = wt->c11_w; plan->c11_b = wt->c11_b; plan->c13_b = wt->c13_b; plan->c20_w = wt->c20_w;
    plan->c20_b = wt->c20_b; plan->c21_w = wt->c21_w; plan->c21_b = wt->c21_b; plan->c23_b = wt->c23_b;
    Carve cv(prepared);
    const PatchPrepared p = patch_prepared(cv, h0, h1, cout);
    put_offsets(cv, p.c13, &plan->o_w13, &plan->o_s13); put_offsets(cv, p.c20m, &plan->o_w20m, &plan->o_s20m);
    put_offsets(cv, p.c20x, &plan->o_w20x, &plan->o_s20x); put_offsets(cv, p.c23, &plan->o_w23, &plan->o_s23);
    int32_t rc = pack_weight(WHO, wt->c13_w, h0, h0, h0, p.c13, stream);
    if (!rc) rc = pack_weight(WHO, wt->c20_w, 2 * h0, h1, h0, p.c20m, stream);
    if (!rc) rc = pack_weight(WHO, wt->c20_w + h0, 2 * h0, h1, h0, p.c20x, stream);
    if (!rc) rc = pack_weight(WHO, wt->c23_w, h1, cout, h1, p.c23, stream);
    return packing_done(WHO, rc, stream);
#undef WHO
}

PSAM_API size_t psam_patch_encoder_ws_bytes(int64_t rows, int64_t groups, int32_t h0, int32_t h1) {
    if (rows <= 0 || groups <= 0 || h0 <= 0 || h1 <= 0) return 0;
    return carved_bytes([&](Carve& cv) { patch_ws(cv, rows, groups, h0, h1); });
}

// out [B*rep*G, cout] = max over the K group members of conv2(cat(max conv1(x), conv1(x))), x = [rel. xyz (/ radius) | feats (| feats - centre feats)]
PSAM_API int32_t psam_patch_encoder(const psam_patch_encoder_plan_t* plan, const void* prepared, const float* xyz, const float* feats, const float* centers,
                                    const int64_t* knn_idx, const int64_t* center_idx, int32_t B, int32_t rep, int32_t N, int32_t G, int32_t K, int32_t C,
                                    float radius, float* out, void* ws, size_t ws_bytes, hipStream_t stream) {
    PSAM_REQUIRE(plan && prepared && xyz && feats && centers && knn_idx && out && ws, PSAM_EINVAL, "psam_patch_encoder: null pointer");
    const int h0 = plan->h0, h1 = plan->h1, cout = plan->cout, a = kpad32(h0), b = kpad32(h1);
    const int64_t groups = (int64_t)B * rep * G, rows = groups * K;
    PSAM_REQUIRE(B > 0 && rep > 0 && N > 0 && G > 0 && (K == 32 || (K > 0 && K % 64 == 0)) && rows % 256 == 0 && rows < ((int64_t)1 << 31), PSAM_EINVAL,
                 "psam_patch_encoder: group size must be 32 or a multiple of 64, and B * rep * G * K a multiple of 256");
    const int Kp = K <= 64 ? K : 64, parts = K / Kp;      // the GEMM epilogues pool 64-row parts of a larger group; psam_group_max pools the parts
    PSAM_REQUIRE(plan->cin == 3 + C * (center_idx ? 2 : 1), PSAM_EINVAL, "psam_patch_encoder: feature channels do not match the first Linear");
    PSAM_REQUIRE(ws_bytes >= psam_patch_encoder_ws_bytes(rows, groups, h0, h1), PSAM_EWORKSPACE, "psam_patch_encoder: workspace too small");
    auto P = [&](int64_t off) { return at(prepared, off); };
    Carve cv(ws);
    const PatchWs w = patch_ws(cv, rows, groups, h0, h1);
    float* part1 = parts > 1 ? w.x3 : w.y1;                 // [groups * parts, h0] partial maxima of conv1.3 (x3 is free until conv2.0 writes it)
    float* part2 = parts > 1 ? w.x1 : out;                  // [groups * parts, cout] partial maxima of conv2.3 (x1 is free after conv1.3)
    PSAM_REQUIRE(parts == 1 || ((int64_t)groups * parts * h0 <= rows * b && (int64_t)groups * parts * cout <= rows * a), PSAM_EINVAL,
                 "psam_patch_encoder: partial maxima do not fit the workspace");
    int32_t rc = psam_patch_l1_ex(xyz, feats, centers, knn_idx, center_idx, plan->c10_w, plan->c10_b, plan->c11_w, plan->c11_b, plan->eps, B, rep, N, G, K, C, radius, w.x1, w.s1, stream);
    if (rc) return rc;
    psam_gemm_fuse_t f;
    std::memset(&f, 0, sizeof(f));
    f.pack_out = 1; f.out_scale = w.s2; f.out_k1 = plan->k1; f.out_k2 = plan->k2; f.gmax_out = part1; f.gmax_ld = h0; f.gmax_k = Kp;
    rc = psam_gemm_f16x3p_ex(w.x1, a, w.s1, P(plan->o_w13), a, P(plan->o_s13), w.x2, a, plan->c13_b, nullptr, 0, nullptr, 0, 0, (int32_t)rows, h0, a, 1.f, 0, &f, stream);
    if (rc) return rc;
    if (parts > 1) { rc = psam_group_max(part1, h0, w.y1, h0, groups, parts, h0, stream); if (rc) return rc; }
    const Lin c20m{plan->c20_w, 2 * h0, plan->c20_b, P(plan->o_w20m), P(plan->o_s20m), h1, h0};
    rc = host_linear(c20m, w.y1, groups, w.g1, 0, G, w.y1p, w.sy, stream);      // the pooled half of conv2.0, one row per group
    if (rc) return rc;
    if (h1 == 512 && rows % 128 == 0 && psam_gemm_f16x3p_fused_row_ln(h1)) {
        // conv2.0 -> LayerNorm -> GELU in ONE GEMM on full-row 128x512 tiles (register epilogue): packed rows out, scaled by the LayerNorm's a-priori bound
        std::memset(&f, 0, sizeof(f));
        f.row_ln_g = plan->c21_w; f.row_ln_b = plan->c21_b; f.row_ln_eps = plan->eps; f.pack_out = 1; f.out_scale = w.rs; f.out_k1 = 0.f; f.out_k2 = plan->ln21_bound;
        rc = psam_gemm_f16x3p_ex(w.x2, a, w.s2, P(plan->o_w20x), a, P(plan->o_s20x), w.x3, b, nullptr, nullptr, 0, w.g1, h1, K, (int32_t)rows, h1, a, 1.f, PSAM_ACT_GELU, &f, stream);
        if (rc) return rc;
    } else if (h0 == 128 && h1 == 512 && rows % 64 == 0) {
        // the same three steps in one register-row kernel (patch_rowln.hip): the 128 -> 512 weight stays in registers, x3 receives the packed rows at once
        rc = psam_linear128_ln_gelu_pack(w.x2, a, w.s2, P(plan->o_w20x), a, P(plan->o_s20x), w.g1, h1, K, plan->c21_w, plan->c21_b, plan->eps, plan->ln21_bound, rows, h1,
                                         w.x3, b, w.rs, stream);
        if (rc) return rc;
    } else {
        rc = psam_gemm_f16x3p_ex(w.x2, a, w.s2, P(plan->o_w20x), a, P(plan->o_s20x), w.x3, h1, nullptr, nullptr, 0, w.g1, h1, K, (int32_t)rows, h1, a, 1.f, 0, nullptr, stream);
        if (rc) return rc;
        rc = psam_layernorm_ex(w.x3, h1, nullptr, 0, plan->c21_w, plan->c21_b, w.x3, b, rows, h1, plan->eps, PSAM_ACT_GELU, w.rs, 1, stream);
        if (rc) return rc;
    }
    std::memset(&f, 0, sizeof(f));
    f.gmax_out = part2; f.gmax_ld = cout; f.gmax_k = Kp; f.no_store = 1;
    rc = psam_gemm_f16x3p_ex(w.x3, b, w.rs, P(plan->o_w23), b, P(plan->o_s23), out, cout, plan->c23_b, nullptr, 0, nullptr, 0, 0, (int32_t)rows, cout, b, 1.f, 0, &f, stream);
    if (rc || parts == 1) return rc;
    return psam_group_max(part2, cout, out, cout, groups, parts, cout, stream);
}

// ================================================================================================================================
// psam_upscale_masks: the mask decoder after its transformer (pc_sam/model/mask_decoder.py:146-176) -- 3-NN interpolation G -> N, output_upscaling
// (Linear, LayerNorm, GELU, Linear, GELU) and the hyper-network products -- as the Python host runs it in "f16x3": the first Linear on the G
// patch rows BEFORE the interpolation (an affine combination commutes with it), LayerNorm + GELU inside the interpolation kernel (packed rows),
// the second Linear + GELU as one GEMM whose epilogue takes the C products per row; the [N, 256] activations are never written.
// transformer_dim 256, Z * N % 256 == 0, N % 32 == 0, C <= 4.
// ================================================================================================================================
namespace {
struct UpscalePrepared { Packed u0, u3; };
UpscalePrepared upscale_prepared(Carve& cv, int dim) { return {take_packed(cv, dim, dim), take_packed(cv, dim, dim)}; }

struct UpscaleWs { float *kp, *k1, *sk, *up, *s1, *parts; };
UpscaleWs upscale_ws(Carve& cv, int64_t Z, int N, int G, int C, int dim) {
    const int64_t a = kpad32(dim), planes = psam_gemm_f16x3p_hyper_planes(dim, 0);
    UpscaleWs w;
    w.kp = cv.take<float>(Z * G * a); w.k1 = cv.take<float>(Z * G * a); w.sk = cv.take<float>(Z * G);      // the patch rows packed, after the first Linear, their scales
    w.up = cv.take<float>(Z * N * a); w.s1 = cv.take<float>(Z * N);                                        // interpolated rows after LayerNorm + GELU, packed, their scales
    w.parts = cv.take<float>(planes * Z * C * N);                                                          // partial hyper-network products
    return w;
}
}  // namespace

PSAM_API size_t psam_upscale_masks_prepared_bytes(int32_t dim) {
    if (dim <= 0) return 0;
    return carved_bytes([&](Carve& cv) { upscale_prepared(cv, dim); });
}

PSAM_API int32_t psam_upscale_masks_prepare(const psam_upscale_weights_t* wt, psam_upscale_plan_t* plan, void* prepared, size_t prepared_bytes, hipStream_t stream) {
#define WHO "psam_upscale_masks_prepare"
    PSAM_REQUIRE(wt && plan && prepared && wt->u0_w && wt->u0_b && wt->u1_w && wt->u1_b && wt->u3_w && wt->u3_b, PSAM_EINVAL, WHO ": null pointer");
    PSAM_REQUIRE(wt->dim == 256, PSAM_EINVAL, WHO ": transformer_dim must be 256");
    PSAM_REQUIRE(prepared_bytes >= psam_upscale_masks_prepared_bytes(wt->dim), PSAM_EWORKSPACE, WHO ": prepared buffer too small");
    const int E = wt->dim;
    std::memset(plan, 0, sizeof(*plan));
    plan->dim = E; plan->eps = wt->eps; plan->u0_w = wt->u0_w; plan->u0_b = wt->u0_b; plan->u1_w = wt->u1_w; plan->u1_b = wt->u1_b; plan->u3_b = wt->u3_b;
    Carve cv(prepared);
    const UpscalePrepared p = upscale_prepared(cv, E);
    put_offsets(cv, p.u0, &plan->o_w0, &plan->o_s0); put_offsets(cv, p.u3, &plan->o_w3, &plan->o_s3);
    int32_t rc = pack_weight(WHO, wt->u0_w, E, E, E, p.u0, stream);
    if (!rc) rc = pack_weight(WHO, wt->u3_w, E, E, E, p.u3, stream);
    return packing_done(WHO, rc, stream);
#undef WHO
}

PSAM_API size_t psam_upscale_masks_ws_bytes(int64_t Z, int32_t N, int32_t G, int32_t C, int32_t dim) {
    if (Z <= 0 || N <= 0 || G <= 0 || C <= 0 || dim <= 0) return 0;
    return carved_bytes([&](Carve& cv) { upscale_ws(cv, Z, N, G, C, dim); });
}

// keys [Z*G, 256]: the patch tokens after the transformer; idx3 / w3 [Z / rep, N, 3]: compute_interp_weights (psam_three_nn); hyper [Z, C, 256]: the
// hyper-network outputs of the selected mask tokens (psam_mlp3); masks [Z, C, N] out.
PSAM_API int32_t psam_upscale_masks(const psam_upscale_plan_t* plan, const void* prepared, const float* keys, const int64_t* idx3, const float* w3,
                                    const float* hyper, int32_t rep, int64_t Z, int32_t N, int32_t G, int32_t C, float* masks, void* ws, size_t ws_bytes,
                                    hipStream_t stream) {
    PSAM_REQUIRE(plan && prepared && keys && idx3 && w3 && hyper && masks && ws, PSAM_EINVAL, "psam_upscale_masks: null pointer");
    const int E = plan->dim, a = kpad32(E);
    PSAM_REQUIRE(rep > 0 && Z > 0 && Z % rep == 0 && N > 0 && G > 0 && C > 0 && C <= 4 && (Z * N) % 256 == 0 && N % 32 == 0 && Z * N < ((int64_t)1 << 31), PSAM_EINVAL,
                 "psam_upscale_masks: need Z * N % 256 == 0, N % 32 == 0, C <= 4");
    PSAM_REQUIRE(ws_bytes >= psam_upscale_masks_ws_bytes(Z, N, G, C, E), PSAM_EWORKSPACE, "psam_upscale_masks: workspace too small");
    auto P = [&](int64_t off) { return at(prepared, off); };
    const int planes = psam_gemm_f16x3p_hyper_planes(E, 0);
    const int64_t count = Z * C * N;
    Carve cv(ws);
    const UpscaleWs w = upscale_ws(cv, Z, N, G, C, E);
    const Lin u0{plan->u0_w, E, plan->u0_b, P(plan->o_w0), P(plan->o_s0), E, E};
    int32_t rc = host_linear(u0, keys, Z * G, w.k1, 0, G, w.kp, w.sk, stream);
    if (rc) return rc;
    rc = psam_interp3_ex(w.k1, idx3, w3, w.up, rep, Z, N, G, E, w.s1, plan->u1_w, plan->u1_b, plan->eps, PSAM_ACT_GELU, stream);
    if (rc) return rc;
    psam_gemm_fuse_t f;
    std::memset(&f, 0, sizeof(f));
    f.hyper = hyper; f.masks = planes > 1 ? w.parts : masks; f.hyper_c = C; f.hyper_rows = N; f.hyper_pstride = count; f.no_store = 1;
    rc = psam_gemm_f16x3p_ex(w.up, a, w.s1, P(plan->o_w3), a, P(plan->o_s3), masks, E, plan->u3_b, nullptr, 0, nullptr, 0, 0, (int32_t)(Z * N), E, a, 1.f, PSAM_ACT_GELU, &f, stream);
    if (rc || planes <= 1) return rc;
    return psam_sum_planes(w.parts, planes, count, count, masks, stream);
}

// ================================================================================================================================
// psam_twoway_decoder: TwoWayTransformer.forward (pc_sam/model/transformer.py:61-100; blocks :144-176, Attention :214-236) -- the decoder's
// transformer over the patch tokens (`keys`, Z*G rows) and the output / prompt tokens (Z*T rows) -- sequenced by the library exactly as the Python
// host sequences it: per nn.Linear the kernel the host would pick (host_linear: <= 64 rows: psam_linear_skinny; >= 256 rows and N, K >= 128: the
// packed-operand "f16x3" GEMM on a weight packed at prepare time; otherwise psam_linear), psam_attention_small for every attention, psam_layernorm
// with the residual folded in, psam_add_bcast for the positional additions.  (The one-launch token-side kernel psam_twoway_tokens is slower than
// these launches, DESIGN.md 4.4, so it is not used here.)
// ================================================================================================================================
namespace {
// The Linears of the transformer in the order _prepare packs them, which is the order of their slots in the plan (o_packed / o_scales): 14 per layer,
// then the four of the final attention (whose `layer` is the depth)
enum TwSlot {
    TW_SELF_Q, TW_SELF_K, TW_SELF_V, TW_SELF_O,      // self_attn
    TW_T2I_Q, TW_T2I_K, TW_T2I_V, TW_T2I_O,          // cross_attn_token_to_image
    TW_MLP_1, TW_MLP_2,
    TW_I2T_Q, TW_I2T_K, TW_I2T_V, TW_I2T_O,          // cross_attn_image_to_token
    TW_PER_LAYER,
    TW_FINAL_Q = TW_PER_LAYER, TW_FINAL_K, TW_FINAL_V, TW_FINAL_O, TW_FINAL_END      // final_attn_token_to_image
};
constexpr int TW_MAX_LINEARS = TW_PER_LAYER * PSAM_TWOWAY_MAX_DEPTH + (TW_FINAL_END - TW_FINAL_Q);
static_assert(sizeof(psam_twoway_plan_t::o_packed) == TW_MAX_LINEARS * sizeof(int64_t) && sizeof(psam_twoway_plan_t::o_scales) == sizeof(psam_twoway_plan_t::o_packed),
              "psam_twoway_plan_t holds one packed weight per Linear");
constexpr int tw_index(int depth, int layer, int slot) { return slot < TW_PER_LAYER ? TW_PER_LAYER * layer + slot : TW_PER_LAYER * depth + slot - TW_FINAL_Q; }
template <typename F> void tw_for_each(int depth, F&& f) {      // every (layer, slot), in slot order
    for (int i = 0; i < depth; ++i)
        for (int s = 0; s < TW_PER_LAYER; ++s) f(i, s);
    for (int s = TW_FINAL_Q; s < TW_FINAL_END; ++s) f(depth, s);
}
// Shape, weight and bias of one Linear (layers == nullptr: the shape alone): q / k / v project E -> inner, out_proj inner -> E; inner = E in the
// self-attention and E / downsample in the other attentions
Lin tw_linear(const psam_twoway_weights_t& W, const psam_twoway_layer_weights_t* layers, int layer, int slot) {
    static const psam_twoway_layer_weights_t none{};
    const int E = W.dim, IX = W.dim / W.downsample;
    const psam_twoway_layer_weights_t& L = layers && slot < TW_PER_LAYER ? layers[layer] : none;
    if (slot == TW_MLP_1) return Lin{L.m1_w, E, L.m1_b, nullptr, nullptr, W.mlp, E};
    if (slot == TW_MLP_2) return Lin{L.m2_w, W.mlp, L.m2_b, nullptr, nullptr, E, W.mlp};
    const psam_attn_weights_t& a = slot >= TW_FINAL_Q ? W.final_attn : slot < TW_T2I_Q ? L.self_attn : slot < TW_MLP_1 ? L.t2i : L.i2t;
    const int inner = slot < TW_T2I_Q ? E : IX;
    switch ((slot >= TW_FINAL_Q ? slot - TW_FINAL_Q : slot < TW_MLP_1 ? slot : slot - TW_I2T_Q) & 3) {
        case 0: return Lin{a.q_w, E, a.q_b, nullptr, nullptr, inner, E};
        case 1: return Lin{a.k_w, E, a.k_b, nullptr, nullptr, inner, E};
        case 2: return Lin{a.v_w, E, a.v_b, nullptr, nullptr, inner, E};
        default: return Lin{a.o_w, inner, a.o_b, nullptr, nullptr, E, inner};
    }
}

struct TwPrepared {
    Packed lin[TW_MAX_LINEARS];
    Packed cat[PSAM_TWOWAY_MAX_DEPTH]; float* cat_bias[PSAM_TWOWAY_MAX_DEPTH];      // per layer: [t2i.k_proj | i2t.q_proj] as one weight (they share their input rows), its bias
};
TwPrepared tw_prepared(Carve& cv, const psam_twoway_weights_t& W) {      // reads the dimensions of W only; W.depth <= PSAM_TWOWAY_MAX_DEPTH
    const int IX = W.dim / W.downsample;
    TwPrepared p;
    tw_for_each(W.depth, [&](int layer, int slot) {
        const Lin l = tw_linear(W, nullptr, layer, slot);
        p.lin[tw_index(W.depth, layer, slot)] = take_packed(cv, l.N, l.K);
    });
    for (int i = 0; i < W.depth; ++i) { p.cat[i] = take_packed(cv, 2 * IX, W.dim); p.cat_bias[i] = cv.take<float>(2 * IX); }
    return p;
}

struct TwWs { float *q, *pq, *pk, *pv, *ta, *ty, *tm, *k, *ik, *iv, *iq, *ia, *iy, *pack_buf, *scale_buf, *kin_p, *kin_s, *nq, *nk, *nv, *lntmp, *kv_p, *kv_s; };
TwWs tw_ws(Carve& cv, int64_t Z, int T, int G, int dim, int mlp) {
    const int64_t R = Z * T, I = Z * G, E = dim, big = std::max(R, I);
    TwWs b;
    b.q = cv.take<float>(R * E); b.pq = cv.take<float>(R * E); b.pk = cv.take<float>(R * E); b.pv = cv.take<float>(R * E);      // token rows: queries + query_pe, projections
    b.ta = cv.take<float>(R * E); b.ty = cv.take<float>(R * E); b.tm = cv.take<float>(R * mlp);                                // attention output, Linear output, MLP hidden rows
    b.k = cv.take<float>(I * E); b.ik = cv.take<float>(I * E); b.iv = cv.take<float>(I * E); b.iq = cv.take<float>(I * E);      // patch rows: keys + key_pe, projections
    b.ia = cv.take<float>(I * E); b.iy = cv.take<float>(I * E);
    b.pack_buf = cv.take<float>(big * kpad32(std::max(mlp, dim))); b.scale_buf = cv.take<float>(big);                            // host_linear's packed input rows
    b.kin_p = cv.take<float>(I * kpad32(dim)); b.kin_s = cv.take<float>(I);      // the packed keys + key_pe rows (shared by two projections per layer) and their scales
    b.nq = cv.take<float>(R * E); b.nk = cv.take<float>(R * E); b.nv = cv.take<float>(R * E); b.lntmp = cv.take<float>(8 * R * 256);      // regrouped sequence: next projections, Linear + LN scratch
    b.kv_p = cv.take<float>(I * kpad32(dim)); b.kv_s = cv.take<float>(I);        // regrouped sequence: the packed keys rows
    return b;
}

// The two-way transformer has two chains per layer that do not depend on each other: the token side (self-attention, norm1, the q projection of
// the token -> patch attention; later the token MLP) and the projections of the PATCH rows (keys + key_pe packed once, k / v of token -> patch, q of
// patch -> token).  psam_twoway_decoder issues the patch-side chain on a side stream forked from the caller's stream by an event and joins it (two
// events) where its results are consumed -- inside a graph capture the side stream joins the capture and the graph gets two parallel branches.
// Same kernels on the same data: same bits.  One side stream + three events per (device, caller stream), created on first use outside a capture
// (a captured call on a stream that has none yet runs the serial sequence).
// MEASURED SLOWER, so OFF by default (PSAM_TWOWAY_FORK=1 / psam_twoway_decoder_force_fork(1) switch it on): the event hand-overs cost more than the
// six short launches they take off the critical path -- eager two-way stage 0.43 -> 0.43 ms (no gain), and inside captured graphs every fork / join
// splits the graph into segments: cfg #2 792 -> 704 clouds/s, cfg #5 131 -> 94 sessions/s, a replayed click 0.61 -> 1.27 ms (profiles/r04/r04_twoway_fork.txt).
struct TwSide { hipStream_t side; hipEvent_t fork, join1, join2; };
psam_knob k_tw_fork("PSAM_TWOWAY_FORK", 0);      // read by experiments builds only
const TwSide* tw_side(hipStream_t stream) {
#ifndef PSAM_BUILD_EXPERIMENTS
    (void)stream;
    return nullptr;      // the forked form lost (profiles/r04/r04_twoway_fork.txt): the default build creates no streams or events and keeps no per-stream state
#else
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, TwSide> table;
    if (k_tw_fork.get() == 0) return nullptr;
    int dev = 0;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipGetDevice(&dev) != hipSuccess || hipStreamIsCapturing(stream, &cs) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    auto it = table.find({dev, stream});
    if (it != table.end()) return &it->second;
    if (cs != hipStreamCaptureStatusNone) return nullptr;
    TwSide t;
    if (hipStreamCreateWithFlags(&t.side, hipStreamNonBlocking) != hipSuccess) return nullptr;
    if (hipEventCreateWithFlags(&t.fork, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&t.join1, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&t.join2, hipEventDisableTiming) != hipSuccess) return nullptr;
    return &(table[{dev, stream}] = t);
#endif
}

// The launch sequence of psam_twoway_decoder: 0 the operator-by-operator sequence, 1 regrouped with packed-operand GEMMs on the patch side, 2 (default)
// regrouped with the exact-fp32 row kernel there.  psam_twoway_decoder_force_fast: -1 = environment PSAM_TWOWAY_FAST, otherwise the mode.
psam_knob k_tw_fast("PSAM_TWOWAY_FAST", 2);
}  // namespace

#ifdef PSAM_BUILD_EXPERIMENTS
PSAM_API void psam_twoway_decoder_force_fork(int32_t mode) { k_tw_fork.force(mode); }
#endif
PSAM_API void psam_twoway_decoder_force_fast(int32_t mode) { k_tw_fast.force(mode); }

PSAM_API size_t psam_twoway_decoder_prepared_bytes(int32_t depth, int32_t dim, int32_t mlp, int32_t downsample) {
    if (depth <= 0 || depth > PSAM_TWOWAY_MAX_DEPTH || dim <= 0 || mlp <= 0 || downsample <= 0) return 0;
    psam_twoway_weights_t W{};
    W.depth = depth; W.dim = dim; W.mlp = mlp; W.downsample = downsample;
    return carved_bytes([&](Carve& cv) { tw_prepared(cv, W); });
}

PSAM_API int32_t psam_twoway_decoder_prepare(const psam_twoway_weights_t* wt, psam_twoway_plan_t* plan, void* prepared, size_t prepared_bytes, hipStream_t stream) {
#define WHO "psam_twoway_decoder_prepare"
    PSAM_REQUIRE(wt && plan && prepared && wt->layers, PSAM_EINVAL, WHO ": null pointer");
    PSAM_REQUIRE(wt->depth > 0 && wt->depth <= PSAM_TWOWAY_MAX_DEPTH && wt->dim > 0 && wt->dim % 32 == 0 && wt->heads > 0 && wt->mlp > 0 && wt->mlp % 32 == 0 && wt->downsample > 0 &&
                     wt->dim % wt->downsample == 0 && (wt->dim / wt->downsample) % wt->heads == 0 && wt->dim % wt->heads == 0,
                 PSAM_EINVAL, WHO ": bad dimensions");
    PSAM_REQUIRE(prepared_bytes >= psam_twoway_decoder_prepared_bytes(wt->depth, wt->dim, wt->mlp, wt->downsample), PSAM_EWORKSPACE, WHO ": prepared buffer too small");
    std::memset(plan, 0, sizeof(*plan));
    plan->weights = *wt;
    for (int i = 0; i < wt->depth; ++i) plan->layers[i] = wt->layers[i];
    plan->weights.layers = nullptr;      // the plan carries its own copy of the per-layer pointer blocks
    const int E = wt->dim, IX = wt->dim / wt->downsample, kp = kpad32(E);
    Carve cv(prepared);
    const TwPrepared p = tw_prepared(cv, *wt);
    int32_t rc = PSAM_OK;
    tw_for_each(wt->depth, [&](int layer, int slot) {
        const int i = tw_index(wt->depth, layer, slot);
        const Lin l = tw_linear(*wt, wt->layers, layer, slot);
        put_offsets(cv, p.lin[i], &plan->o_packed[i], &plan->o_scales[i]);
        if (!rc) rc = pack_weight(WHO, l.w, l.ldw, l.N, l.K, p.lin[i], stream);
    });
    // k_proj of cross_attn_token_to_image and q_proj of cross_attn_image_to_token both read keys + key_pe (transformer.py:160-175): one [2 IX, E] weight
    for (int i = 0; i < wt->depth && !rc; ++i) {
        put_offsets(cv, p.cat[i], &plan->o_cat_packed[i], &plan->o_cat_scales[i]); plan->o_cat_bias[i] = cv.offset_of(p.cat_bias[i]);
        const Lin halves[2] = {tw_linear(*wt, wt->layers, i, TW_T2I_K), tw_linear(*wt, wt->layers, i, TW_I2T_Q)};
        for (int h = 0; h < 2 && !rc; ++h) {
            if (!halves[h].b) { rc = fail(WHO, "null weight pointer"); break; }
            rc = pack_weight(WHO, halves[h].w, E, IX, E, Packed{p.cat[i].w + (int64_t)h * IX * kp, p.cat[i].s + h * IX}, stream);
            if (!rc && hipMemcpyAsync(p.cat_bias[i] + h * IX, halves[h].b, (size_t)IX * 4, hipMemcpyDeviceToDevice, stream) != hipSuccess) rc = fail(WHO, "bias copy failed");
        }
    }
    return packing_done(WHO, rc, stream);
#undef WHO
}

PSAM_API size_t psam_twoway_decoder_ws_bytes(int64_t Z, int32_t T, int32_t G, int32_t dim, int32_t mlp) {
    if (Z <= 0 || T <= 0 || G <= 0 || dim <= 0 || mlp <= 0) return 0;
    return carved_bytes([&](Carve& cv) { tw_ws(cv, Z, T, G, dim, mlp); });
}

// tokens [Z*T, dim] (output tokens + sparse prompt embeddings = the point embedding `query_pe`), keys [Z*G, dim] (src = image embedding + dense
// prompt; UPDATED IN PLACE to the transformer's second output), pos [Z / rep, G, dim] (image positional encoding, shared by the rep prompt sets of
// a cloud) -> queries [Z*T, dim] (the transformer's first output)
PSAM_API int32_t psam_twoway_decoder(const psam_twoway_plan_t* plan, const void* prepared, const float* tokens, float* keys, const float* pos, int32_t rep,
                                     int64_t Z, int32_t T, int32_t G, float* queries, void* ws, size_t ws_bytes, int32_t* counters, hipStream_t stream) {
    PSAM_REQUIRE(plan && prepared && tokens && keys && pos && queries && ws, PSAM_EINVAL, "psam_twoway_decoder: null pointer");
    const psam_twoway_weights_t& W = plan->weights;
    const int E = W.dim, IX = W.dim / W.downsample, H = W.heads, mlp = W.mlp;
    const int64_t R = Z * T, I = Z * G;
    PSAM_REQUIRE(rep > 0 && Z > 0 && Z % rep == 0 && T > 0 && G > 0 && R < ((int64_t)1 << 31) && I < ((int64_t)1 << 31), PSAM_EINVAL, "psam_twoway_decoder: bad shape");
    // every attention is psam_attention_small, whose scores of one query live in LDS (Lk * 16 <= 128 KiB): refused here, before the first launch
    PSAM_REQUIRE(T <= 8192 && G <= 8192, PSAM_EINVAL, "psam_twoway_decoder: at most 8192 tokens and 8192 patch tokens per prompt set (psam_attention_small)");
    PSAM_REQUIRE(ws_bytes >= psam_twoway_decoder_ws_bytes(Z, T, G, E, mlp), PSAM_EWORKSPACE, "psam_twoway_decoder: workspace too small");
    // Linear `slot` of `layer` (the final attention: layer = depth) with the packed form _prepare made of it (matrices of at least 128 x 128)
    auto lin = [&](int layer, int slot) {
        Lin l = tw_linear(W, plan->layers, layer, slot);
        const int i = tw_index(W.depth, layer, slot);
        if (l.N >= 128 && l.K >= 128) { l.packed = at(prepared, plan->o_packed[i]); l.scales = at(prepared, plan->o_scales[i]); }
        return l;
    };
    Carve cv(ws);
    const TwWs b = tw_ws(cv, Z, T, G, E, mlp);
    int32_t rc = PSAM_OK;
    // Round 4, fewer and wider launches with the same arithmetic (the same bits as the per-operator sequence the Python host issues):
    //  * token side (R <= 64 rows): the q / k / v projections of an attention are ONE psam_linear_skinny_multi launch, `queries + query_pe` is added
    //    while the rows are loaded -- no psam_add_bcast, no separate launches;
    //  * patch side: `keys + key_pe` is added inside the pass that scales and packs the rows (psam_scale_pack_rows_g8_add), and the packed rows feed
    //    BOTH projections that read them in a layer (k of tokens -> patches, q of patches -> tokens): one pack instead of an add and two packs.
    const bool tok_fast = R <= 64 && (E & 15) == 0;
    // y [M, N] = act(x W^T + b): the host's dispatch, never the row kernel (the Python host's operator sequence has none)
    auto linear = [&](const Lin& l, const float* x, int64_t M, float* y, int act, hipStream_t s) -> int32_t { return host_linear(l, x, M, y, act, 0, b.pack_buf, b.scale_buf, s); };
    // Linears on the R token rows (K = E each) as one launch, xadd added to the rows on load
    auto tok_multi = [&](std::initializer_list<Job> js) -> int32_t {
        const psam_skinny_jobs_t jobs = skinny_jobs(js);
        return psam_linear_skinny_multi(&jobs, E, E, E, (int32_t)R, E, stream);
    };
    auto gemm_packed = [&](const Lin& l, const float* xp, const float* sx, int64_t M, float* y, hipStream_t s) -> int32_t {
        const int kp = kpad32(l.K);
        return psam_gemm_f16x3p_ex(xp, kp, sx, l.packed, kp, l.scales, y, l.N, l.b, nullptr, 0, nullptr, 0, 0, (int32_t)M, l.N, kp, 1.f, 0, nullptr, s);
    };
    // k_in = keys + pos, packed: shared by every projection of the layer that reads it (needs I >= 256 and packed weights)
    auto pack_kin = [&](hipStream_t s) -> int32_t { return psam_scale_pack_rows_g8_add(keys, E, pos, E, G, rep, (int32_t)I, E, b.kin_p, kpad32(E), b.kin_s, s); };
    // softmax(q k^T / sqrt(hd)) v of projected rows (row strides ldq / ldk / ldv; out dense)
    auto sattn = [&](int inner, const float* oq, int64_t ldq, const float* ok, int64_t ldk, const float* ov, int64_t ldv, float* out, int Lq, int Lk) -> int32_t {
        return psam_attention_small(oq, ldq, Lq * ldq, ok, ldk, Lk * ldk, ov, ldv, Lk * ldv, out, inner, (int64_t)Lq * inner, Z, H, Lq, Lk, inner / H,
                                    1.0f / std::sqrt((float)(inner / H)), stream);
    };
#define TWCK(call) do { rc = (call); if (rc) return rc; } while (0)
#define TWHIP(call) do { if ((call) != hipSuccess) { psam_set_error("psam_twoway_decoder: stream fork / join failed"); return PSAM_EINVAL; } } while (0)
    const TwSide* sd = tok_fast ? tw_side(stream) : nullptr;      // patch-side projections on a forked side stream (see TwSide)
    const int tw_fast = k_tw_fast.get();
    // ---- Round 5: the short sequence (36 launches for depth 2 against 50; profiles/r05/r05_click_kernels_*.txt).  Same operators, regrouped along their
    // data dependences:
    //  * every `queries = norm(queries + Linear(..))` of the token side is ONE launch (psam_linear_skinny_ln: the last workgroup of the Linear
    //    normalises the rows; lin2 of the MLP, K = 2048, split over 8 workgroup rows instead of walking K in 16 dependent rounds);
    //  * the token projections that read the layer's final `queries` -- k / v of patches -> tokens AND the next layer's self-attention q / k / v (or
    //    the final attention's q) -- are one psam_linear_skinny_multi launch (the patch -> token attention in between only changes `keys`);
    //  * patch side: keys + key_pe and keys are packed in one pass (psam_scale_pack_rows_g8_add_dual), the k projection of tokens -> patches and the
    //    q projection of patches -> tokens are one GEMM on the concatenated weight (both read keys + key_pe).
    // Needs the caller's arrival-counter block (`counters`) and embedding_dim 256.
    const bool fast = tok_fast && !sd && tw_fast != 0 && E == 256 && IX >= 128 && 2 * IX <= E && IX <= 512 && I >= 256 && (mlp & 15) == 0 && (IX & 15) == 0 &&
                      plan->o_cat_packed[0] != 0 && counters != nullptr;
    if (fast) {
        auto lin_ln = [&](const Lin& l, const float* x, const float* res, const float* nw, const float* nb) -> int32_t {
            return psam_linear_skinny_ln(x, l.K, l.w, l.K, l.b, res, E, nw, nb, W.eps, b.lntmp, queries, E, (int32_t)R, E, l.K, counters, stream);
        };
        const bool small_rows = tw_fast >= 2 && rows_multi_fits(G, E);
        // Linears on the I patch rows (`keys`, key_pe added on load where xadd = pos) as one launch of the exact-fp32 row kernel
        auto rows_multi = [&](std::initializer_list<Job> js) -> int32_t {
            const psam_skinny_jobs_t jobs = skinny_jobs(js);
            return psam_linear_rows_multi(&jobs, E, E, G, rep, E, I, E, stream);
        };
        auto dual_pack = [&]() -> int32_t { return psam_scale_pack_rows_g8_add_dual(keys, E, pos, E, G, rep, (int32_t)I, E, b.kin_p, b.kin_s, b.kv_p, b.kv_s, kpad32(E), stream); };
        float *aq = b.pq, *ak = b.pk, *av = b.pv;      // self-attention projections of the layer at hand
        float *cqo = b.nq, *jko = b.nk, *jvo = b.nv;   // q of tokens -> patches (and of the final attention); k / v of patches -> tokens
        {   // first layer: q = k = v = the tokens, no positional encoding (skip_first_layer_pe)
            const Lin sq = lin(0, TW_SELF_Q), sk = lin(0, TW_SELF_K), sv = lin(0, TW_SELF_V);
            TWCK(tok_multi({{&sq, tokens, nullptr, aq}, {&sk, tokens, nullptr, ak}, {&sv, tokens, nullptr, av}}));
        }
        for (int i = 0; i < W.depth; ++i) {
            const psam_twoway_layer_weights_t& Lw = plan->layers[i];
            const Lin so = lin(i, TW_SELF_O), cq = lin(i, TW_T2I_Q), cvl = lin(i, TW_T2I_V), co = lin(i, TW_T2I_O), m1 = lin(i, TW_MLP_1), m2 = lin(i, TW_MLP_2);
            const Lin jk = lin(i, TW_I2T_K), jv = lin(i, TW_I2T_V), jo = lin(i, TW_I2T_O);
            const Lin cat{nullptr, E, at(prepared, plan->o_cat_bias[i]), at(prepared, plan->o_cat_packed[i]), at(prepared, plan->o_cat_scales[i]), 2 * IX, E};
            // patch side: k of tokens -> patches | q of patches -> tokens (both from keys + key_pe; ik: row stride 2 IX) and v (from keys)
            if (small_rows) {      // one launch, exact fp32 products, key_pe added on load
                const Lin ck = lin(i, TW_T2I_K), jq = lin(i, TW_I2T_Q);
                TWCK(rows_multi({{&ck, keys, pos, b.ik, 2 * IX}, {&jq, keys, pos, b.ik + IX, 2 * IX}, {&cvl, keys, nullptr, b.iv}}));
            } else {               // both packed forms of the keys in one pass, [k | q] as one GEMM on the concatenated weight
                TWCK(dual_pack());
                TWCK(gemm_packed(cat, b.kin_p, b.kin_s, I, b.ik, stream));
                TWCK(gemm_packed(cvl, b.kv_p, b.kv_s, I, b.iv, stream));
            }
            // self-attention of the tokens + norm1 (the first layer replaces the queries: no residual)
            TWCK(sattn(E, aq, E, ak, E, av, E, b.ta, T, T));
            TWCK(lin_ln(so, b.ta, i == 0 ? nullptr : queries, Lw.n1_w, Lw.n1_b));
            // tokens attend to the patch tokens + norm2
            TWCK(tok_multi({{&cq, queries, tokens, cqo}}));
            TWCK(sattn(IX, cqo, IX, b.ik, 2 * IX, b.iv, IX, b.ta, T, G));
            TWCK(lin_ln(co, b.ta, queries, Lw.n2_w, Lw.n2_b));
            // token MLP + norm3
            TWCK(psam_linear_skinny(queries, E, m1.w, E, m1.b, nullptr, 0, b.tm, mlp, (int32_t)R, mlp, E, PSAM_ACT_RELU, stream));
            TWCK(lin_ln(m2, b.tm, queries, Lw.n3_w, Lw.n3_b));
            // every projection of the finished queries: k / v of patches -> tokens, and what the NEXT attention of the token side needs
            if (i + 1 < W.depth) {
                const Lin nsq = lin(i + 1, TW_SELF_Q), nsk = lin(i + 1, TW_SELF_K), nsv = lin(i + 1, TW_SELF_V);
                TWCK(tok_multi({{&jk, queries, tokens, jko}, {&jv, queries, nullptr, jvo}, {&nsq, queries, tokens, aq}, {&nsk, queries, tokens, ak}, {&nsv, queries, nullptr, av}}));
            } else {
                const Lin fq = lin(W.depth, TW_FINAL_Q);
                TWCK(tok_multi({{&jk, queries, tokens, jko}, {&jv, queries, nullptr, jvo}, {&fq, queries, tokens, cqo}}));
            }
            // patch tokens attend to the tokens + norm4
            TWCK(sattn(IX, b.ik + IX, 2 * IX, jko, IX, jvo, IX, b.ia, G, T));
            TWCK(psam_linear_ln256(b.ia, IX, jo.w, IX, jo.b, keys, E, Lw.n4_w, Lw.n4_b, W.eps, keys, E, I, E, IX, stream));      // out_proj + residual + norm4: one launch, 16 whole rows per workgroup
        }
        const Lin fk = lin(W.depth, TW_FINAL_K), fv = lin(W.depth, TW_FINAL_V), fo = lin(W.depth, TW_FINAL_O);
        if (small_rows) {
            TWCK(rows_multi({{&fk, keys, pos, b.ik}, {&fv, keys, nullptr, b.iv}}));
        } else {
            TWCK(dual_pack());
            TWCK(gemm_packed(fk, b.kin_p, b.kin_s, I, b.ik, stream));
            TWCK(gemm_packed(fv, b.kv_p, b.kv_s, I, b.iv, stream));
        }
        TWCK(sattn(IX, cqo, IX, b.ik, IX, b.iv, IX, b.ta, T, G));
        TWCK(lin_ln(fo, b.ta, queries, W.nf_w, W.nf_b));
        return PSAM_OK;
    }
    // ---- the operator sequence
    // Attention.forward up to out_proj: projections + softmax(q k^T / sqrt(hd)) v
    auto attn = [&](const Lin& lq, const Lin& lk, const Lin& lv, const float* q_in, int64_t Mq, const float* k_in, const float* v_in, int64_t Mk, float* oq, float* ok,
                    float* ov, float* out, int Lq, int Lk) -> int32_t {
        int32_t r = linear(lq, q_in, Mq, oq, 0, stream);
        if (!r) r = linear(lk, k_in, Mk, ok, 0, stream);
        if (!r) r = linear(lv, v_in, Mk, ov, 0, stream);
        if (!r) r = sattn(lq.N, oq, lq.N, ok, lq.N, ov, lq.N, out, Lq, Lk);
        return r;
    };
    // queries + query_pe / keys + key_pe as rows of their own (b.q / b.k), where no kernel adds the positional encoding while it loads the rows
    auto add_query_pe = [&]() -> int32_t { return psam_add_bcast(queries, (int64_t)T * E, 1, tokens, (int64_t)T * E, E, b.q, (int64_t)T * E, Z, T, E, stream); };
    auto add_key_pe = [&]() -> int32_t { return psam_add_bcast(pos, (int64_t)G * E, rep, keys, (int64_t)G * E, E, b.k, (int64_t)G * E, Z, G, E, stream); };
    const float* cur = tokens;      // queries start as the tokens themselves (transformer.py:84)
    for (int i = 0; i < W.depth; ++i) {
        const psam_twoway_layer_weights_t& Lw = plan->layers[i];
        const Lin sq = lin(i, TW_SELF_Q), sk = lin(i, TW_SELF_K), sv = lin(i, TW_SELF_V), so = lin(i, TW_SELF_O);
        const Lin cq = lin(i, TW_T2I_Q), ck = lin(i, TW_T2I_K), cvl = lin(i, TW_T2I_V), co = lin(i, TW_T2I_O), m1 = lin(i, TW_MLP_1), m2 = lin(i, TW_MLP_2);
        const Lin jq = lin(i, TW_I2T_Q), jk = lin(i, TW_I2T_K), jv = lin(i, TW_I2T_V), jo = lin(i, TW_I2T_O);
        const bool key_fast = I >= 256 && ck.packed && jq.packed && cvl.packed;
        const bool fork = sd && key_fast;
        if (fork) {      // keys (as the previous layer left them) -> k_in packed, k / v for token -> patch, q for patch -> token: beside the token chain below
            TWHIP(hipEventRecord(sd->fork, stream));
            TWHIP(hipStreamWaitEvent(sd->side, sd->fork, 0));
            TWCK(pack_kin(sd->side));
            TWCK(gemm_packed(ck, b.kin_p, b.kin_s, I, b.ik, sd->side));
            TWCK(linear(cvl, keys, I, b.iv, 0, sd->side));
            TWHIP(hipEventRecord(sd->join1, sd->side));
            TWCK(gemm_packed(jq, b.kin_p, b.kin_s, I, b.iq, sd->side));
            TWHIP(hipEventRecord(sd->join2, sd->side));
        }
        // self-attention of the tokens (the first layer without positional encoding and without residual: skip_first_layer_pe)
        if (tok_fast) {
            const float* pe = i == 0 ? nullptr : tokens;
            TWCK(tok_multi({{&sq, cur, pe, b.pq}, {&sk, cur, pe, b.pk}, {&sv, cur, nullptr, b.pv}}));
            TWCK(sattn(E, b.pq, E, b.pk, E, b.pv, E, b.ta, T, T));
        } else if (i == 0) {
            TWCK(attn(sq, sk, sv, cur, R, cur, cur, R, b.pq, b.pk, b.pv, b.ta, T, T));
        } else {
            TWCK(add_query_pe());
            TWCK(attn(sq, sk, sv, b.q, R, b.q, queries, R, b.pq, b.pk, b.pv, b.ta, T, T));
        }
        TWCK(linear(so, b.ta, R, b.ty, 0, stream));
        TWCK(psam_layernorm(b.ty, E, i == 0 ? nullptr : queries, i == 0 ? 0 : E, Lw.n1_w, Lw.n1_b, queries, E, R, E, W.eps, 0, stream));
        cur = queries;
        // tokens attend to the patch tokens
        if (tok_fast) {
            TWCK(tok_multi({{&cq, queries, tokens, b.pq}}));
        } else {
            TWCK(add_query_pe());
            TWCK(linear(cq, b.q, R, b.pq, 0, stream));
        }
        if (fork) {
            TWHIP(hipStreamWaitEvent(stream, sd->join1, 0));
        } else {
            if (key_fast) {
                TWCK(pack_kin(stream));
                TWCK(gemm_packed(ck, b.kin_p, b.kin_s, I, b.ik, stream));
            } else {
                TWCK(add_key_pe());
                TWCK(linear(ck, b.k, I, b.ik, 0, stream));
            }
            TWCK(linear(cvl, keys, I, b.iv, 0, stream));
        }
        TWCK(sattn(IX, b.pq, IX, b.ik, IX, b.iv, IX, b.ta, T, G));
        TWCK(linear(co, b.ta, R, b.ty, 0, stream));
        TWCK(psam_layernorm(b.ty, E, queries, E, Lw.n2_w, Lw.n2_b, queries, E, R, E, W.eps, 0, stream));
        // token MLP
        TWCK(linear(m1, queries, R, b.tm, PSAM_ACT_RELU, stream));
        TWCK(linear(m2, b.tm, R, b.ty, 0, stream));
        TWCK(psam_layernorm(b.ty, E, queries, E, Lw.n3_w, Lw.n3_b, queries, E, R, E, W.eps, 0, stream));
        // patch tokens attend to the tokens
        if (fork) TWHIP(hipStreamWaitEvent(stream, sd->join2, 0));
        else if (key_fast) TWCK(gemm_packed(jq, b.kin_p, b.kin_s, I, b.iq, stream));      // keys + key_pe: packed once above, unchanged since
        else TWCK(linear(jq, b.k, I, b.iq, 0, stream));
        if (tok_fast) {
            TWCK(tok_multi({{&jk, queries, tokens, b.pk}, {&jv, queries, nullptr, b.pv}}));
        } else {
            TWCK(add_query_pe());
            TWCK(linear(jk, b.q, R, b.pk, 0, stream));
            TWCK(linear(jv, queries, R, b.pv, 0, stream));
        }
        TWCK(sattn(IX, b.iq, IX, b.pk, IX, b.pv, IX, b.ia, G, T));
        TWCK(linear(jo, b.ia, I, b.iy, 0, stream));
        TWCK(psam_layernorm(b.iy, E, keys, E, Lw.n4_w, Lw.n4_b, keys, E, I, E, W.eps, 0, stream));
    }
    // the final attention of the tokens to the patch tokens
    const Lin fq = lin(W.depth, TW_FINAL_Q), fk = lin(W.depth, TW_FINAL_K), fv = lin(W.depth, TW_FINAL_V), fo = lin(W.depth, TW_FINAL_O);
    const bool fork = sd && I >= 256 && fk.packed && fv.packed;
    if (fork) {
        TWHIP(hipEventRecord(sd->fork, stream));
        TWHIP(hipStreamWaitEvent(sd->side, sd->fork, 0));
        TWCK(pack_kin(sd->side));
        TWCK(gemm_packed(fk, b.kin_p, b.kin_s, I, b.ik, sd->side));
        TWCK(linear(fv, keys, I, b.iv, 0, sd->side));
        TWHIP(hipEventRecord(sd->join1, sd->side));
    }
    if (tok_fast) {
        TWCK(tok_multi({{&fq, queries, tokens, b.pq}}));
    } else {
        TWCK(add_query_pe());
        TWCK(linear(fq, b.q, R, b.pq, 0, stream));
    }
    if (fork) {
        TWHIP(hipStreamWaitEvent(stream, sd->join1, 0));
    } else {
        if (I >= 256 && fk.packed) {
            TWCK(pack_kin(stream));
            TWCK(gemm_packed(fk, b.kin_p, b.kin_s, I, b.ik, stream));
        } else {
            TWCK(add_key_pe());
            TWCK(linear(fk, b.k, I, b.ik, 0, stream));
        }
        TWCK(linear(fv, keys, I, b.iv, 0, stream));
    }
    TWCK(sattn(IX, b.pq, IX, b.ik, IX, b.iv, IX, b.ta, T, G));
    TWCK(linear(fo, b.ta, R, b.ty, 0, stream));
    TWCK(psam_layernorm(b.ty, E, queries, E, W.nf_w, W.nf_b, queries, E, R, E, W.eps, 0, stream));
#undef TWCK
#undef TWHIP
    return PSAM_OK;
}
