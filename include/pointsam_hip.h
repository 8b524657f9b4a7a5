/*
 * pointsam_hip.h -- C ABI of libpointsam_hip.so (gfx950 / MI355X), the drop-in boundary for the Point-SAM
 * inference hot path (encode + prompt decode).
 *
 * The reference (zyc00/Point-SAM) has no FFI of its own: its "operator API" for this path is the set of Python
 * call sites into third-party native code and ATen.  Each entry point below names the reference interface it
 * replaces (file:line under the reference checkout).  The Python host (point_sam_amd/ops.py) binds these with
 * ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer valid on `stream`; calls are asynchronous and never allocate;
 *   - tensors are fp32 row-major unless stated; indices are int64 (torch.long) as in the reference;
 *   - return value: 0 = ok, < 0 = invalid argument (PSAM_E*), > 0 = hipError_t of the failed launch;
 *     psam_last_error_string() describes the last failure on the calling thread;
 *   - thread-safe for distinct streams / workspaces.  The psam_*_force_* / psam_*_set_* hooks are process-wide atomic switches (csrc/knob.h; the table
 *     of all of them with their environment variables: INTEGRATION.md): any thread may set one while others run calls; a value < 0 hands the switch
 *     back to its environment variable (read once per process) or its default.
 */
#ifndef POINTSAM_HIP_H
#define POINTSAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* psam_stream_t; /* == hipStream_t */

#define PSAM_OK 0
#define PSAM_EINVAL (-1)
#define PSAM_EALIGN (-2)
#define PSAM_EWORKSPACE (-3)

#define PSAM_ACT_NONE 0
#define PSAM_ACT_GELU 1 /* exact erf GELU (torch.nn.GELU default) */
#define PSAM_ACT_RELU 2
#define PSAM_ACT_SWIGLU 3 /* GEMM only: W packs alternating 32-row blocks of fc1_g / fc1_x; C gets N/2 columns silu(g)*x */

int32_t psam_version(void);
const char* psam_last_error_string(void);

/* ---------------------------------------------------------------- point tokenizer */

/* Farthest point sampling + center gather.
 * Replaces torkit3d.ops.sample_farthest_points(points, num_samples) and torkit3d batch_index_select:
 * pc_sam/model/common.py:91-92 (also :22-23, :199-200).  Start index 0, fp32 squared distances without FMA,
 * arg-max with lowest index on ties (bit-exact vs oracle/tokenizer_oracle.c).
 *   xyz [B,N,3] -> fps_idx [B,G] int64, centers [B,G,3];  ws: psam_fps_workspace_bytes() bytes, 16B aligned. */
size_t psam_fps_workspace_bytes(int32_t B, int32_t N, int32_t G);
int32_t psam_fps(const float* xyz, int32_t B, int32_t N, int32_t G, int64_t* fps_idx, float* centers, void* ws, size_t ws_bytes,
                 psam_stream_t stream);
void psam_fps_set_cooperative(int32_t on); /* test hook: 0 = never use the multi-workgroup kernel for N > 32768, 2 = use it without the one-XCD placement */
void psam_fps_set_pruning(int32_t mode);   /* A/B and test hook: 0 = the multi-workgroup kernel scans every point in every iteration, 1 = it buckets the cloud by
                                            * grid cell and skips, exactly, the waves whose bounding box the new centre cannot reach; -1 = default
                                            * (environment PSAM_FPS_PRUNE, else 1) */
/* test queries (thread-local, host-side bookkeeping).  psam_fps_last_instance: the kernel instance the calling thread's last psam_fps launched,
 * kind * 100 + PPT4 (kind 0 = the single-workgroup kernel, PPT4 = 1 .. 8 groups of 4096 points held in registers / LDS, 0 = streamed; 1 = the
 * multi-workgroup kernel, 2 = the pruned multi-workgroup kernel, PPT4 in {1, 2, 4}); psam_fps_last_grid_x: the width of that launch's grid
 * (workgroups per cloud x 8 with the one-XCD placement, x 1 without; 0 for kind 0).  Both -1 before the first launch and after a refused call. */
int32_t psam_fps_last_instance(void);
int32_t psam_fps_last_grid_x(void);

/* K nearest points of each center, ascending by (squared distance, index); the [G,N] distance matrix is never
 * materialised.  Replaces knn_points(centers, xyz, K) = torch.cdist + torch.topk: pc_sam/model/common.py:27-56,97.
 *   centers [B,G,3], xyz [B,N,3] -> knn_idx [B,G,K] int64.  K <= 1024. */
int32_t psam_knn(const float* centers, const float* xyz, int32_t B, int32_t G, int32_t N, int32_t K, int64_t* knn_idx, psam_stream_t stream);
/* tuning / test hook: 1 = the band kernel (one or two distance evaluations per pair; default), 0 = the four-pass kernel, -1 = default (environment PSAM_KNN_BAND) */
void psam_knn_force_band(int32_t mode);
/* test query (thread-local): the kernel the calling thread's last psam_knn launched, 0 = four-pass, 1 = band; -1 before the first launch and after a refused call */
int32_t psam_knn_last_instance(void);

/* 3 nearest centers of every point + normalised 1/max(d^2, eps) weights.
 * Replaces compute_interp_weights(query, key): pc_sam/model/common.py:238-255 (called from mask_decoder.py:151-156).
 *   xyz [B,N,3], centers [B,G,3] -> idx3 [B,N,3] int64, w3 [B,N,3]. */
int32_t psam_three_nn(const float* xyz, const float* centers, int32_t B, int32_t N, int32_t G, float eps, int64_t* idx3, float* w3,
                      psam_stream_t stream);

/* Neighbourhood gather out[bf,g,k,:] = [xyz[idx]-center, feats[bf,idx,:]]  (bf = b*rep + m).
 * Replaces the gather/centre/concat of KNNGrouper.forward: pc_sam/model/common.py:99-120, and of
 * group_with_centers_and_knn: pc_sam/model/common.py:126-187 (rep > 1: several feature sets per cloud).
 *   feats [B*rep,N,C] -> out [B*rep,G,K,3+C]. */
int32_t psam_group_gather(const float* xyz, const float* feats, const float* centers, const int64_t* knn_idx, int32_t B, int32_t rep,
                          int32_t N, int32_t G, int32_t K, int32_t C, float* out, psam_stream_t stream);

/* Same gather fused with the first mini-PointNet layer: GELU(LayerNorm_128(Linear(3+C -> 128))).
 * Replaces PatchEncoder.conv1[0:3] on the grouped features: pc_sam/model/common.py:486-489,499. C in {1,3}.
 *   out [B*rep*G*K, 128]. */
int32_t psam_patch_l1(const float* xyz, const float* feats, const float* centers, const int64_t* knn_idx, const float* W, const float* bias,
                      const float* lnw, const float* lnb, float eps, int32_t B, int32_t rep, int32_t N, int32_t G, int32_t K, int32_t C,
                      float* out, psam_stream_t stream);
/* Both with the grouper's `radius` option (KNNGrouper.radius, common.py:107-108; MaskEncoder.radius, common.py:161-164;
 * configs/model/enc_with_radius.yaml): relative coordinates divided by radius; radius <= 0 = none. */
int32_t psam_group_gather_r(const float* xyz, const float* feats, const float* centers, const int64_t* knn_idx, int32_t B, int32_t rep,
                            int32_t N, int32_t G, int32_t K, int32_t C, float radius, float* out, psam_stream_t stream);
/* the same with a row stride ldo >= 3 + C; the tail of every row is written as zeros (K of the following Linear % 4 == 0) */
int32_t psam_group_gather_ld(const float* xyz, const float* feats, const float* centers, const int64_t* knn_idx, int32_t B, int32_t rep, int32_t N,
                             int32_t G, int32_t K, int32_t C, float radius, float* out, int64_t ldo, psam_stream_t stream);
int32_t psam_patch_l1_r(const float* xyz, const float* feats, const float* centers, const int64_t* knn_idx, const float* W, const float* bias,
                        const float* lnw, const float* lnb, float eps, int32_t B, int32_t rep, int32_t N, int32_t G, int32_t K, int32_t C,
                        float radius, float* out, psam_stream_t stream);
/* The same with the remaining grouper options and a packed output:
 *   center_idx [B,G] (the groups' FPS indices) != NULL: `centralize_features` (KNNGrouper / group_with_centers_and_knn,
 *   common.py:116-118, 183-186): input = [rel xyz, features, features - centre features], W [128, 3 + 2C];
 *   scale_out [rows] != NULL: out receives the g8-packed rows (A operand of psam_gemm_f16x3p for conv1.3) and scale_out their scales. */
int32_t psam_patch_l1_ex(const float* xyz, const float* feats, const float* centers, const int64_t* knn_idx, const int64_t* center_idx,
                         const float* W, const float* bias, const float* lnw, const float* lnb, float eps, int32_t B, int32_t rep, int32_t N,
                         int32_t G, int32_t K, int32_t C, float radius, float* out, float* scale_out, psam_stream_t stream);
/* The kernel instance the calling thread's last psam_patch_l1* launched: 10 x its input width (4 / 6: C = 1 / 3; 5 / 9: the same centralised) + 1 when it
 * wrote the packed form; -1 after a refused call. */
int32_t psam_patch_l1_last_instance(void);

/* Click simulation of the evaluation protocol.  psam_error_regions: fn = gt & !(logit > 0), fp = !gt & (logit > 0)
 * (logits == NULL: fn = gt, fp = 0) -- sample_fixed_points, pc_sam/model/common.py:388-405.  psam_border_farthest: per
 * region the member point farthest from the region's complement (squared distance; -1/-1 when either is empty) --
 * sample_furthest_points_from_border + torkit3d chamfer_distance, pc_sam/model/common.py:443-474.
 *   gt/fn/fp/region [Z,N] uint8, xyz [B,N,3], Z = B*rep. */
int32_t psam_error_regions(const uint8_t* gt, const float* logits, uint8_t* fn, uint8_t* fp, int64_t total, psam_stream_t stream);
size_t psam_border_farthest_workspace_bytes(int32_t Z, int32_t N);
int32_t psam_border_farthest(const float* xyz, const uint8_t* region, int32_t B, int32_t rep, int32_t N, int64_t* out_idx, float* out_dist,
                             void* ws, size_t ws_bytes, psam_stream_t stream);

/* Max over the K members of each group: x [groups*K, C] -> y [groups, C].
 * Replaces torch.max(x, dim=-2): pc_sam/model/common.py:502,505. */
int32_t psam_group_max(const float* x, int64_t ldx, float* y, int64_t ldy, int64_t groups, int32_t K, int32_t C, psam_stream_t stream);

/* ---------------------------------------------------------------- dense layers (fp32-exact MFMA) */

/* C[z] = act(alpha * A[z] @ W[z]^T + bias + rowbias[row/rowgroup]) + residual[z];  A [M,K], W [N,K] (nn.Linear layout).
 * Replaces every nn.Linear / F.linear / matmul on the path (cuBLAS in the reference): common.py:486-497,
 * pc_encoder.py:99-116, timm Eva blocks, transformer.py:199-202,248-249, mask_decoder.py:53-59,176,201-203.
 * Batch index z = z1*batch2 + z2 with element strides s?1 / s?2.  K, lda, ldw and batch strides multiples of 4. */
int32_t psam_gemm_f32(const float* A, int64_t lda, int64_t sA1, int64_t sA2, const float* W, int64_t ldw, int64_t sW1, int64_t sW2, float* C,
                      int64_t ldc, int64_t sC1, int64_t sC2, const float* bias, const float* residual, int64_t ldr, int64_t sR1, int64_t sR2,
                      const float* rowbias, int64_t ldrb, int32_t rowgroup, int32_t M, int32_t N, int32_t K, int32_t batch1, int32_t batch2,
                      float alpha, int32_t act, psam_stream_t stream);
/* Same contract, fp32-accurate on the bf16 matrix pipe: each fp32 operand is split exactly into 3 bf16 terms while its
 * K slab is staged, 6 of the 9 partial products are accumulated in fp32 (dropped terms <= 2^-24 relative).  128x128
 * tiles: use for M, N >= 128. */
int32_t psam_gemm_bf16x6(const float* A, int64_t lda, int64_t sA1, int64_t sA2, const float* W, int64_t ldw, int64_t sW1, int64_t sW2, float* C,
                         int64_t ldc, int64_t sC1, int64_t sC2, const float* bias, const float* residual, int64_t ldr, int64_t sR1, int64_t sR2,
                         const float* rowbias, int64_t ldrb, int32_t rowgroup, int32_t M, int32_t N, int32_t K, int32_t batch1, int32_t batch2,
                         float alpha, int32_t act, psam_stream_t stream);
/* fp32-grade GEMM on the fp16 matrix pipe ("f16x3"; 2-D form of the psam_gemm_f32 contract, same reference call sites).
 * Each operand row is scaled by a power of two (row maximum into [2^14, 2^15): psam_row_scale_f16; a static weight's scales are
 * computed once at load) and split into hi + lo fp16; hi*hi + hi*lo + lo*hi are accumulated in fp32 (dropped lo*lo and split
 * residual <= 3*2^-22 relative per product) and the epilogue multiplies by 1/(scaleA[row] scaleW[col]) exactly. */
int32_t psam_row_scale_f16(const float* X, int64_t ldx, int32_t rows, int32_t cols, float* scale, psam_stream_t stream);
/* Production form of the large GEMMs ("f16x3p", csrc/gemm_f16x3p.hip): BOTH operands pre-packed in the "g8" form -- per group of 8
 * consecutive k: [hi k0..k7 (8 x fp16) | lo k0..k7] in the same 32-bit-per-element container -- so that one 16-byte chunk is one
 * matrix-instruction operand and a K slab moves global -> LDS by LDS-DMA with no staging registers or arithmetic.  K % 32 == 0 (pack
 * pads with zeros up to the next multiple of 32: ldp >= that), K >= 128, packed rows 32-byte aligned.  Replaces the same reference
 * call sites as psam_gemm_f32 (every nn.Linear of pc_sam/model/ *.py and of the timm Eva blocks). */
int32_t psam_pack_rows_f16x2_g8(const float* X, int64_t ldx, const float* scale, int32_t rows, int32_t K, void* P, int64_t ldp, psam_stream_t stream);
int32_t psam_gemm_f16x3p(const void* A, int64_t lda, const float* scaleA, const void* W, int64_t ldw, const float* scaleW, float* C, int64_t ldc,
                         const float* bias, const float* residual, int64_t ldr, const float* rowbias, int64_t ldrb, int32_t rowgroup, int32_t M,
                         int32_t N, int32_t K, float alpha, int32_t act, psam_stream_t stream);
void psam_gemm_f16x3p_force_config(int32_t cfg); /* tuning hook: tile / ring configuration index, -1 = auto */
/* Test hooks: the configuration index (ping-pong kernel: 50 ..; the full-row tile of the row epilogues: 40) and the split-K factor (1: unsplit) of the
 * calling thread's last psam_gemm_f16x3p(_ex) call; -1 and 0 when that call was refused.  A forced configuration runs as forced or is refused. */
int32_t psam_gemm_f16x3p_last_config(void);
int32_t psam_gemm_f16x3p_last_splitk(void);
/* Epilogue of the packed-operand GEMMs: 1 = register-only epilogue on transposed accumulator tiles (csrc/gemm_epilogue_t.h) wherever the
 * launch's options allow it, 0 = always the LDS-transposition epilogue (csrc/gemm_epilogue.h), -1 = default (environment PSAM_GEMM_TR, else 1).
 * Both give the same bits; the hook exists for A/B measurements and the bitwise test. */
void psam_gemm_f16x3p_force_epilogue(int32_t mode);
/* split-K launches of psam_gemm_f16x3p_ex: 1 = in-kernel fix-up (the last workgroup of a tile adds the partial accumulators in split order and runs the
 * epilogue; no reduction launch), 0 = partial planes + reduction launch, -1 = the default (fix-up wherever psam_gemm_fuse_t.counters is given and the workspace allows;
 * environment PSAM_GEMM_SPLITK_FIXUP=0 switches it off).  Tuning / test hook: both forms give the same bits for power-of-two scales. */
void psam_gemm_f16x3p_force_splitk_fixup(int32_t mode);
#ifdef PSAM_BUILD_EXPERIMENTS
/* Batch-sized launches (>= 2048 rows) of the packed-operand GEMM on the 128x128 register-epilogue configuration: the persistent kernel (csrc/gemm_f16x3c.hip: resident
 * workgroups draw whole tiles from per-XCD queues and keep one continuous stream of K slabs going across tile boundaries; the same bits, measured the same
 * time: profiles/r05/r05_continuous_sweep.txt) -- -1 = default (environment PSAM_GEMM_CONTINUOUS, else off), 0 = never, 1 = wherever it applies. */
void psam_gemm_f16x3p_force_continuous(int32_t mode);
#endif
/* ARRIVAL-COUNTER BLOCK (round 6: the library allocates nothing and keeps no per-stream state).  Kernels with an in-kernel fix-up -- the split-K GEMM
 * (the last workgroup of a tile adds the partial accumulators), the key-split attention (the last arrival combines the partial softmax states), the
 * skinny Linear + LayerNorm of the decoder's token side (the last workgroup normalises the rows) -- count their workgroups in through device memory the
 * CALLER owns: PSAM_COUNTER_BYTES bytes, zero before the first use (one hipMemsetAsync), left zero by every launch that completes.  Launches that
 * share a block must be ordered with respect to each other (one stream, or one graph); streams or graphs that run CONCURRENTLY need a block each.
 * A captured launch carries the block's address like any other buffer: a graph replays on any stream.  After a FAILED launch re-zero the block.
 * NULL where an entry takes `counters`: the entry runs without the in-kernel fix-up (reduction pass, unsplit attention, two launches). */
#define PSAM_COUNTER_BYTES 65536
/* psam_attention_f16x3(_ex) with few workgroups (one cloud, head dim in (64, 128]): up to four workgroups per (query block, head) share the key tiles and
 * the last arrival combines their partial softmax states in split order.  0 = never split, 1 = split wherever it pays (also where the environment
 * says PSAM_ATTN_KEYSPLIT=0), -1 = the default (environment PSAM_ATTN_KEYSPLIT, else 1). */
void psam_attention_f16x3_force_keysplit(int32_t mode);
/* What the calling thread's last psam_attention_f16x3(_ex, _ex2) launched: the channel-layout instance (64: head dim 64; 96: head dims in (64, 96] on the
 * 128-wide layout with 96 active channels; 128: the full 128-channel instance), -1 after a refused call; and the key-split factor actually used
 * (1 = unsplit), 0 after a refused call.  psam_attention_f32_last_instance: the head dim whose instance the last psam_attention_f32 launched, or -1. */
int32_t psam_attention_f16x3_last_instance(void);
int32_t psam_attention_f16x3_last_keysplit(void);
int32_t psam_attention_f32_last_instance(void);
/* psam_twoway_decoder: 1 = the patch-side projections of a layer run on a side stream forked from (and joined back into) the caller's stream -- also
 * inside a graph capture --, 0 = everything in sequence on the caller's stream, -1 = the default (environment PSAM_TWOWAY_FORK, else 0: the fork measured
 * slower, csrc/blocks.hip TwSide).  Same kernels, same bits. */
#ifdef PSAM_BUILD_EXPERIMENTS      /* measured-and-rejected paths: built only with PSAM_BUILD_EXPERIMENTS=1 (point_sam_amd/build.py) */
void psam_twoway_decoder_force_fork(int32_t mode);
#endif
/* 1 when psam_gemm_f16x3p_ex accepts psam_gemm_fuse_t.row_ln_* for N output columns (Linear -> LayerNorm -> activation in one GEMM; common.py:493-496,
 * mask_decoder.py:53-59): N == 256 always, N == 512 with the register epilogue (packed output scaled by the a-priori bound out_k2, out_k1 == 0). */
int32_t psam_gemm_f16x3p_fused_row_ln(int32_t N);
/* The same GEMM with fused extras (all optional; M % 256 == 0 and N % 128 == 0 required when any is used) -- what lets the EVA02 MLP
 * `fc2(LayerNorm(SiLU(fc1_g x) * fc1_x x))` (timm SwiGLU with scale_mlp) run as two GEMMs and nothing in between:
 *   pack_out : C receives the g8-packed output rows (the next GEMM's A operand), scaled per row by out_scale[row] (written here) =
 *              the power of two that puts the BOUND B = out_k1 / scaleA[row] + out_k2 (B^2 with the SwiGLU gate) of the row's magnitude
 *              into [2^14, 2^15) -- out_k1 = 2^15 sqrt(K) max_n ||W[n]||_2, out_k2 = max |bias| (Cauchy-Schwarz);
 *   stats    : [M, psam_gemm_f16x3p_stat_segs(N), 2] (mean, centred sum of squares) of every 32-column segment of the gated rows over
 *              the columns < stat_cols; psam_ln_stats_finalize merges them (fixed order) into the LayerNorm's mean / rstd per row;
 *   gmax_*   : gmax_out [M / gmax_k, >= N] (row stride gmax_ld) = per-column maximum over every group of gmax_k (32 or 64) consecutive
 *              output rows -- PatchEncoder's max-pool over the group members (common.py:491,497); no_store: C is not written;
 *   row_ln_* : (N == 256) LayerNorm over each output row before the activation -- Linear -> LayerNorm -> GELU of the decoder's upscaling
 *              MLP (mask_decoder.py:53-59) in one epilogue (with pack_out pass out_k1 = 0, out_k2 >= sqrt(255) max|gamma| + max|beta|);
 *   hyper    : (N == 256) masks[z, c, n] = <hyper[z, c, :], out[z * hyper_rows + n, :]>, c < hyper_c <= 4, hyper_rows % 32 == 0 -- the hyper-network product
 *              of mask_decoder.py:171-176 taken from the rows as they are finished (with no_store the [rows, 256] output is not written);
 *   ln_*     : LayerNorm of the A rows folded into the GEMM: C = rstd[row] (A W'^T - mean[row] c[col]) + bias (+ residual), with the
 *              caller's W' = W * gamma (per column), c = W' 1, bias = W beta + b. */
typedef struct {
    float* out_scale; float out_k1, out_k2; int32_t pack_out;
    float* stats; int32_t stat_cols;
    const float* ln_mean; const float* ln_rstd; const float* ln_c;
    float* gmax_out; int64_t gmax_ld; int32_t gmax_k; int32_t no_store;
    const float* row_ln_g; const float* row_ln_b; float row_ln_eps;
    const float* hyper; float* masks; int32_t hyper_c; int32_t hyper_rows;
    int64_t hyper_pstride;
    /* split-K: splitk > 1 workgroups per output tile share the K loop; partial products go to splitk planes of splitk_ws (splitk_plane >=
     * M * N floats apart), added in a fixed order with bias / activation / residual applied afterwards.  No other extras, act != SwiGLU,
     * no rowbias, N % 4 == 0, splitk <= K / 128.  psam_gemm_f16x3p_splitk() suggests the factor for a shape (1: none). */
    float* splitk_ws; int64_t splitk_plane; int32_t splitk;
    /* pack_out with a bound PER ROW: out_scale[row] = f16_row_scale(out_bound[row]) instead of the k1 / k2 form (out_bound[row] >= max |output
     * row|; psam_layernorm_ex2 writes it from the L2 norm of the A row).  Tighter than k1 / scaleA + k2 by sqrt(K) max|a| / ||a||_2. */
    const float* out_bound;
    /* split-K with the in-kernel fix-up: the caller's arrival-counter block (PSAM_COUNTER_BYTES, see above); NULL = partial planes + reduction launch */
    int32_t* counters;
} psam_gemm_fuse_t;
int32_t psam_gemm_f16x3p_splitk(int32_t M, int32_t N, int32_t K, int32_t act);
/* hyper without row_ln_*: any N % 128 == 0, M % 256 == 0; every 64-column wave tile contributes the partial products of its columns:
 * masks then holds psam_gemm_f16x3p_hyper_planes(N, 0) = N / 64 planes of [Z, C, hyper_rows], hyper_pstride elements apart, and
 * psam_sum_planes adds them in a fixed order.  With row_ln_* (full-row tile, N == 256) there is one plane. */
int32_t psam_gemm_f16x3p_hyper_planes(int32_t N, int32_t with_row_ln);
int32_t psam_sum_planes(const float* parts, int32_t P, int64_t pstride, int64_t count, float* out, psam_stream_t stream);
int32_t psam_gemm_f16x3p_stat_segs(int32_t N);
int32_t psam_gemm_f16x3p_ex(const void* A, int64_t lda, const float* scaleA, const void* W, int64_t ldw, const float* scaleW, float* C, int64_t ldc,
                            const float* bias, const float* residual, int64_t ldr, const float* rowbias, int64_t ldrb, int32_t rowgroup, int32_t M,
                            int32_t N, int32_t K, float alpha, int32_t act, const psam_gemm_fuse_t* fuse, psam_stream_t stream);
int32_t psam_ln_stats_finalize(const float* stats, int32_t rows, int32_t segs, int32_t cols, float eps, float* mean, float* rstd, psam_stream_t stream);
/* Linear (128 -> 512) -> LayerNorm -> GELU -> g8-packed rows in one persistent kernel (csrc/patch_rowln.hip): PatchEncoder's per-row half of conv2.0, conv2.1
 * and its GELU (common.py:493-496) without the [rows, 512] fp32 activation.  x [rows, ldx] / w [512, ldw]: g8-packed operands of 128 columns with their row
 * scales; rowbias [rows / rowgroup, ldrb]: a bias row per group of rowgroup consecutive rows (the pooled half of conv2.0 with its bias); out [rows, ldo]
 * receives the packed rows scaled by out_scale[row] = the power of two that puts `bound` (>= max|gamma| sqrt(512) + max|beta|, which bounds every LayerNorm
 * output and its GELU) into [2^14, 2^15).  h1 == 512, rows % 64 == 0, rows < 2^31, rowgroup % 32 == 0; packed rows 32-byte, the fp32 vectors 16-byte aligned.
 * The caller guarantees rows % rowgroup == 0 (rows = groups x rowgroup): the entry does not check it, and rowbias is read as rows / rowgroup whole rows. */
int32_t psam_linear128_ln_gelu_pack(const void* x, int64_t ldx, const float* x_scale, const void* w, int64_t ldw, const float* w_scale, const float* rowbias,
                                    int64_t ldrb, int32_t rowgroup, const float* gamma, const float* beta, float eps, float bound, int64_t rows, int32_t h1,
                                    void* out, int64_t ldo, float* out_scale, psam_stream_t stream);
/* Row scales and g8 packing of fp32 rows in ONE pass (an activation no LayerNorm produced, e.g. the attention output). */
int32_t psam_scale_pack_rows_g8(const float* X, int64_t ldx, int32_t rows, int32_t K, void* P, int64_t ldp, float* scale, psam_stream_t stream);
int32_t psam_linear(const float* x, int64_t ldx, const float* W, int64_t ldw, const float* bias, const float* residual, int64_t ldr, float* y,
                    int64_t ldy, int32_t M, int32_t N, int32_t K, int32_t act, psam_stream_t stream);
void psam_gemm_bf16x6_force_config(int32_t cfg); /* tuning hook: 0=128x128, 1=128x64 tiles, -1=auto */
void psam_gemm_force_config(int32_t cfg); /* tuning hook: 0=128x128, 1=128x64, 2=64x64 tiles, -1=auto */

/* y = act(LayerNorm(x (+ res))).  Replaces nn.LayerNorm / apex FusedLayerNorm (pc_sam/utils/torch_utils.py:28-38)
 * at common.py:488,494, timm blocks, transformer.py:59,128-138, mask_decoder.py:55. */
int32_t psam_layernorm(const float* x, int64_t ldx, const float* res, int64_t ldr, const float* w, const float* b, float* y, int64_t ldy,
                       int64_t rows, int32_t cols, float eps, int32_t act, psam_stream_t stream);
/* Same, plus row_scale[rows] (optional): the power-of-two f16x3 scale of every OUTPUT row (psam_row_scale_f16 fused in). */
/* psam_layernorm_ex: pack != 0 writes y as the g8-packed form of the row-scaled output, zero-padded to cols rounded up to 32 when ldy has
 * room (needs row_scale; 256 <= cols <= 4096; 32-byte aligned output rows): the A operand of psam_gemm_f16x3p. */
int32_t psam_layernorm_ex(const float* x, int64_t ldx, const float* res, int64_t ldr, const float* w, const float* b, float* y, int64_t ldy,
                          int64_t rows, int32_t cols, float eps, int32_t act, float* row_scale, int32_t pack, psam_stream_t stream);
/* psam_layernorm_ex2: row_bound (optional, with pack, [rows]) receives c2 t^2 + c1 t + c0, t = 1.0001 x the L2 norm of the output row: the
 * a-priori bound of the rows of the GEMM that consumes this output (|W_n . h + b_n| <= ||W_n|| t + |b_n|; psam_gemm_fuse_t.out_bound). */
int32_t psam_layernorm_ex2(const float* x, int64_t ldx, const float* res, int64_t ldr, const float* w, const float* b, float* y, int64_t ldy,
                           int64_t rows, int32_t cols, float eps, int32_t act, float* row_scale, int32_t pack, float* row_bound, float c2,
                           float c1, float c0, psam_stream_t stream);
int32_t psam_layernorm_rs(const float* x, int64_t ldx, const float* res, int64_t ldr, const float* w, const float* b, float* y, int64_t ldy,
                          int64_t rows, int32_t cols, float eps, int32_t act, float* row_scale, psam_stream_t stream);
/* The kernel instance the calling thread's last psam_layernorm* launched: NREG of the scalar kernel (2, 4, 8, 16, 44 registers per lane; 0 = the
 * streaming kernel for more than 2816 columns), 1000 + NV4 of the float4 kernel (1, 2, 4, 8, 16), + 100 when it wrote the packed form; -1 after a
 * refused call. */
int32_t psam_layernorm_last_instance(void);

/* out = LayerNorm_H(SiLU(gx[:,0:H]) * gx[:,xoff:xoff+H]), zero-padded to ldo columns.
 * Replaces timm SwiGLU (act, mul, norm) inside eva02 blocks (called through pc_encoder.py:138-139). */
int32_t psam_swiglu_ln(const float* gx, int64_t ldg, int32_t xoff, const float* w, const float* b, float* out, int64_t ldo, int64_t rows,
                       int32_t H, float eps, psam_stream_t stream);
/* The kernel instance the calling thread's last psam_swiglu_ln launched: 8, 32 or 44 registers per lane, 0 = streaming (H > 2816); -1 after a
 * refused call. */
int32_t psam_swiglu_ln_last_instance(void);

/* softmax(q k^T * scale) v per (batch, head), flash-style on the matrix cores; q/k/v/o are [B,L,H*hd] views.
 * Replaces F.scaled_dot_product_attention inside timm EvaAttention (pc_encoder.py:138-139).
 * hd in {16,24,32,48,64,88,96,128}. */
int32_t psam_attention_f32(const float* q, int64_t ldq, int64_t sq, const float* k, int64_t ldk, int64_t sk, const float* v, int64_t ldv,
                           int64_t sv, float* o, int64_t ldo, int64_t so, int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t hd,
                           float scale, psam_stream_t stream);
/* Same contract on the fp16 matrix pipe with fp32-grade products (power-of-two scaling + hi/lo fp16 split of Q, K, V and of the
 * probabilities, 3 MFMA products each; csrc/attention.hip).  head_dim 64, or a multiple of 8 in (64, 128] (computed zero-padded to 128). */
int32_t psam_attention_f16x3(const float* q, int64_t ldq, int64_t sq, const float* k, int64_t ldk, int64_t sk, const float* v, int64_t ldv,
                           int64_t sv, float* o, int64_t ldo, int64_t so, int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t hd,
                           float scale, psam_stream_t stream);
/* The same with a PACKED output for the output projection (psam_gemm_f16x3p): a_scale [B*Lk] = the row scales of the qkv GEMM's A
 * operand (LayerNorm output), k1 = 2^15 sqrt(D) max_n ||W_v[n]||_2, k2 = max |b_v|: every |V| of a cloud -- hence every attention
 * output, a convex combination of V rows -- is below B = k1 / min_rows(a_scale) + k2; o receives the g8-packed rows scaled by the
 * power of two that puts B into [2^14, 2^15), o_scale [B*Lq] that scale.  a_scale == NULL: plain fp32 output. */
int32_t psam_attention_f16x3_ex(const float* q, int64_t ldq, int64_t sq, const float* k, int64_t ldk, int64_t sk, const float* v, int64_t ldv,
                                int64_t sv, float* o, int64_t ldo, int64_t so, int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t hd, float scale,
                                const float* a_scale, float k1, float k2, float* o_scale, psam_stream_t stream);
/* the same with the KEY SPLIT: few workgroups (one cloud, head dim in (64, 128]: 16 heads x 4 query blocks = 64 on 256 CUs) -- up to max_keysplit <= 4
 * workgroups per (query block, head) share the key tiles and the last arrival combines their partial softmax states in split order, inside the kernel.
 * Needs ks_ws (psam_attention_f16x3_keysplit_ws_bytes(...) bytes of scratch for the partial states) and the caller's arrival-counter block `counters`
 * (PSAM_COUNTER_BYTES, see above); with either NULL, or max_keysplit = 1, the launch is unsplit (what psam_attention_f16x3_ex does; a caller that keeps
 * the chip busy from several streams -- throughput -- is better off without the split's extra work). */
size_t psam_attention_f16x3_keysplit_ws_bytes(int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t hd, int32_t max_keysplit);
int32_t psam_attention_f16x3_ex2(const float* q, int64_t ldq, int64_t sq, const float* k, int64_t ldk, int64_t sk, const float* v, int64_t ldv,
                                int64_t sv, float* o, int64_t ldo, int64_t so, int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t hd, float scale,
                                const float* a_scale, float k1, float k2, float* o_scale, int32_t max_keysplit, void* ks_ws, size_t ks_ws_bytes,
                                int32_t* counters, psam_stream_t stream);

/* Self-attention on PRE-PACKED operands (head dim 64): qkv [B*L, ld] holds every row's q | k | v (column blocks of D = H*64 containers) in
 * the g8-packed hi|lo fp16 form of psam_gemm_f16x3p, all rows with ONE power-of-two scale (sc[b*L] is read) -- what the qkv GEMM writes with
 * psam_gemm_fuse_t {pack_out = 1, out_k1 = 0, out_k2 = an a-priori bound of |q|, |k|, |v|}.  Replaces the SDPA call of timm's EvaAttention
 * (pc_sam/model/pc_encoder.py:138-139) together with the conversions the fp32-input kernels above do per tile: K / V tiles move global -> LDS
 * by LDS-DMA, V is transposed on read (ds_read_b64_tr_b16), nothing is scaled or split in the kernel except the probabilities.
 * o [B*L, ldo]: g8-packed output for the projection GEMM, o_scale [B*L] = f16_row_scale(v_bound) for every row (v_bound >= max |v|). */
int32_t psam_attention_packed(const void* qkv, int64_t ld, const float* sc, float* o, int64_t ldo, float* o_scale, int32_t B, int32_t H, int32_t L,
                              int32_t hd, float scale, float v_bound, psam_stream_t stream);
/* Tuning hook: -1 default (environment PSAM_ATTN_VARIANT, else 1), 0 = 256-row workgroups of eight waves on a three-tile ring -- 128-row workgroups of four
 * waves where the 256-row grid would leave CUs idle --, 1 = two 128-row workgroups per CU on a two-tile ring where that grid is at most four per CU (else
 * as 0), 2 = four waves with two query blocks each (experiments builds only).  A variant the build cannot run -- 2 in a default build, anything above 2,
 * by this hook or by the environment -- is REFUSED by psam_attention_packed (PSAM_EINVAL): a forced variant runs as forced or not at all.  The variant
 * does not decide everything: L <= 128 always runs the eight-wave kernel, and a forced workgroup shape (below) wins over it. */
void psam_attention_packed_force_variant(int32_t v);
/* Test / tuning hook, the process-level twin of the environment's PSAM_ATTN_PACKED_NW: -1 default (the environment, else 0), 0 = by shape and CU count,
 * 4 / 8 = the four- / eight-wave kernel on the three-tile ring whatever the shape and variant; any other value makes psam_attention_packed refuse. */
void psam_attention_packed_force_nw(int32_t nw);
/* The kernel instance the calling thread's last psam_attention_packed launched, as waves * 100 + ring tiles * 10 + query blocks per wave
 * (831, 431, 421; 432 in experiments builds); -1 after a refused call. */
int32_t psam_attention_packed_last_instance(void);

/* y [M, N] = act(x [M, K] W [N, K]^T + bias) + residual for M <= 64 rows (K % 16 == 0, rows 16-byte aligned; act: none / GELU / ReLU),
 * exact fp32 products.  The decoder's token-side nn.Linear calls (7 output tokens per prompt): transformer.py:109-236.  An inf or a NaN in a row of x
 * reaches that row of y only (as NaN where K has a ragged last round of 128), and the ReLU of this entry and of the two below keeps a NaN, as torch.relu does. */
int32_t psam_linear_skinny(const float* x, int64_t ldx, const float* W, int64_t ldw, const float* bias, const float* residual, int64_t ldr,
                           float* y, int64_t ldy, int32_t M, int32_t N, int32_t K, int32_t act, psam_stream_t stream);

/* Up to PSAM_SKINNY_MAX_JOBS skinny Linears over the same M <= 64 input rows in one launch: y_i = act_i((x_i + xadd_i) W_i^T + bias_i), xadd optional (the
 * decoder's q = k = queries + query_pe, v = queries: transformer.py:153-170,214-236).  All jobs share ldx (x rows), ldxadd, ldw, M and K. */
typedef struct {
    const float* x; const float* xadd; const float* W; const float* bias; float* y;
    int64_t ldy;
    int32_t N, act;
} psam_skinny_job_t;
#define PSAM_SKINNY_MAX_JOBS 6
typedef struct {
    psam_skinny_job_t job[PSAM_SKINNY_MAX_JOBS];
    int32_t n;
} psam_skinny_jobs_t;
int32_t psam_linear_skinny_multi(const psam_skinny_jobs_t* jobs, int64_t ldx, int64_t ldxadd, int64_t ldw, int32_t M, int32_t K, psam_stream_t stream);
/* The same for ANY number of rows (a few hundred to a few thousand: the decoder's patch rows), exact fp32 products, 32 x 32 tiles: y_i [M, N_i] =
 * act_i((x_i + xadd_i) W_i^T + bias_i).  xadd_i (optional) holds sets of rows_per_set rows; row r adds row (r / (rep * rows_per_set)) * rows_per_set +
 * r % rows_per_set (key_pe of the cloud, shared by its rep prompt sets: transformer.py:160-175). */
int32_t psam_linear_rows_multi(const psam_skinny_jobs_t* jobs, int64_t ldx, int64_t ldxadd, int32_t rows_per_set, int32_t rep, int64_t ldw, int64_t M, int32_t K,
                               psam_stream_t stream);
/* Skinny Linear + residual + LayerNorm in one launch: y [M, 256] = LayerNorm(x W^T + bias + residual) * ln_w + ln_b, M <= 64 rows, N == 256 -- the
 * `queries = norm(queries + out_proj(attn))` / `norm3(queries + mlp(queries))` steps of the decoder's token side (transformer.py:153-176).  The last
 * workgroup to finish its columns normalises the rows (`counters`: the caller's arrival-counter block, PSAM_COUNTER_BYTES, see above; required).  K is
 * split over up to 8 workgroup rows (lin2 of the token MLP: K = 2048).  tmp: psam_linear_skinny_ln_tmp_floats(M, K) floats. */
size_t psam_linear_skinny_ln_tmp_floats(int32_t M, int32_t K);
int32_t psam_linear_skinny_ln(const float* x, int64_t ldx, const float* W, int64_t ldw, const float* bias, const float* residual, int64_t ldr,
                              const float* ln_w, const float* ln_b, float eps, float* tmp, float* y, int64_t ldy, int32_t M, int32_t N, int32_t K,
                              int32_t* counters, psam_stream_t stream);
/* The same for ANY number of rows and a short K (K % 16 == 0, K <= 512): y [M, 256] = LayerNorm(x W^T + bias + residual) * ln_w + ln_b, a workgroup per
 * 16 whole rows, exact fp32 products -- `keys = norm4(keys + out_proj(attn))` of the decoder's patch side (transformer.py:170-175; K = 128). */
int32_t psam_linear_ln256(const float* x, int64_t ldx, const float* W, int64_t ldw, const float* bias, const float* residual, int64_t ldr, const float* ln_w,
                          const float* ln_b, float eps, float* y, int64_t ldy, int64_t M, int32_t N, int32_t K, psam_stream_t stream);
/* psam_scale_pack_rows_g8 of X + add[(row / (rep * rows_per_set)) * rows_per_set + row % rows_per_set]: the broadcast positional add of the decoder's
 * keys (k = keys + key_pe, transformer.py:160-170) folded into the pass that scales and packs the rows for the k / q projection GEMMs. */
int32_t psam_scale_pack_rows_g8_add(const float* X, int64_t ldx, const float* add, int64_t ldadd, int32_t rows_per_set, int32_t rep, int32_t rows, int32_t K,
                                    void* P, int64_t ldp, float* scale, psam_stream_t stream);

/* Both packed forms of the decoder's patch rows in one pass (K <= 256): P_sum / scale_sum = psam_scale_pack_rows_g8_add's output (keys + key_pe, the
 * operand of the k / q projections), P_x / scale_x = psam_scale_pack_rows_g8 of X alone (the operand of the v projection); transformer.py:160-170. */
int32_t psam_scale_pack_rows_g8_add_dual(const float* X, int64_t ldx, const float* add, int64_t ldadd, int32_t rows_per_set, int32_t rep, int32_t rows, int32_t K,
                                         void* P_sum, float* scale_sum, void* P_x, float* scale_x, int64_t ldp, psam_stream_t stream);

/* ONE EVA02 (SwiGLU) transformer block of the patch encoder in one call (csrc/blocks.hip) -- timm's block as the reference runs it
 * (pc_sam/model/pc_encoder.py:138-139, no rope): x += proj(SDPA(LN1 x)); x += fc2(LN(SiLU(fc1_g h) * fc1_x h)), h = LN2 x.  "f16x3" arithmetic with
 * every hand-over fused as the Python host does it: eight launches, nothing in between.  Head dim 64 (heads == dim / 64), 256 <= dim <= 4096,
 * dim % 128 == 0 (packed LayerNorm; fused epilogues on whole 128-column tiles), hidden rounded up to 32 a multiple of 64 and >= 128, B * L % 256 == 0;
 * _prepare refuses any other dim / heads / hidden and psam_eva_block any other B * L with PSAM_EINVAL, before anything is launched.
 * psam_eva_block_prepare (load time; copies the weights to the host once, uses a temporary device buffer, synchronises) packs a block's weights
 * -- given in the reference's / timm's state-dict layout, [out, in] fp32 device pointers -- into `prepared` (psam_eva_block_prepared_bytes) and
 * fills the host-side `plan`; the LayerNorm parameters and the projection bias are read through the plan at run time and must stay alive. */
typedef struct {
    const float *norm1_w, *norm1_b, *q_w, *q_b, *k_w, *v_w, *v_b, *proj_w, *proj_b, *norm2_w, *norm2_b;      /* attn.k_proj has no bias */
    const float *fc1_g_w, *fc1_g_b, *fc1_x_w, *fc1_x_b, *mlp_norm_w, *mlp_norm_b, *fc2_w, *fc2_b;
    int32_t dim, heads, hidden;      /* hidden: SwiGLU width (2730 for eva02_large) */
    float eps;                       /* LayerNorm eps of the transformer (1e-6) */
} psam_eva_block_weights_t;
typedef struct {
    int32_t dim, heads, hidden, hidden_pad;
    float eps, qkv_bound, v_bound, u_c2, u_c1, u_c0;      /* a-priori bounds of the packed hand-overs */
    const float *norm1_w, *norm1_b, *norm2_w, *norm2_b, *proj_b;
    int64_t o_wqkv, o_sqkv, o_bqkv, o_wproj, o_sproj, o_w1, o_s1, o_b1, o_w2g, o_s2g, o_lnc, o_lnd;      /* byte offsets into `prepared` */
} psam_eva_block_plan_t;
size_t psam_eva_block_prepared_bytes(int32_t dim, int32_t hidden);
int32_t psam_eva_block_prepare(const psam_eva_block_weights_t* weights, psam_eva_block_plan_t* plan, void* prepared, size_t prepared_bytes, psam_stream_t stream);
size_t psam_eva_block_ws_bytes(int64_t M, int32_t dim, int32_t hidden);
/* x [B*L, dim] fp32, updated in place; ws: psam_eva_block_ws_bytes(B*L, dim, hidden) bytes of scratch */
int32_t psam_eva_block(const psam_eva_block_plan_t* plan, const void* prepared, float* x, int32_t B, int32_t L, void* ws, size_t ws_bytes, psam_stream_t stream);

/* ONE GELU-MLP transformer block with a fused qkv projection (timm eva_giant_patch14_560, configs/model/giant.yaml; called through
 * pc_sam/model/pc_encoder.py:138-139, no rope): x += proj(SDPA(qkv(LN1 x) + [q_bias | 0 | v_bias])); x += fc2(GELU(fc1(LN2 x))).  "f16x3" arithmetic,
 * sequenced as the Python host sequences it (bit-identical): LayerNorm (packed rows) | qkv GEMM | attention on the fp16 pipe for head dims that are
 * multiples of 8 in (64, 128] (88 runs zero-padded to 128) or 64, output packed for the projection | projection + residual | LayerNorm | fc1 + GELU |
 * fc2 + residual.  Few token rows (one cloud: M = 512) leave most of the chip idle on whole-tile launches: every plain GEMM of the block takes the
 * library's split-K factor (psam_gemm_f16x3p_splitk) with the partial planes in the caller's workspace; when fc1 needs no split its epilogue hands
 * GELU(.) to fc2 g8-packed (per-row bound from the LayerNorm's L2 norm) and the scale + pack pass disappears.  dim % 32 == 0, hidden % 32 == 0,
 * hidden >= 128, 256 <= dim <= 4096, B * L >= 256.  `precision`: PSAM_PRECISION_F16X3 (the f32 / bf16x6 arithmetic of the same block is reachable through the
 * per-operator entries only). */
#define PSAM_PRECISION_F16X3 2
typedef struct {
    const float *norm1_w, *norm1_b, *qkv_w, *q_bias, *v_bias, *proj_w, *proj_b, *norm2_w, *norm2_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
    int32_t dim, heads, hidden, precision;
    float eps;
} psam_eva_gelu_block_weights_t;
typedef struct {
    int32_t dim, heads, hidden, precision;
    float eps, vk1, vk2, u_c1, u_c0;      /* attention-output bound from the LayerNorm row scale; fc1 row bound c1 t + c0 from t = ||LN2 x||_2 */
    int32_t attn_keysplit;                /* max key split of the attention (psam_attention_f16x3_ex2): _prepare sets 4; 1 = off (throughput callers) */
    const float *norm1_w, *norm1_b, *norm2_w, *norm2_b, *proj_b, *fc1_b, *fc2_b;
    int64_t o_wqkv, o_sqkv, o_bqkv, o_wproj, o_sproj, o_w1, o_s1, o_w2, o_s2;      /* byte offsets into `prepared` */
} psam_eva_gelu_block_plan_t;
size_t psam_eva_gelu_block_prepared_bytes(int32_t dim, int32_t hidden);
int32_t psam_eva_gelu_block_prepare(const psam_eva_gelu_block_weights_t* weights, psam_eva_gelu_block_plan_t* plan, void* prepared, size_t prepared_bytes,
                                    psam_stream_t stream);
size_t psam_eva_gelu_block_ws_bytes(int64_t M, int32_t dim, int32_t hidden);      /* includes the split-K planes and the key-split partial states */
/* x [B*L, dim] fp32, updated in place.  counters: the caller's arrival-counter block (PSAM_COUNTER_BYTES, see above) for the split-K fix-up and the
 * key-split attention of single-cloud shapes; NULL = reduction passes / unsplit attention (same bits for the GEMMs, round-off for the attention). */
int32_t psam_eva_gelu_block(const psam_eva_gelu_block_plan_t* plan, const void* prepared, float* x, int32_t B, int32_t L, void* ws, size_t ws_bytes,
                            int32_t* counters, psam_stream_t stream);

/* PatchEncoder.forward on kNN groups in one call (csrc/blocks.hip): the mini-PointNet of the patch embedding (features = rgb) and of the mask
 * encoder (features = mask logits) -- pc_sam/model/common.py:477-506 after the gather of :99-120 / :126-187 -- "f16x3", fused as the Python host
 * runs it (five launches for hidden dims (128, 512), where psam_linear128_ln_gelu_pack replaces conv2.0's GEMM and the LayerNorm pass, else six; both max-pools inside GEMM epilogues -- for group sizes above 64 as 64-row parts + psam_group_max over the parts).
 * hidden_dims[0] == 128, group size 32 or a multiple of 64, B * rep * G * K % 256 == 0.
 * Weights: the reference's conv1.{0,1,3} / conv2.{0,1,3} tensors ([out, in] fp32 device pointers); the plan keeps pointers to the small ones. */
typedef struct {
    const float *c10_w, *c10_b, *c11_w, *c11_b, *c13_w, *c13_b, *c20_w, *c20_b, *c21_w, *c21_b, *c23_w, *c23_b;
    int32_t cin, h0, h1, cout;
    float eps;
} psam_patch_encoder_weights_t;
typedef struct {
    int32_t cin, h0, h1, cout;
    float eps, k1, k2, ln21_bound;      /* ln21_bound >= max |gamma| sqrt(h1) + max |beta| of conv2.1: scale of the rows the fused conv2.0 GEMM packs */
    const float *c10_w, *c10_b, *c11_w, *c11_b, *c13_b, *c20_w, *c20_b, *c21_w, *c21_b, *c23_b;
    int64_t o_w13, o_s13, o_w20m, o_s20m, o_w20x, o_s20x, o_w23, o_s23;
} psam_patch_encoder_plan_t;
size_t psam_patch_encoder_prepared_bytes(int32_t h0, int32_t h1, int32_t cout);
int32_t psam_patch_encoder_prepare(const psam_patch_encoder_weights_t* weights, psam_patch_encoder_plan_t* plan, void* prepared, size_t prepared_bytes,
                                   psam_stream_t stream);
size_t psam_patch_encoder_ws_bytes(int64_t rows, int64_t groups, int32_t h0, int32_t h1);
/* feats [B*rep, N, C] (rep mask sets per cloud share xyz / centers / knn_idx); center_idx [B, G] != NULL: centralize_features; out [B*rep*G, cout] */
int32_t psam_patch_encoder(const psam_patch_encoder_plan_t* plan, const void* prepared, const float* xyz, const float* feats, const float* centers,
                           const int64_t* knn_idx, const int64_t* center_idx, int32_t B, int32_t rep, int32_t N, int32_t G, int32_t K, int32_t C,
                           float radius, float* out, void* ws, size_t ws_bytes, psam_stream_t stream);

/* The mask decoder after its transformer in one call (csrc/blocks.hip; pc_sam/model/mask_decoder.py:146-176): 3-NN interpolation G -> N,
 * output_upscaling and the hyper-network products, "f16x3", fused as the Python host runs it (the first Linear on the G patch rows before the
 * interpolation, LayerNorm + GELU inside the interpolation kernel, the products inside the second GEMM's epilogue).  transformer_dim 256. */
typedef struct { const float *u0_w, *u0_b, *u1_w, *u1_b, *u3_w, *u3_b; int32_t dim; float eps; } psam_upscale_weights_t;
typedef struct { int32_t dim; float eps; const float *u0_w, *u0_b, *u1_w, *u1_b, *u3_b; int64_t o_w0, o_s0, o_w3, o_s3; } psam_upscale_plan_t;
size_t psam_upscale_masks_prepared_bytes(int32_t dim);
int32_t psam_upscale_masks_prepare(const psam_upscale_weights_t* weights, psam_upscale_plan_t* plan, void* prepared, size_t prepared_bytes, psam_stream_t stream);
size_t psam_upscale_masks_ws_bytes(int64_t Z, int32_t N, int32_t G, int32_t C, int32_t dim);
/* keys [Z*G, 256], idx3 / w3 [Z / rep, N, 3] (psam_three_nn), hyper [Z, C, 256] (psam_mlp3) -> masks [Z, C, N]; Z * N % 256 == 0, N % 32 == 0, C <= 4 */
int32_t psam_upscale_masks(const psam_upscale_plan_t* plan, const void* prepared, const float* keys, const int64_t* idx3, const float* w3, const float* hyper,
                           int32_t rep, int64_t Z, int32_t N, int32_t G, int32_t C, float* masks, void* ws, size_t ws_bytes, psam_stream_t stream);

/* TwoWayTransformer.forward in one call (csrc/blocks.hip; pc_sam/model/transformer.py:61-100 with TwoWayAttentionBlock :103-176 and Attention
 * :179-236): the decoder's transformer over the patch tokens and the output / prompt tokens, sequenced as the Python host sequences it (per
 * nn.Linear the kernel the host would pick by row count; psam_attention_small; LayerNorm with the residual folded in).  Weights in the
 * reference's state-dict layout ([out, in] fp32 device pointers); _prepare packs every matrix for the rows >= 256 case. */
#define PSAM_TWOWAY_MAX_DEPTH 4
typedef struct { const float *q_w, *q_b, *k_w, *k_b, *v_w, *v_b, *o_w, *o_b; } psam_attn_weights_t;      /* q_proj, k_proj, v_proj, out_proj */
typedef struct {
    psam_attn_weights_t self_attn, t2i, i2t;      /* self_attn, cross_attn_token_to_image, cross_attn_image_to_token */
    const float *n1_w, *n1_b, *n2_w, *n2_b, *n3_w, *n3_b, *n4_w, *n4_b, *m1_w, *m1_b, *m2_w, *m2_b;      /* norm1..4, mlp.lin1, mlp.lin2 */
} psam_twoway_layer_weights_t;
typedef struct {
    int32_t depth, dim, heads, mlp, downsample;      /* 2, 256, 8, 2048, 2 in every reference config */
    float eps;
    const psam_twoway_layer_weights_t* layers;       /* [depth] (host array) */
    psam_attn_weights_t final_attn;                  /* final_attn_token_to_image */
    const float *nf_w, *nf_b;                        /* norm_final_attn */
} psam_twoway_weights_t;
typedef struct {
    psam_twoway_weights_t weights;
    psam_twoway_layer_weights_t layers[PSAM_TWOWAY_MAX_DEPTH];
    int64_t o_packed[14 * PSAM_TWOWAY_MAX_DEPTH + 4], o_scales[14 * PSAM_TWOWAY_MAX_DEPTH + 4];
    int64_t o_cat_packed[PSAM_TWOWAY_MAX_DEPTH], o_cat_scales[PSAM_TWOWAY_MAX_DEPTH], o_cat_bias[PSAM_TWOWAY_MAX_DEPTH];      /* per layer: [t2i.k_proj | i2t.q_proj] as one weight */
} psam_twoway_plan_t;
size_t psam_twoway_decoder_prepared_bytes(int32_t depth, int32_t dim, int32_t mlp, int32_t downsample);
int32_t psam_twoway_decoder_prepare(const psam_twoway_weights_t* weights, psam_twoway_plan_t* plan, void* prepared, size_t prepared_bytes, psam_stream_t stream);
size_t psam_twoway_decoder_ws_bytes(int64_t Z, int32_t T, int32_t G, int32_t dim, int32_t mlp);
/* tokens [Z*T, dim] (= query_pe), keys [Z*G, dim] in / out (src -> the transformer's second output), pos [Z / rep, G, dim] -> queries [Z*T, dim].
 * counters: the caller's arrival-counter block (PSAM_COUNTER_BYTES, see above) for the fused Linear + LayerNorm launches of the regrouped sequence;
 * NULL = the operator-by-operator sequence (the same operators, other launch boundaries: results equal to fp32 round-off).
 * Z % rep == 0, T <= 8192 and G <= 8192 (every attention is psam_attention_small: Lk * 16 <= 128 KiB); anything else is refused with PSAM_EINVAL before
 * the first launch. */
int32_t psam_twoway_decoder(const psam_twoway_plan_t* plan, const void* prepared, const float* tokens, float* keys, const float* pos, int32_t rep, int64_t Z,
                            int32_t T, int32_t G, float* queries, void* ws, size_t ws_bytes, int32_t* counters, psam_stream_t stream);
/* A/B and test hook: 0 = the operator-by-operator launch sequence (what the Python host issues), 1 = the regrouped sequence (fused Linear + LayerNorm
 * launches of the token side, merged projections; csrc/blocks.hip) with packed-operand GEMMs on the patch side, 2 = the regrouped sequence with the
 * exact-fp32 row kernel there, -1 = default (environment PSAM_TWOWAY_FAST, else 2). */
void psam_twoway_decoder_force_fast(int32_t mode);

/* Token side of one TwoWayAttentionBlock in ONE launch (csrc/twoway.hip): self-attention + norm1, token -> image attention + norm2, the MLP
 * + norm3 on the Z * T <= 64 output-token rows, and the k / v projections of the image -> token attention that follows -- what
 * pc_sam/model/transformer.py:144-175 does for `queries`; mode 1: only the token -> image attention + LayerNorm of :91-99
 * (final_attn_token_to_image / norm_final_attn passed in the cq / co / n2 slots).  embedding_dim 256, attention_downsample_rate 2.
 * Weights are the reference's [out, in] matrices; kimg / vimg are the k / v projections of the patch tokens ([Z, G, 128] views, computed by the
 * image-side GEMMs); queries [Z*T, 256] is updated in place, ktok / vtok [Z*T, 128] receive the projections for the image -> token attention.
 * ws: psam_twoway_tokens_ws_floats(mlp) floats of scratch (mode 1: mlp = 0). */
typedef struct {
    int32_t Z, T, G, heads, mlp, mode, skip_pe, reserved;
    float eps;
    float* queries; const float* pe;
    const float* kimg; int64_t ldk, sk; const float* vimg; int64_t ldv, sv;
    const float *sq_w, *sq_b, *sk_w, *sk_b, *sv_w, *sv_b, *so_w, *so_b, *n1_g, *n1_b;
    const float *cq_w, *cq_b, *co_w, *co_b, *n2_g, *n2_b;
    const float *m1_w, *m1_b, *m2_w, *m2_b, *n3_g, *n3_b;
    const float *ik_w, *ik_b, *iv_w, *iv_b;
    float *ktok, *vtok;
    float* ws; int64_t ws_floats;
} psam_twoway_tokens_t;
#ifdef PSAM_BUILD_EXPERIMENTS      /* the one-launch token side measured slower than the launches it replaces: experiments build only */
int64_t psam_twoway_tokens_ws_floats(int32_t mlp);
int32_t psam_twoway_tokens(const psam_twoway_tokens_t* args, psam_stream_t stream);
#endif

/* Voronoi variant (PointCloudSAMNN, configs/model/voronoi.yaml).  psam_nn_group_feats: per-point features relative to the nearest centre --
 * mode 0 = NNGrouper.forward (pc_sam/model/common.py:203-211): [unit offset 3 | distance 1 | feats C]; mode 1 = MaskEncoderNN.forward
 * (prompt_encoder.py:281-287): [logit | offset 3 | distance] for mask set z = b * rep + r; rows ldo floats apart, zero-padded (ldo % 4 == 0
 * for the Linear that follows).  psam_scatter_amax: the max-pool of rows into their cells (torch scatter_reduce "amax": pc_encoder.py:190-193
 * with include_self = 0 -- cells without points end as 0 --, prompt_encoder.py:291-297 with include_self = 1 -- zeros take part);
 * dest(r) = idx[(r / rows_per_set / idx_rep) * rows_per_set + r % rows_per_set] + (r / rows_per_set) * set_stride; exact in any order. */
int32_t psam_nn_group_feats(const float* xyz, const float* centers, const int64_t* nn_idx, const float* feats, const float* logits, int32_t B, int32_t rep,
                            int32_t N, int32_t G, int32_t C, int32_t mode, float* out, int64_t ldo, psam_stream_t stream);
int32_t psam_scatter_amax(const float* x, int64_t ldx, const int64_t* idx, int64_t rows, int32_t C, int64_t rows_per_set, int64_t set_stride,
                          int32_t idx_rep, float* out, int64_t out_rows, int32_t include_self, psam_stream_t stream);

/* Three-layer ReLU MLP on a few rows -- mask_decoder.py:189-211 (MLP), the hyper-networks :171-176 and the IoU head :180 in one launch
 * each.  Weights stacked in the reference's [out, in] layout: w1 [M, dh, din], w2 [M, dh, dh], w3 [M, dout, dh]; biases [M, dh], [M, dh],
 * [M, dout].  MLP m reads the row x + z*ldx + m*sx (z < Z) and writes dout values at out + z*ldo + m*so.  din, dh <= 1024, % 4 == 0. */
int32_t psam_mlp3(const float* x, int64_t ldx, int64_t sx, const float* w1, const float* b1, const float* w2, const float* b2,
                  const float* w3, const float* b3, float* out, int64_t ldo, int64_t so, int32_t Z, int32_t M, int32_t din, int32_t dh,
                  int32_t dout, psam_stream_t stream);

/* Two psam_mlp3 stacks over the same Z rows in ONE launch -- the hyper-networks (mask tokens) and the IoU head (token 0) both read the transformer's
 * token output (mask_decoder.py:167-182).  Fields as the arguments of psam_mlp3; the same bits as two psam_mlp3 calls. */
typedef struct {
    const float *x, *w1, *b1, *w2, *b2, *w3, *b3;
    float* out;
    int64_t ldx, sx, ldo, so;
    int32_t M, din, dh, dout;
} psam_mlp3_args_t;
int32_t psam_mlp3_pair(const psam_mlp3_args_t* a, const psam_mlp3_args_t* b, int32_t Z, psam_stream_t stream);

/* Same contraction for the decoder's token-sized problems (any hd, few queries or few keys).
 * Replaces Attention.forward's matmul-softmax-matmul: pc_sam/model/transformer.py:226-233. */
int32_t psam_attention_small(const float* q, int64_t ldq, int64_t sq, const float* k, int64_t ldk, int64_t sk, const float* v, int64_t ldv,
                             int64_t sv, float* out, int64_t ldo, int64_t so, int64_t Z, int32_t H, int32_t Lq, int32_t Lk, int32_t hd,
                             float scale, psam_stream_t stream);
/* Test / A-B hook: 0 = psam_attention_small always runs one wave per query; 1 (default) = few queries against >= 128 keys run one workgroup per query,
 * the keys split over its four waves. */
void psam_attention_small_force_split(int32_t on);
/* The kernel the calling thread's last psam_attention_small launched: 0 = one wave per query, 1 = one workgroup per query (keys split over its waves),
 * 4 / 8 = the few-keys kernel (Lk <= 16, Lq >= 64) at head dim 16 / 32; -1 after a refused call. */
int32_t psam_attention_small_last_instance(void);

/* ---------------------------------------------------------------- encodings, token assembly, upsampling */

/* y[r,0:128] = GELU(W[128,3] @ centers[r] + bias): first layer of PointCloudEncoder.pos_embed, pc_encoder.py:102-104,130. */
int32_t psam_pos_l1(const float* centers, const float* W, const float* bias, float* y, int64_t rows, psam_stream_t stream);

/* [sin, cos](2*pi * x @ gauss[3,F]) (+ point_embeddings[label]); row r -> out + (r / rows_per_batch)*batch_stride
 * + (r % rows_per_batch)*2F.  *flag |= 1 if a coordinate leaves [-1-1e-6, 1+1e-6] (the reference raises ValueError).
 * Replaces PositionEmbeddingRandom.forward and PointEncoder.forward: pc_sam/model/prompt_encoder.py:27-48,63-77. */
int32_t psam_fourier_pe(const float* coords, const float* gauss, int32_t F, const int64_t* labels, const float* emb0, const float* emb1,
                        float* out, int64_t rows, int32_t rows_per_batch, int64_t batch_stride, int32_t* flag, psam_stream_t stream);

/* out[z,r,:] = a[z/rep,r,:] + (b ? b[z*sb + r*ldb + :] : 0).  Replaces repeat_interleave + adds:
 * pc_sam/model/mask_decoder.py:136-139, pc_sam/model/transformer.py:153-170, prompt_encoder.py:119-122. */
int32_t psam_add_bcast(const float* a, int64_t sa, int32_t rep, const float* b, int64_t sb, int64_t ldb, float* out, int64_t so, int64_t Z,
                       int64_t R, int32_t C, psam_stream_t stream);

/* out[z,n,:] = sum_k w3[b,n,k] * src[z, idx3[b,n,k], :], b = z/rep.  Replaces interpolate_features:
 * pc_sam/model/common.py:258-274 (mask_decoder.py:163). */
int32_t psam_interp3(const float* src, const int64_t* idx3, const float* w3, float* out, int32_t rep, int64_t Z, int32_t N, int32_t G, int32_t C,
                     psam_stream_t stream);
/* scale_out [Z*N] != NULL (C == 256): out receives the g8-packed rows (A operand of psam_gemm_f16x3p) and scale_out their row scales.
 * ln_gamma / ln_beta != NULL (C == 256): LayerNorm(ln_eps) and the activation `act` (none / GELU / ReLU) are applied to every interpolated
 * row -- `interp -> Linear -> LayerNorm -> GELU` of mask_decoder.py:53-59,163 evaluated as `Linear (on the G patch rows) -> interp + LayerNorm
 * + GELU`: the interpolation is an affine combination (weights sum to 1), so it commutes with the Linear layer. */
int32_t psam_interp3_ex(const float* src, const int64_t* idx3, const float* w3, float* out, int32_t rep, int64_t Z, int32_t N, int32_t G, int32_t C,
                        float* scale_out, const float* ln_gamma, const float* ln_beta, float ln_eps, int32_t act, psam_stream_t stream);
/* The kernel the calling thread's last psam_interp3* launched: 256 = the C == 256 kernel (four rows per wave), 0 = the generic one; -1 after a
 * refused call. */
int32_t psam_interp3_last_instance(void);

/* ---------------------------------------------------------------- mask proposals */

/* Automatic mask proposals (point_sam_amd/proposals.py): the post-processing of K candidate masks of one cloud.  A mask is a row of
 * W = ceil(N / 64) 64-bit words: bit (n % 64) of word (n / 64) is point n, bits past N are zero.  All counts are exact integers.
 *
 * psam_mask_pack: rows [K, N] of logits (row stride ld floats) -> rows dst_row .. dst_row + K - 1 of bits [*, W] and of the three areas:
 *   bit = logit > thr (fp32 compare, NaN is false); area_hi / area_lo count logit > fl32(thr + off) / logit > fl32(thr - off). */
int32_t psam_mask_pack(const float* logits, int64_t ld, int32_t K, int32_t N, float thr, float off, int32_t dst_row, uint64_t* bits,
                       int32_t* area, int32_t* area_hi, int32_t* area_lo, psam_stream_t stream);
/* valid[k] = area >= min_points && (double)area < (double)max_area_frac * N && score >= pred_iou_thr (NaN false) && area_lo > 0 &&
 *   (double)area_hi >= (double)stab_thr * (double)area_lo. */
int32_t psam_mask_valid(const int32_t* area, const int32_t* area_hi, const int32_t* area_lo, const float* score, int32_t K, int32_t N,
                        int32_t min_points, float max_area_frac, float pred_iou_thr, float stab_thr, uint8_t* valid, psam_stream_t stream);
/* inter [Ka, Kb] int32 = popcount(a_i & b_j); a [Ka, W], b [Kb, W].  a == b (same pointer, Ka == Kb): the upper triangle is computed and mirrored. */
int32_t psam_mask_intersections(const uint64_t* a, const uint64_t* b, int32_t Ka, int32_t Kb, int32_t W, int32_t* inter, psam_stream_t stream);
/* Greedy non-maximum suppression on the device.  order [K] = a permutation of the candidates, best first; candidate i (taken in order) is kept
 * iff valid[i] and no already kept j has (double)inter[i,j] > (double)iou_thr * (double)(area[i] + area[j] - inter[i,j]).  keep [K] uint8.
 * K <= 16384; ws: psam_mask_nms_workspace_bytes(K) bytes, 8-byte aligned. */
size_t psam_mask_nms_workspace_bytes(int32_t K);
int32_t psam_mask_nms(const int32_t* order, const uint8_t* valid, const int32_t* area, const int32_t* inter, int32_t K, float iou_thr,
                      uint8_t* keep, void* ws, size_t ws_bytes, psam_stream_t stream);
/* labels [N] int32 = the rank (0, 1, ... among the kept masks in `order`) of the best kept mask that contains the point, -1 if none.
 * ws: psam_mask_paint_workspace_bytes(K) bytes, 4-byte aligned. */
size_t psam_mask_paint_workspace_bytes(int32_t K);
int32_t psam_mask_paint(const uint64_t* bits, const int32_t* order, const uint8_t* keep, int32_t K, int32_t N, int32_t* labels, void* ws,
                        size_t ws_bytes, psam_stream_t stream);

/* ---------------------------------------------------------------- full-resolution scenes */

/* A scan of M points is reduced to a working cloud (one real point per occupied voxel), the model runs on the working cloud, and every point of
 * the scan receives the result of its voxel's representative (point_sam_amd/scene.py).  Integer work and bit-for-bit copies only: every output is
 * exact and does not depend on the order in which the waves run.
 *
 * psam_voxel_downsample: xyz [M, 3] on the device, 0 < M <= 2^28; origin: three floats in HOST memory.  Cell of a point, per axis, in fp32 with every operation rounded on its own:
 *   c = floorf((x - origin) * inv_h), inv_h = fl32(1) / fl32(voxel size), computed by the caller.  Voxel key = cx | cy << 21 | cz << 42; the
 *   representative of a voxel is its point with the lowest index.  keep_idx[0 .. *count) = the representatives in increasing order (room for M
 *   entries), inv[i] = the position in keep_idx of point i's representative; keep_idx == inv == NULL: only *count is written.
 *   *flag = 1 if a coordinate is not finite or a cell falls outside [0, 2^21) on any axis, else 0 (the call clears it); with the flag raised the
 *   other outputs are in range but meaningless.  ws: psam_voxel_downsample_workspace_bytes(M) bytes, 16-byte aligned (an open-addressing table
 *   at load factor <= 0.5 and the scan's counters).  A null pointer, a bad M, an inv_h that is not finite and positive, or a short workspace: -1. */
size_t psam_voxel_downsample_workspace_bytes(int32_t M);
int32_t psam_voxel_downsample(const float* xyz, int32_t M, const float* origin, float inv_h, int64_t* keep_idx, int64_t* inv, int32_t* count,
                              int32_t* flag, void* ws, size_t ws_bytes, psam_stream_t stream);
/* dst[r, i] = src[r, inv[i]], i < M, for R rows of Nw 32-bit words copied bit for bit (fp32 logits, int32 labels); src_ld / dst_ld = row strides
 * in words.  inv is read once per point for all rows; an index outside [0, Nw) stores a zero word. */
int32_t psam_scene_expand_rows(const void* src, int64_t src_ld, const int64_t* inv, int32_t R, int32_t Nw, int32_t M, void* dst, int64_t dst_ld,
                               psam_stream_t stream);
/* Packed masks (the layout of psam_mask_pack): bit i of row k of bits_f [K, ceil(M / 64)] = bit inv[i] of row k of bits_w [K, ceil(Nw / 64)];
 * bits past M are zero.  area_f [K] (may be NULL) = the popcount of each full row, an integer sum. */
int32_t psam_scene_expand_bits(const uint64_t* bits_w, const int64_t* inv, int32_t K, int32_t Nw, int32_t M, uint64_t* bits_f, int32_t* area_f,
                               psam_stream_t stream);

/* ---------------------------------------------------------------- scene crops */

/* A ball of a scan -- centre c, radius r -- as a cloud of its own: its points normalised to (x - c) / r, reduced to one real point per occupied
 * voxel of the normalised ball, and the crop cloud's result pasted back into the scan (point_sam_amd/scene.py: build_crop).  One call selects,
 * normalises, voxel-reduces, compacts and gathers; every output is exact and does not depend on the order in which the waves run.
 *
 * psam_crop_downsample: xyz, rgb [M, 3] on the device, 0 < M <= 2^28; center: three floats in HOST memory; r2 = fl32(r) * fl32(r),
 *   inv_r = fl32(1) / fl32(r), inv_h = fl32(1) / fl32(voxel size in crop units) or 0 for no voxel reduction, all computed by the caller.  In fp32
 *   with every operation rounded on its own:
 *     member      d = x - c per axis, q = (dx dx + dy dy) + dz dz; a point is a member iff q <= r2 (NaN compares false: a non-finite point is
 *                 not a member, and not an error)
 *     coordinate  u = fminf(fmaxf(d * inv_r, -1), 1) per axis
 *     cell        floorf((u - (-1)) * inv_h) per axis, the cell of psam_voxel_downsample at origin (-1, -1, -1); key = cx | cy << 21 | cz << 42.
 *                 The representative of a voxel is its MEMBER with the lowest scan index (points off the ball never enter the table); with
 *                 inv_h == 0 every member is its own representative.
 *   keep_idx[0 .. count) = the representatives' scan indices, increasing; inv[i] = the position in keep_idx of member i's representative, -1 for
 *   a non-member; wxyz[j] = u of point keep_idx[j]; wrgb[j] = rgb[keep_idx[j]] copied bit for bit.  keep_idx, wxyz and wrgb need room for M
 *   entries.  keep_idx == inv == wxyz == wrgb == NULL (rgb may then be NULL): counts only.
 *   result: three adjacent int32 on the device, cleared by the call: result[0] = count, result[1] = the number of members, result[2] = 1 if a
 *   member's cell falls outside [0, 2^21) on any axis (the other outputs are then in range but meaningless), else 0.
 *   ws: psam_crop_downsample_workspace_bytes(M) bytes, 16-byte aligned.  A null pointer, a bad M, a centre that is not finite, r2 / inv_r not
 *   finite and positive, inv_h negative or not finite, or a short workspace: -1. */
size_t psam_crop_downsample_workspace_bytes(int32_t M);
int32_t psam_crop_downsample(const float* xyz, const float* rgb, int32_t M, const float* center, float r2, float inv_r, float inv_h,
                             int64_t* keep_idx, int64_t* inv, float* wxyz, float* wrgb, int32_t* result, void* ws, size_t ws_bytes,
                             psam_stream_t stream);
/* dst[r, i] = inv[i] in [0, Nw) ? src[r, inv[i]] : fill, i < M, for R rows of 32-bit words copied bit for bit; fill is a 32-bit pattern
 * (0xFF800000 = -inf for fp32 logits, 0xFFFFFFFF = -1 for int32 labels); src_ld / dst_ld = row strides in words. */
int32_t psam_crop_expand_rows(const void* src, int64_t src_ld, const int64_t* inv, int32_t R, int32_t Nw, int32_t M, uint32_t fill, void* dst,
                              int64_t dst_ld, psam_stream_t stream);
/* Packed masks: bit i of row k of bits_f [K, ceil(M / 64)] = inv[i] in [0, Nw) ? bit inv[i] of row k of bits_w [K, ceil(Nw / 64)] : 0; bits
 * past M are zero.  area_f [K] (may be NULL) = the popcount of each full row. */
int32_t psam_crop_expand_bits(const uint64_t* bits_w, const int64_t* inv, int32_t K, int32_t Nw, int32_t M, uint64_t* bits_f, int32_t* area_f,
                              psam_stream_t stream);

/* ---------------------------------------------------------------- interpolated scene masks */

/* The last step of a scene or a crop with smooth edges (point_sam_amd/scene.py: build_interp_plan): a scan point receives the inverse-distance blend
 * of up to three working points instead of its voxel representative's value.  The arithmetic follows the model's own feature upsampling
 * (common.py:238-274 of the reference, psam_three_nn / psam_interp3 here); the candidates are the grid's.  All arithmetic is fp32, every operation
 * rounded on its own, division IEEE; every output is a function of the inputs alone.  No call allocates or synchronises with the host.
 *
 * This is NOT a true 3-NN: a working point two cells away can be nearer than the third candidate.  The definition is the 27-cell one below.  Measured
 * on the CPU (uniform clouds and sphere surfaces, 2 - 130 points per voxel): the 27 candidates contain the true nearest working point for 100 % of
 * 20 000 sampled scan points per case and the true three nearest for 99.9 %; the voxel's own representative is the nearest for only 51 - 72 %.
 *
 * Plan (common.py:238-255).  xyz [M, 3], inv [M] (the downsample's; a value outside [0, Nw), a crop's -1 among them, makes the point OFF),
 *   wxyz [Nw, 3] the working cloud as the encoder saw it, nbr [Nw, 26] of psam_region_neighbors on the grid the working cloud was built on
 *   (8-byte aligned).  center == NULL: a scene, the query coordinate is p = xyz[i].  center: three floats in HOST memory, a crop: p = the crop's
 *   normalised coordinate fminf(fmaxf((x - c) * inv_r, -1), 1) per axis, the one psam_crop_downsample writes to wxyz.
 *     candidates  v = inv[i] and every nbr[v, o] in [0, Nw), o = 0 .. 25
 *     distance    q_r = (dx dx + dy dy) + dz dz, d = p - wxyz[r]
 *     selection   the three candidates lowest in (q, r), lexicographic: a tie goes to the lower rank; missing entries are idx = -1, w = 0
 *     exact hit   q_0 == 0, or a single candidate: idx3 = (r0, -1, -1), w3 = (1, 0, 0)
 *     otherwise   a_j = 1 / fmaxf(q_j, eps); s = a0 + a1, then s = s + a2 with a third candidate; w_j = a_j / s
 *     off point   idx3 = (-1, -1, -1), w3 = (0, 0, 0)
 *   idx3 [M, 3] int32, w3 [M, 3] fp32: 24 bytes per scan point.  Coordinates of points that are not off must be finite.  A null pointer, M or Nw
 *   outside (0, 2^28], a centre or inv_r that is not finite (inv_r also not positive), eps negative or not finite: -1; a misaligned pointer: -2. */
int32_t psam_interp_scene_plan(const float* xyz, int32_t M, const int64_t* inv, const float* wxyz, const int32_t* nbr, int32_t Nw,
                               const float* center, float inv_r, float eps, int32_t* idx3, float* w3, psam_stream_t stream);
/* Apply (common.py:258-274), R fp32 rows; src_ld / dst_ld = row strides in floats; idx3 and w3 are read once per point for all rows.  An entry of
 * idx3 outside [0, Nw) is unused and never dereferenced; entries are used in order (without the first the point is off, without the second the
 * third is ignored).  With l_j = src[r, idx_j]:
 *     off point           dst[r, i] = fill
 *     idx_1 unused        the 32-bit word src[r, idx_0] is COPIED: no arithmetic, NaN payloads and infinities survive
 *     otherwise           acc = w0 l0 + w1 l1, then acc = acc + w2 l2 if idx_2 is used
 * so dst[r, keep_idx[j]] == src[r, j] bit for bit for a plan of psam_interp_scene_plan (a representative is an exact hit). */
int32_t psam_interp_scene_rows(const float* src, int64_t src_ld, const int32_t* idx3, const float* w3, int32_t R, int32_t Nw, int32_t M,
                               float fill, float* dst, int64_t dst_ld, psam_stream_t stream);
/* The packed masks of the same values without the [K, M] floats in between (the layout of psam_mask_pack): bit i of row k of
 * bits_f [K, ceil(M / 64)] = value[k, i] > thr, fp32 compare: NaN is false; an off point is 0; bits past M are zero.  area_f [K] (may be NULL) = the
 * popcount of each row, an integer sum. */
int32_t psam_interp_scene_bits(const float* src, int64_t src_ld, const int32_t* idx3, const float* w3, int32_t K, int32_t Nw, int32_t M,
                               float thr, uint64_t* bits_f, int32_t* area_f, psam_stream_t stream);

/* ---------------------------------------------------------------- masks carried to another cloud */

/* A radius-limited 3-NN search from the points of one cloud into ANOTHER cloud (point_sam_amd/transfer.py), written as a plan in the format of
 * psam_interp_scene_plan: psam_interp_scene_rows / psam_interp_scene_bits apply it unchanged (Nw = N).  All arithmetic is fp32, every operation
 * rounded on its own; every output is a function of the inputs alone.  No call allocates or synchronises with the host.
 *
 * src [N, 3] the sources, qry [M, 3] the queries, r the radius: h = r, inv_h = fl32(1 / r), r2 = fl32(r * r); origin: three floats in HOST memory
 * (the Python host takes fl32(min of the sources per axis - r)); pose: NULL, or 12 floats in HOST memory, row-major 3 x 4, query frame -> source frame.
 *     query coordinate  p = qry[i] bit for bit without a pose, else p_a = ((P[a][0] x + P[a][1] y) + P[a][2] z) + P[a][3]
 *     cells             those of the voxel downsample with (origin, inv_h); a source without a cell (not finite, or outside [0, 2^21) on an axis) is
 *                       never a candidate, a query without a cell has no candidates
 *     candidates        every source j whose cell differs from cell(p) by at most 1 on every axis (cells outside [0, 2^21) hold nothing) and whose
 *                       q_j = (dx dx + dy dy) + dz dz <= r2, d = p - src[j]; NaN compares false
 *     selection, weights, exact hit (q_0 == 0 or a lone candidate: a copy), unused entries: psam_interp_scene_plan's, ordered by (q, j), eps its eps
 *     no candidate      idx3 = (-1, -1, -1), w3 = (0, 0, 0)
 * The 27-cell set IS the definition.  It equals the true radius-r search except where the fp32 rounding of (x - origin) * inv_h moves a point across
 * a cell face while the two points lie at distance ~ r: a source with q <= r2 can then sit two cells away and is not seen.
 *
 * The index (workspace, 16-byte aligned, psam_transfer_index_workspace_bytes(N) bytes, 0 for N outside (0, 2^28]) belongs to (src, N, origin, inv_h):
 * psam_transfer_plan must be given the same four.  Its layout is private; results do not depend on the order in which sources arrived in it.
 * A null pointer, N or M outside (0, 2^28], inv_h, r2 or eps not finite and positive, an origin or pose that is not finite: -1; a misaligned
 * pointer: -2; a short workspace: -3. */
size_t psam_transfer_index_workspace_bytes(int32_t N);
int32_t psam_transfer_index_build(const float* src, int32_t N, const float* origin, float inv_h, void* ws, size_t ws_bytes, psam_stream_t stream);
int32_t psam_transfer_plan(const float* src, int32_t N, const void* ws, size_t ws_bytes, const float* origin, float inv_h, float r2,
                           const float* qry, int32_t M, const float* pose, float eps, int32_t* idx3, float* w3, psam_stream_t stream);

/* ---------------------------------------------------------------- pose between two clouds */

/* One step of point-to-point ICP on the index above (point_sam_amd/align.py): per query its nearest source within a radius, fused with the sums over
 * those pairs from which the host solves for the rigid motion.  No per-point intermediate is formed unless `nearest` is asked for; no float atomics.
 * The call allocates nothing and does not synchronise with the host.
 *
 * src, N, index_ws, origin, inv_h: the four the index was built from and its workspace (psam_transfer_index_build).  qry [M, 3] the queries; pose: NULL
 * (identity), or 12 floats in HOST memory, row-major 3 x 4, query frame -> source frame.  qry_bits: NULL (every query takes part), or ceil(M / 64)
 * words in the layout of psam_mask_pack: query i takes part when bit i is set; bits past M are IGNORED whatever the caller left there.
 *     posed coordinate  p: psam_transfer_plan's, bit for bit
 *     candidates        psam_transfer_plan's: the indexed sources j of the 27 cells around cell(p) with q_j = (dx dx + dy dy) + dz dz <= r2, d = p - src[j],
 *                       in the same fp32 arithmetic; NaN compares false.  The 27-cell set IS the definition.  r2 is any finite positive value: below
 *                       the index's own fl32(r * r) it shrinks the search without a rebuild; above it the 27 cells truncate the search
 *     pair              the candidate lowest in (q, j); a query without a candidate, without a cell, or that takes no part has none
 *     nearest [M]       (may be NULL) the pair's j, -1 without one
 * sums [PSAM_ALIGN_SUMS] f64 on the device, over the paired queries, x = the query AS GIVEN (not posed), s = src[pair], both converted to fp64:
 *     [0] the number of pairs   [1] sum q (the pair's fp32 q, converted)   [2..4] sum x   [5..7] sum s   [8..16] sum x_a s_b, row-major
 *     [17] sum |x|^2   [18] sum |s|^2   [19] the number of participating queries that have a cell (paired or not)
 *   Every TERM is exact in fp64 (a converted fp32 value, or the product of two: 48 significant bits; |x|^2 and |s|^2 enter as their three products);
 *   only the additions round, each an IEEE fp64 addition.  Order of the additions, fixed: lane l of wave w holds query 64 w + l and adds its terms
 *   starting from 0; the 64 lanes are combined by the xor butterfly 32, 16, 8, 4, 2, 1; a second kernel adds the waves' partials in wave order within
 *   32 segments of ceil(ceil(M / 64) / 32) consecutive waves, then the segments in order.  The order is a function of M alone -- not of the bits, the
 *   pose, the data or the schedule: the same inputs give the same twenty words from run to run.  The counts are exact integers.
 *   Error of the others: |sums - exact| <= (n - 1) u / (1 - (n - 1) u) * sum |term|, u = 2^-53, n the number of terms -- the bound of ANY order.
 * ws: psam_align_workspace_bytes(M) bytes (0 for M outside (0, 2^28]), 8-byte aligned.
 * Every refusal comes before any launch and leaves sums untouched: a null pointer (qry_bits, pose and nearest excepted), N or M outside (0, 2^28],
 * inv_h or r2 not finite and positive, an origin or pose that is not finite: -1; a misaligned pointer (index_ws 16 bytes; sums, ws and qry_bits 8;
 * src, qry and nearest 4): -2; a short index_ws or ws: -3. */
#define PSAM_ALIGN_SUMS 20
size_t psam_align_workspace_bytes(int32_t M);
int32_t psam_align_step(const float* src, int32_t N, const void* index_ws, size_t index_ws_bytes, const float* origin, float inv_h, float r2,
                        const float* qry, int32_t M, const uint64_t* qry_bits, const float* pose, int32_t* nearest, double* sums, void* ws,
                        size_t ws_bytes, psam_stream_t stream);

/* One step of point-to-PLANE ICP on the same index (point_sam_amd/align.py: solve_plane): psam_align_step's pair per query, and the sums of the 6 x 6
 * normal equations of the linearised point-to-plane residual.  The call allocates nothing and does not synchronise with the host; no atomics.
 *
 * Every argument of psam_align_step means what it means there.  src_normals [N, 3] f32 (non-null, 4-byte aligned): one normal per source, taken as
 * given -- not normalised, either sign; psam_normals_voxel's output fits.
 *     pair, nearest     psam_align_step's, bit for bit: the same posed coordinate p, cells, candidates and order (q, j)
 *     used pair         one whose normal n has nn = (n_x n_x + n_y n_y) + n_z n_z, in fp32, finite and > 0: the (0, 0, 0) of a voxel below min_points
 *                       drops out, and so does a normal with a NaN or an infinity -- it enters no sum
 *     terms             p (the POSED coordinate's fp32 words; the query itself without a pose), s = src[pair] and n converted to fp64, then in fp64,
 *                       every operation rounded on its own: d = p - s; r = (d_x n_x + d_y n_y) + d_z n_z; c = p x n, c_x = p_y n_z - p_z n_y and
 *                       cyclic; J = (c_x, c_y, c_z, n_x, n_y, n_z)
 * sums [PSAM_PLANE_SUMS] f64 on the device:
 *     [0] the number of used pairs   [1] sum q over them (the pair's fp32 q, converted)   [2] sum r r   [3..8] sum J_a r
 *     [9..29] sum J_a J_b for a <= b, the upper triangle row-major: 00, 01, .., 05, 11, .., 55
 *     [30] the number of paired queries whose pair was not used   [31] the number of participating queries that have a cell (paired or not)
 *   Order of the additions, fixed, and psam_align_step's: lane l of wave w holds the one term of query 64 w + l; the 64 lanes are combined by the xor
 *   butterfly 32, 16, 8, 4, 2, 1; a second kernel adds the waves' partials in wave order within 32 segments of ceil(ceil(M / 64) / 32) consecutive
 *   waves, then the segments in order.  A function of M alone: the same inputs give the same thirty-two words from run to run.  The counts are exact.
 *   Error of the others: |sums - sum of the terms| <= (n - 1) u / (1 - (n - 1) u) * sum |term|, u = 2^-53, n the number of terms.
 * ws: psam_plane_workspace_bytes(M) bytes (0 for M outside (0, 2^28]), 8-byte aligned.
 * Refusals: psam_align_step's codes in its order, before any launch, sums untouched; src_normals counts among the pointers that may not be null (-1)
 * and must be 4-byte aligned (-2). */
#define PSAM_PLANE_SUMS 32
size_t psam_plane_workspace_bytes(int32_t M);
int32_t psam_plane_step(const float* src, const float* src_normals, int32_t N, const void* index_ws, size_t index_ws_bytes, const float* origin,
                        float inv_h, float r2, const float* qry, int32_t M, const uint64_t* qry_bits, const float* pose, int32_t* nearest, double* sums,
                        void* ws, size_t ws_bytes, psam_stream_t stream);

/* The score of a global pose search (point_sam_amd/align.py: search): under each of P poses, the number of queries that land on the indexed cloud.
 * One launch for all P poses; the call allocates nothing, needs no workspace and does not synchronise with the host.
 *
 * src, N, index_ws, origin, inv_h, r2, qry [M, 3]: psam_align_step's.  poses [P, 12] f32 in DEVICE memory, each row-major 3 x 4, query frame ->
 * source frame.  counts [P] int32 on the device:
 *     counts[p]         the number of queries i with AT LEAST ONE candidate under pose p
 *     posed coordinate  p_a = ((P[a][0] x + P[a][1] y) + P[a][2] z) + P[a][3]: psam_transfer_plan's, bit for bit
 *     candidates        psam_align_step's: the indexed sources j of the 27 cells around cell(p) with q_j = (dx dx + dy dy) + dz dz <= r2, d = p - src[j],
 *                       in the same fp32 arithmetic; NaN compares false.  The 27-cell set IS the definition, no cell is pruned by a geometric bound.
 *                       r2 at or below the index's own fl32(r * r); above it the 27 cells truncate the search
 *     no hit            a query without a cell -- one that is not finite, or whose posed coordinate is not finite or outside [0, 2^21) cells on an axis
 *   Hence counts[p] == sums[0] of psam_align_step with pose p, the same r2 and no qry_bits, for every p.  Existence needs no order among the
 *   candidates: the walk visits psam_align_step's cells and chains in the same order under the same step bound and stops at the first hit.  The
 *   counts are integers added with integer atomics onto words the call itself clears on the stream: exact, and independent of schedule and order.
 * The poses are in device memory, so this entry CANNOT validate them: the caller does, before the upload (ops.align_score: every entry finite).  A
 * pose that is not finite yields coordinates that are not finite and a count of 0.
 * Limits: 0 < N, M <= 2^28, 0 < P <= 2^20.  Every refusal comes before any launch and leaves counts untouched: a null pointer, N, M or P outside its
 * range, inv_h or r2 not finite and positive, an origin that is not finite: -1; a misaligned pointer (index_ws 16 bytes; src, qry, poses and counts
 * 4): -2; a short index_ws: -3. */
#define PSAM_ALIGN_SCORE_POSES 4      /* poses per workgroup: a chunk of the grid (query tiles x pose chunks) */
int32_t psam_pose_score(const float* src, int32_t N, const void* index_ws, size_t index_ws_bytes, const float* origin, float inv_h, float r2,
                         const float* qry, int32_t M, const float* poses, int32_t P, int32_t* counts, psam_stream_t stream);

/* ---------------------------------------------------------------- camera views */

/* A picture of a cloud and the way back from it (point_sam_amd/views.py): a z-buffer of point splats, the point under a pixel, packed masks painted
 * into the image, image masks lifted to packed masks of the points visible in the view.  All arithmetic is fp32, every operation rounded on its own,
 * division IEEE; every output is a function of the inputs alone.  No call allocates, creates a stream or an event, or synchronises with the host.
 *
 * Camera.  pose: 12 floats in HOST memory, row-major 3 x 4, from the cloud's frame to the camera's (the convention of psam_transfer_plan's pose);
 *   fx, fy finite and > 0, cx, cy finite; width, height in [1, 8192]; near finite and > 0.  The camera looks along +z of its frame.
 * Projection of point i = (x, y, z):
 *     c_a = ((P[a][0] x + P[a][1] y) + P[a][2] z) + P[a][3]
 *     u = fx (c_x / c_z) + cx,  v = fy (c_y / c_z) + cy
 *     in view   iff c_z >= near, c_z is finite, 0 <= u < width and 0 <= v < height: fp32 compares, a NaN is false everywhere, and the compares come
 *               before any conversion to an integer (u = -0.0 is in pixel 0, u == width is out, u ~ 1e30 is out)
 *     pixel     (floorf(u), floorf(v)), p = y * width + x
 *     key_i     (bits(c_z) << 32) | i as an unsigned 64-bit word; c_z > 0, so the bit order is the value order.  0 < N <= 2^28
 * Splat with footprint s in 0 .. 3: point i offers key_i to every pixel (px + dx, py + dy), |dx|, |dy| <= s, inside the image.  keys [height, width]
 *   uint64 holds the minimum key offered to each pixel, all ones where none was: the low word is the winner's index (-1 if empty), the high word its
 *   depth as a float (a NaN pattern if empty: read it as +inf).  The minimum of a set does not depend on the order of arrival and equal depths go to
 *   the lower index, so keys depends on (points, camera, s) alone.
 * Pick with window w in 0 .. 16: for a click at integer pixel (qx, qy) (pixels [P, 2] int32, x first; may lie outside the image), among the non-empty
 *   pixels (qx + dx, qy + dy), |dx|, |dy| <= w, inside the image the one lowest in (dx dx + dy dy, key); point_index [P] = its point index, -1 if none.
 * Paint, bits [K, ceil(N / 64)] in the layout of psam_mask_pack: a pixel whose key is empty or whose index is not below N (checked before a bit word is
 *   read: keys of another cloud give a wrong picture, not a wild load) has no point.
 *     ids [height, width] int32            the lowest row k whose bit for the pixel's point is set (proposals are best first), -1 if none or no point
 *     rows [K, height, width] uint8        that bit of row k, 0 without a point
 * Lift, img [K, height, width] uint8 and tau >= 0 (+inf allowed): bit i of row k of bits [K, ceil(N / 64)] iff point i is in view with centre pixel p,
 *   keys[p] is not empty, c_z <= depth(keys[p]) + tau (one rounded add) and img[k, p] != 0.  img == NULL: K must be 1, every pixel counts as set -- the
 *   VISIBLE SET of the view.  Bits past N are zero; area [K] (may be NULL) = the rows' popcounts.  keys must be psam_view_splat's for the same points
 *   and camera (any s).
 * A null pointer, N outside (0, 2^28], a side outside [1, 8192], s outside 0 .. 3, w outside 0 .. 16, fx, fy or near not finite and positive, cx, cy or
 * a pose entry not finite, tau negative or NaN, K or P < 1: -1, before any launch; a misaligned pointer: -2. */
int32_t psam_view_splat(const float* xyz, int32_t N, const float* pose, float fx, float fy, float cx, float cy, int32_t width, int32_t height,
                        float znear, int32_t s, uint64_t* keys, psam_stream_t stream);
int32_t psam_view_pick(const uint64_t* keys, int32_t width, int32_t height, const int32_t* pixels, int32_t P, int32_t w, int32_t* point_index,
                       psam_stream_t stream);
int32_t psam_view_paint_ids(const uint64_t* keys, int32_t width, int32_t height, const uint64_t* bits, int32_t K, int32_t N, int32_t* ids,
                            psam_stream_t stream);
int32_t psam_view_paint_rows(const uint64_t* keys, int32_t width, int32_t height, const uint64_t* bits, int32_t K, int32_t N, uint8_t* rows,
                             psam_stream_t stream);
int32_t psam_view_lift_bits(const float* xyz, int32_t N, const float* pose, float fx, float fy, float cx, float cy, int32_t width, int32_t height,
                            float znear, const uint64_t* keys, const uint8_t* img, int32_t K, float tau, uint64_t* bits, int32_t* area,
                            psam_stream_t stream);

/* ---------------------------------------------------------------- RGB-D frames */

/* From pictures to a scan (point_sam_amd/views.py: FrameSet): F depth images with colour and a camera each are unprojected into one compacted scan,
 * and every frame becomes a view of that scan whose keys point at each pixel's OWN point -- the keys psam_view_pick, the two paints and
 * psam_view_lift_bits take, dense and without a splat footprint.  All arithmetic is fp32, every operation rounded on its own, division IEEE; there
 * are no atomics: every output bit is a function of the inputs alone.  No call allocates, creates a stream or an event, or synchronises with the host.
 *
 * Inputs.  depth [F, H, W]: fp32 (depth_u16 = 0), or uint16 with a depth_scale (depth_u16 = 1), measured along the camera's +z in the cameras' world
 *   units.  rgb [F, H, W, 3]: uint8 (rgb_u8 = 1), or fp32 already in the trained convention (rgb_u8 = 0).  cameras [F, 18] fp32 in DEVICE memory, one
 *   row per frame: the 12 pose words (world -> camera, row-major 3 x 4), then fx, fy, cx, cy, near, far.  The rotation must be orthonormal (the Python
 *   host checks max|R R^T - I| <= 1e-4 in fp64): the inverse used below is the transpose.  The table is device memory and is not inspected by the entry
 *   point; the Python host validates it (far > near, far finite) before the call, and a row whose near or far is a NaN keeps no pixel.
 *   edge: 0 = no edge filter, or a finite number > 0.  1 <= F, sides in 1 .. 8192, F H W <= 2^28.
 * Depth value   fp32: d = the word.  uint16: d = (float)raw * depth_scale, one rounded multiply.
 * Range-valid   d finite and d >= near and d <= far: fp32 compares, false for a NaN.  A raw uint16 0 fails d >= near.
 * Edge filter   a range-valid pixel is dropped iff one of its four neighbours (x +- 1, y +- 1) is inside the image, in the same frame, range-valid, and
 *               has fabsf(d - d_n) > edge * d: one rounded subtraction, one rounded product with this pixel's own d.  Neighbours outside the image
 *               or not range-valid do not count.
 * Kept          a pixel is kept iff it is range-valid and not dropped.  The scan's point order is the kept pixels in ascending (f, y, x);
 *               index [F, H, W] int32 holds a kept pixel's position in that order, -1 elsewhere; *count (DEVICE memory) = M, the number kept.
 * Unprojection  a = (((float)x + 0.5f) - cx) / fx,  b = (((float)y + 0.5f) - cy) / fy,  c = (a d, b d, d),  q_i = c_i - P[i][3],
 *               p_j = ((P[0][j] q_0 + P[1][j] q_1) + P[2][j] q_2): xyz [M, 3], the world point.
 * Colour        uint8: ((float)v / 255.0f - 0.5f) / 0.5f; fp32: copied.  rgb_out [M, 3].
 *   xyz, rgb_out need room for F H W points.  ws: the frames workspace-bytes query below gives its size (0 for a shape outside the limits), 16-byte aligned.
 * Finish.  center: three floats in HOST memory, scale > 0: n_j = (p_j - m_j) / s in place, one subtraction and one division.  poses [F, 12] fp32 in
 *   DEVICE memory: the cameras' poses in the normalised frame, [R | (R m + t) / s] computed by the host in fp64 and rounded once (near / s goes with
 *   them; intrinsics are unchanged, the projection is scale-free).  keys [F, H, W] uint64: for a pixel with index i in [0, M) (checked before a point
 *   is read), z = the third component of the pose applied to n_i, ((P'[2][0] x + P'[2][1] y) + P'[2][2] z) + P'[2][3]; key = (bits(z) << 32) | i if z
 *   is finite and > 0, all ones otherwise (the point stays in the scan, only the pixel is left empty) and for every pixel without a point.  The depth
 *   stored is the one psam_view_lift_bits recomputes for the same point: a pixel's own point is visible at tau = 0 by construction.
 * A null pointer, a shape outside the limits, a flag that is not 0 or 1, depth_scale (16-bit depth only) or scale not finite and positive, edge
 * negative or not finite, a centre that is not finite, M outside [1, F H W]: -1; a misaligned pointer: -2; a short workspace: -3 -- all before any launch. */
size_t psam_frames_workspace_bytes(int32_t F, int32_t H, int32_t W);
int32_t psam_frames_unproject(const void* depth, int32_t depth_u16, float depth_scale, const void* rgb, int32_t rgb_u8, const float* cameras,
                              int32_t F, int32_t H, int32_t W, float edge, float* xyz, float* rgb_out, int32_t* index, int32_t* count,
                              void* ws, size_t ws_bytes, psam_stream_t stream);
int32_t psam_frames_finish(float* xyz, int32_t M, const int32_t* index, const float* poses, int32_t F, int32_t H, int32_t W, const float* center,
                           float scale, uint64_t* keys, psam_stream_t stream);

/* ---------------------------------------------------------------- label fusion */

/* From the 2-D segmentations of many views to one 3-D labelling of the cloud (point_sam_amd/fusion.py).  V views of one size H x W show one cloud
 * xyz [N, 3]: keys [V, H, W] uint64 are the keys of psam_frames_finish, or psam_view_splat's of V cameras stacked; labels [V, H, W] int32 hold a
 * region id per pixel; cameras [V, 17] fp32 in DEVICE memory, one row per view: the 12 pose words (cloud -> camera, row-major 3 x 4), then fx, fy, cx,
 * cy, near -- the camera of "camera views", its width and height the W and H of the call.  The table is device memory and is not inspected by the
 * entry points; the Python host refuses a row that is not finite or whose fx, fy or near is not positive.  tau >= 0 (+inf allowed).  All arithmetic
 * is the projection's, fp32 with every operation rounded on its own; the rest is integers and bits.  There are no atomics: every output is a function
 * of the inputs alone.  No call allocates, creates a stream or an event, or synchronises with the host.
 *
 * Observation of point i in view v.  The point is VISIBLE iff it is in view (the projection of "camera views") with centre pixel p, keys[v][p] is not
 *   empty and c_z <= depth(keys[v][p]) + tau (one rounded add): the lift rule of psam_view_lift_bits, unchanged.  Its observed label is l =
 *   labels[v][p].  row_base [V + 1] int32 in DEVICE memory is the exclusive prefix of the views' region counts: count_v = row_base[v + 1] - row_base[v],
 *   R = row_base[V] (passed by value), region (v, l) is row row_base[v] + l.  l is VALID iff 0 <= l < count_v (and the row lies in [0, R), whatever
 *   the table holds: nothing is read or written outside the buffers); any other l, INT32_MIN and INT32_MAX included, is a visible but UNLABELLED
 *   observation.  Without row_base (psam_fuse_vote only: ids that already agree between the views) every l >= 0 is valid.
 * psam_fuse_region_bits: bits [R + V, ceil(N / 64)] in the layout of psam_mask_pack, area [R + V] (may be NULL) = the rows' popcounts.
 *   row row_base[v] + l   bit i iff point i is visible in view v with the valid label l: psam_view_lift_bits of the image labels[v] == l
 *   row R + v             bit i iff point i is visible in view v, labelled or not: psam_view_lift_bits without an image
 *   Bits at i >= N are zero.  0 <= R <= 2^20.
 * psam_fuse_vote.  The global label of a labelled observation is g = remap[row_base[v] + l] with remap [R] int32 (DEVICE memory, needs row_base), or
 *   g = l without a remap; a remap entry below 0 (a region that was empty where the links were made) leaves the observation unlabelled.  The views
 *   are walked in ascending v with a table of at most 8 distinct global labels in first-seen order, each with a count; an observation whose label is
 *   not in a full table is dropped.  Outputs, [N] int32 each:
 *     seen       the visible observations            labelled   those that carry a global label            dropped    those the full table refused
 *     label      the table entry with the highest count, ties to the LOWER LABEL (not the earlier view); -1 if the table is empty or that count is
 *                below min_votes (>= 1)
 *     votes      that count, 0 where label is -1
 * psam_label_bits: labels [N] int32 -> bits [K, ceil(N / 64)], area [K] (may be NULL): bit i of row k iff labels[i] == k; a value outside [0, K)
 *   sets nothing.  1 <= K <= 2^20.
 * A null pointer, N outside [1, 2^28], V outside [1, 4096], a side outside [1, 8192], R or K outside its range, tau negative or NaN, min_votes < 1, a
 * remap without row_base: -1; a misaligned pointer (keys and bits 8 bytes, every other 4): -2 -- all before any launch. */
int32_t psam_fuse_region_bits(const float* xyz, int32_t N, const float* cameras, int32_t V, int32_t H, int32_t W, const uint64_t* keys,
                              const int32_t* labels, const int32_t* row_base, int32_t R, float tau, uint64_t* bits, int32_t* area,
                              psam_stream_t stream);
int32_t psam_fuse_vote(const float* xyz, int32_t N, const float* cameras, int32_t V, int32_t H, int32_t W, const uint64_t* keys,
                       const int32_t* labels, const int32_t* row_base, const int32_t* remap, int32_t R, float tau, int32_t min_votes,
                       int32_t* label, int32_t* votes, int32_t* seen, int32_t* labelled, int32_t* dropped, psam_stream_t stream);
int32_t psam_label_bits(const int32_t* labels, int32_t N, int32_t K, uint64_t* bits, int32_t* area, psam_stream_t stream);

/* ---------------------------------------------------------------- connected components of masks */

/* Which points of a packed mask hang together, and the clean-up built on it (point_sam_amd/regions.py).  Cells are those of the voxel
 * downsample above (same origin and inv_h); keep_idx [V] and inv [N] are its outputs for the cloud at that voxel size.  Points i and j are
 * adjacent iff their cells differ by at most 1 on every axis; the components of a point set are those of the subgraph it induces.  A
 * component's id is the lowest inv[] among its points, its size its number of points.  Integers and bits only: every output is exact and does
 * not depend on the order in which the waves run.  No call allocates or synchronises with the host; a null pointer or a bad shape returns -1, a
 * short workspace -3, a workspace that is not 16-byte aligned -2.  K <= 65535 rows per call; N, V <= 2^28.
 *
 * Neighbours: nbr [V, 26] int32, entry o of voxel v = the rank (position in keep_idx) of the occupied voxel at v's cell + offset o, or -1; the
 *   offsets run over (dz, dy, dx) in {-1, 0, 1}^3 with dz slowest and (0, 0, 0) skipped, so offset 25 - o is the opposite of o.  A cell outside
 *   [0, 2^21) on an axis is -1.  origin: three floats in HOST memory. */
size_t psam_region_neighbors_workspace_bytes(int32_t V);
int32_t psam_region_neighbors(const float* xyz, const int64_t* keep_idx, int32_t V, const float* origin, float inv_h, int32_t* nbr, void* ws,
                              size_t ws_bytes, psam_stream_t stream);
/* labels [K, N] int32: per point the id of its component within row k of bits [K, ceil(N / 64)] (the layout of the mask proposals), -1 outside
 *   the set; complement != 0: the set is the points below N that are NOT in the row. */
size_t psam_region_labels_workspace_bytes(int32_t K, int32_t N, int32_t V);
int32_t psam_region_labels(const uint64_t* bits, const int64_t* inv, const int32_t* nbr, int32_t K, int32_t N, int32_t V, int32_t complement,
                           int32_t* labels, void* ws, size_t ws_bytes, psam_stream_t stream);
/* Clean-up of every row with select[k] != 0 (select NULL: every row), in this order: (1) min_hole > 0: every component of the complement with
 *   fewer than min_hole points joins the mask; (2) min_island > 0: every component of the result with fewer than min_island points is removed,
 *   except the largest (size ties: the lowest id); (3) S > 0, seeds [K, S] int32 point indices, -1 = unused: if a seed of the row is a member
 *   after (2), only the components that hold such a seed stay.  An empty row stays empty; an unselected row is copied bit for bit.  bits_out
 *   [K, W] (must not alias bits; bits past N are zero), area_out [K] = the popcounts, changed [K] uint8 = the row differs from its input. */
size_t psam_region_clean_workspace_bytes(int32_t K, int32_t N, int32_t V, int32_t S);
int32_t psam_region_clean(const uint64_t* bits, const uint8_t* select, const int64_t* inv, const int32_t* nbr, const int32_t* seeds, int32_t K,
                          int32_t N, int32_t V, int32_t S, int32_t min_island, int32_t min_hole, uint64_t* bits_out, int32_t* area_out,
                          uint8_t* changed, void* ws, size_t ws_bytes, psam_stream_t stream);

/* ---------------------------------------------------------------- instance geometry */

/* Where a packed mask is, how big it is and what colour it has (point_sam_amd/geometry.py), straight from the bits: the work follows the set bits,
 * no [K, N] matrix is formed.  bits [K, W] in the layout of the mask proposals, W = ceil(N / 64); a bit at a position >= N is IGNORED whatever
 * the caller left there, and xyz / rgb are never read at an index >= N.  S_k = the member points of row k.  0 < K <= 65535, 0 < N <= 2^28.  No call
 * allocates, creates a stream or an event, or synchronises with the host; the workspace is the caller's.  A null pointer, a bad size or a short
 * workspace returns -1, a misaligned pointer -2, with psam_last_error_string set.
 *
 * A wave owns PSAM_INSTANCE_RANGE_WORDS consecutive words of a row; a row of more words is split over ceil(W / PSAM_INSTANCE_RANGE_WORDS) waves whose
 * partial results are combined in range order by a second kernel.
 *
 * psam_instance_moments: xyz [N, 3] f32, rgb [N, 3] f32 or NULL.
 *   count [K] int32   |S_k|, an exact integer
 *   lo, hi [K, 3] f32 the component-wise minimum / maximum of the members' coordinates in the order -inf < .. < -0 < +0 < .. < +inf: exact and
 *                     independent of any order; an empty row gives +inf / -inf
 *   sums [K, 12] f64  sum x, sum y, sum z, sum xx, sum xy, sum xz, sum yy, sum yz, sum zz, sum r, sum g, sum b over S_k.  Every TERM is formed in
 *                     fp64 from the fp32 inputs and is exact (the conversion, and the product of two converted values: 48 significant bits); only
 *                     the additions round, each an IEEE fp64 addition.  With rgb == NULL the last three are 0; an empty row gives twelve zeros.
 *   Order of the additions, fixed: a lane of the wave adds the points of words base + lane, base + 64 + lane, base + 128 + lane, base + 192 + lane
 *   of its range, bits ascending, into its own accumulators starting from 0; the 64 lanes are combined by the xor butterfly 32, 16, 8, 4, 2, 1; the
 *   row's ranges are added in increasing order starting from 0 (a range without members contributes an exact 0).  The order depends on N and on
 *   the row's own bits only: row k gives the same bits from run to run, and the same bits computed alone or among K others.  No float atomics.
 *   Error: |sums - exact| <= (n - 1) u / (1 - (n - 1) u) * sum |term|, u = 2^-53, n = count -- the bound of ANY order of n - 1 additions.
 *   Coordinates are assumed finite; non-finite input does not fault, its results are unspecified.
 *   ws: psam_instance_moments_workspace_bytes(K, N) bytes (0 for a bad shape), 8-byte aligned. */
#define PSAM_INSTANCE_RANGE_WORDS 256
size_t psam_instance_moments_workspace_bytes(int32_t K, int32_t N);
int32_t psam_instance_moments(const float* xyz, const float* rgb, const uint64_t* bits, int32_t K, int32_t N, int32_t* count, double* sums,
                              float* lo, float* hi, void* ws, size_t ws_bytes, psam_stream_t stream);
/* psam_instance_extents: the members of row k in the frame origin [K, 3], axes [K, 3, 3] (row i of axes[k] = axis i; NULL: the identity, p = d), all
 *   on the device.  In fp32, every operation rounded on its own and in exactly this order, per member point:
 *     d   = (x - ox, y - oy, z - oz)
 *     p_i = (d.x a_i0 + d.y a_i1) + d.z a_i2, i = 0, 1, 2                 (the axes need not be orthonormal: nothing assumes it)
 *     r2  = (d.x d.x + d.y d.y) + d.z d.z
 *   lo, hi [K, 3] = the component-wise minimum / maximum of p, r2max [K] = the maximum of r2, in the order above (exact, order-independent); an
 *   empty row gives +inf / -inf / -inf.  ws: psam_instance_extents_workspace_bytes(K, N) bytes, 4-byte aligned. */
size_t psam_instance_extents_workspace_bytes(int32_t K, int32_t N);
int32_t psam_instance_extents(const float* xyz, const uint64_t* bits, int32_t K, int32_t N, const float* origin, const float* axes, float* lo,
                              float* hi, float* r2max, void* ws, size_t ws_bytes, psam_stream_t stream);

/* ---------------------------------------------------------------- normals and superpoints */

/* Surface normals per occupied voxel, a geometric over-segmentation of the cloud grown from them, and the snapping of packed masks to whole segments
 * (point_sam_amd/superpoints.py).  The graph is that of the connected components above: inv [N] of psam_voxel_downsample at origin (-1, -1, -1), nbr
 * [V, 26] of psam_region_neighbors; a point whose inv is outside [0, V) has no cell.  No call allocates or synchronises with the host; the workspace is
 * the caller's, 16-byte aligned.  A null pointer or a bad shape returns -1, a short workspace -3, a misaligned pointer -2, all before any launch.
 * 0 < N <= 2^28, 0 < V <= N.
 *
 * psam_normals_voxel.  The neighbourhood of voxel v is every point whose voxel is v or one of nbr[v, 0 .. 25]; all points of a voxel share its normal.
 *   Fixed point: a coordinate p in [-1, 1] has q = floor((double)p * 2^20) + 2^20, an integer in [0, 2^21]; every step is exact.  A point with a
 *   coordinate that is not finite or outside [-1, 1] takes part in no neighbourhood.
 *   With the neighbourhood's n points, s = sum q and P = sum q q^T:  S = n P - s s^T, formed EXACTLY in integer arithmetic (128-bit where needed; no
 *   accepted shape overflows, csrc/normals.hip) and converted to fp64 once, to nearest even.  S does not depend on the order of the points, on any
 *   translation of q by integers, or on the launch schedule.
 *   count [V] int32       n
 *   scatter [V, 6] f64    S: xx, xy, xz, yy, yz, zz; may be NULL
 *   normal [V, 3] f32     the unit eigenvector of the smallest eigenvalue of S, solved in fp64 (cyclic Jacobi on S scaled by a power of two), rounded
 *                         to fp32.  Sign, decided on the fp32 values: without a viewpoint the component of largest magnitude is positive, on a tie
 *                         the lowest axis decides; with viewpoint [3] (HOST memory, finite) the sign gives n . (viewpoint - mean) >= 0 in fp64, mean =
 *                         (s / n - 2^20) 2^-20 per axis.
 *   curvature [V] f32     l0 / (l0 + l1 + l2) of the eigenvalues l0 <= l1 <= l2 (l0 not below 0), 0 when the sum is 0
 *   A voxel with n < min_points (>= 1; an exact integer test) gets normal (0, 0, 0) and curvature 0.
 *   ws: psam_normals_voxel_workspace_bytes(N, V) = 128 V bytes (sixteen 64-bit integer sums per voxel). */
size_t psam_normals_voxel_workspace_bytes(int32_t N, int32_t V);
int32_t psam_normals_voxel(const float* xyz, const int64_t* inv, const int32_t* nbr, int32_t N, int32_t V, int32_t min_points, const float* viewpoint,
                           int32_t* count, double* scatter, float* normal, float* curvature, void* ws, size_t ws_bytes, psam_stream_t stream);
/* psam_superpoints: count, normal, curvature as psam_normals_voxel wrote them.  Call voxel v smooth iff count[v] >= min_points and curvature[v] <=
 *   max_curvature, and let d(v, u) = |(x x' + y y') + z z'| in fp64 from the stored fp32 normals of v and u, every operation rounded on its own.
 *   Union.   Edge (v, u = nbr[v, o]) joins the two voxels iff both are smooth and d(v, u) >= cos_angle.  The label of a component is its lowest voxel
 *            rank; the size of a label is the number of POINTS (inv in [0, V)) of its voxels.
 *   Absorb.  absorb_rounds (0 .. 64) times, every voxel reading the labels and sizes of the round's start: a voxel v whose label has fewer than
 *            min_size points takes, among its neighbours u whose label has at least min_size, the label of the one with the largest d(v, u) (a
 *            normal of (0, 0, 0) gives 0); a tie goes to the lower label; without such a neighbour it keeps its label.  Sizes are counted again
 *            after every round.  min_size = 0 absorbs nothing.
 *   Compact. The labels still in use become 0 .. S - 1 in increasing order of their value.
 *   voxel_label [V], point_label [N] = voxel_label[inv[i]] (-1 for a point without a cell), size [V; the first S written, the rest zero], *num = S (DEVICE
 *   memory), all int32.  ws: psam_superpoints_workspace_bytes(N, V). */
size_t psam_superpoints_workspace_bytes(int32_t N, int32_t V);
int32_t psam_superpoints(const int64_t* inv, const int32_t* nbr, const int32_t* count, const float* normal, const float* curvature, int32_t N, int32_t V,
                         int32_t min_points, float max_curvature, double cos_angle, int32_t min_size, int32_t absorb_rounds, int32_t* voxel_label,
                         int32_t* point_label, int32_t* size, int32_t* num, void* ws, size_t ws_bytes, psam_stream_t stream);
/* psam_superpoint_snap: bits [K, ceil(N / 64)] in the layout of the mask proposals (bits past N are ignored), point_label [N], size [S] of
 *   psam_superpoints, 0 < S <= N given by the caller, 0 <= q16 <= 65535, 0 < K <= 65535.  cnt[k, s] = the set bits of row k whose point has label s
 *   (a label outside [0, S) counts nowhere).  Bit i of row k of bits_out (must not alias bits; bits past N are zero) is set iff
 *       0 <= point_label[i] < S  and  (int64)cnt[k, point_label[i]] * 65536 > (int64)q16 * size[point_label[i]]
 *   q16 = 0: any touch selects the whole superpoint; q16 = 32768: a strict majority, and rows that were disjoint stay disjoint from there on.
 *   area_out [K] = the popcounts of bits_out, changed [K] uint8 = the row differs from its input below N.
 *   ws: psam_superpoint_snap_workspace_bytes(K, N, S) = the [K, S] int32 table, rounded up to 16 bytes. */
size_t psam_superpoint_snap_workspace_bytes(int32_t K, int32_t N, int32_t S);
int32_t psam_superpoint_snap(const uint64_t* bits, const int32_t* point_label, const int32_t* size, int32_t K, int32_t N, int32_t S, int32_t q16,
                             uint64_t* bits_out, int32_t* area_out, uint8_t* changed, void* ws, size_t ws_bytes, psam_stream_t stream);

/* ---------------------------------------------------------------- scan map */

/* A scan map accumulates posed scans into one persistent, labelled voxel map in the normalised frame (point_sam_amd/scanmap.py).  A map voxel is the
 * voxel of psam_voxel_downsample at origin (-1, -1, -1) and the map's inv_h, bit for bit.  The library allocates nothing and keeps no state: the map
 * lives in a block of the caller's, psam_map_bytes bytes of DEVICE memory, 16-byte aligned, and every entry takes the block with the two capacities
 * it was cleared with (0 < max_voxels, max_pairs <= 2^28).  A null pointer or a bad shape returns -1, a short block or workspace -3, a misaligned
 * pointer -2, all before any launch.  No call synchronises with the host.
 *
 * The block begins with PSAM_MAP_HEADER_INTS int32 words, which the caller may read back:
 *   0 max_voxels   1 max_pairs   2 inv_h (the bits of the float)   3 flags   4 V, the number of voxels   5 the number of adds so far
 *   6 the number of distinct (id, label) pairs   7 .. 9 of the last add: its new voxels, accepted points, rejected points
 *   10, 11 the accepted points of all adds, one uint64                12 .. 15 zero
 * flags != 0: the map is dead until it is cleared (1: an add would have passed max_voxels, 2: its pairs passed max_pairs, 4: its accepted points
 * would have passed 2^31 - 1 in total, the bound under which every count fits an int32 and every sum a 64-bit word).  Both capacity conditions are
 * functions of the inputs alone.  A dead map is never written outside its block, and its adds change nothing further.
 *
 * psam_map_clear.  Empties the map and sets inv_h (finite, positive; the voxel size is 1 / inv_h).
 * psam_map_add.  xyz, rgb [M, 3] fp32, labels [M] int32 or NULL, pose: 12 floats in HOST memory (row-major 3 x 4, scan frame -> map frame, finite) or
 *   NULL for the identity, which applies no arithmetic.  0 < M <= 2^28.  Point i:
 *     p = ((P[a][0] x + P[a][1] y) + P[a][2] z) + P[a][3] per axis, every fp32 operation rounded on its own;
 *     cell_a = floorf((p_a - (-1)) * inv_h), which must lie in [0, 2^21);  fixed point q = floor((double)v * 2^20) + 2^20 for v in [-1, 1].
 *   The point is accepted iff all three cells exist, -1 <= p_a <= 1 and -1 <= rgb <= 1 on every axis (a NaN compares false).  ids [M] int32: the
 *   voxel of an accepted point, -1 for a rejected one.  Voxel ids are dense and permanent: a voxel new in this add gets V_before + r, r its rank
 *   among the new voxels ordered by the lowest accepted point index in them.  Per voxel the map keeps count, sum q [3], sum of the colours' q [3]
 *   (exact integers), first_seen and last_seen (the number of the add, from 1), and per (voxel, label >= 0) the number of points: a negative label
 *   is an unlabelled observation.  ws: psam_map_add_workspace_bytes(M) bytes, 16-byte aligned.
 * psam_map_locate.  ids [M] of xyz under the pose: the same position test and cell, -1 where the map has no such voxel.  Changes nothing.
 * psam_map_labels.  label, votes [V] int32: per voxel the label with the most points, a tie going to the LOWER label; -1 and 0 where the best count
 *   is below min_votes (>= 1).  0 < V <= max_voxels; entries past the map's own V get -1 and 0.
 * psam_map_cloud.  xyz, rgb [V, 3] fp32 = fl32(fl64(fl64(sum) / fl64(count)) * 2^-20 - 1), every fp64 operation rounded on its own; zeros past V.
 * psam_map_fields.  count, first_seen, last_seen [V] int32, keys [V] int64 (cell_x | cell_y << 21 | cell_z << 42) and sums [V, 6] int64 (sum q of the
 *   position, then of the colour), each may be NULL (not all); past V: 0, 0, 0, -1, 0. */
#define PSAM_MAP_HEADER_INTS 16
size_t psam_map_bytes(int32_t max_voxels, int32_t max_pairs);
int32_t psam_map_clear(void* map, size_t map_bytes, int32_t max_voxels, int32_t max_pairs, float inv_h, psam_stream_t stream);
size_t psam_map_add_workspace_bytes(int32_t M);
int32_t psam_map_add(void* map, size_t map_bytes, int32_t max_voxels, int32_t max_pairs, const float* xyz, const float* rgb, const int32_t* labels,
                     int32_t M, const float* pose, int32_t* ids, void* ws, size_t ws_bytes, psam_stream_t stream);
int32_t psam_map_locate(const void* map, size_t map_bytes, int32_t max_voxels, int32_t max_pairs, const float* xyz, int32_t M, const float* pose,
                        int32_t* ids, psam_stream_t stream);
int32_t psam_map_labels(const void* map, size_t map_bytes, int32_t max_voxels, int32_t max_pairs, int32_t V, int32_t min_votes, int32_t* label,
                        int32_t* votes, psam_stream_t stream);
int32_t psam_map_cloud(const void* map, size_t map_bytes, int32_t max_voxels, int32_t max_pairs, int32_t V, float* xyz, float* rgb, psam_stream_t stream);
int32_t psam_map_fields(const void* map, size_t map_bytes, int32_t max_voxels, int32_t max_pairs, int32_t V, int32_t* count, int32_t* first_seen,
                        int32_t* last_seen, int64_t* keys, int64_t* sums, psam_stream_t stream);

/* ---------------------------------------------------------------- scan map carving */

/* Free-space carving of a scan map (ScanMap.carve): the cells between the sensor and what it measured were seen through, and a map voxel that rays
 * keep passing through is a ghost -- a person who walked by, a chair that was moved.  A carve never writes the map block and never adds a voxel: its
 * state lives in a second block of the caller's, psam_carve_bytes(max_voxels) = 64 + 16 max_voxels bytes of DEVICE memory, 16-byte aligned, cleared
 * by psam_carve_clear and used with one map of the same max_voxels.  Return codes as for the map entries; no call synchronises with the host.
 *
 * Cells and rays.  One carve takes a scan xyz [M, 3], its pose (as psam_map_add), a sensor origin (3 floats in HOST memory, the scan's frame, finite),
 * margin (0 <= margin < 2^21) and stamp (1 <= stamp <= 2^31 - 1).  A point's cell is psam_map_add's: the same pose arithmetic, the same acceptance
 * test (all three cells exist and -1 <= p_a <= 1; colour plays no part).  The origin goes through the same arithmetic on the device; if it has no
 * cell, no ray is cast (header word 3 = 0; hits are still marked).  Rays run from cell centre to cell centre, so two points in one cell give one
 * ray: the rays of a carve are its distinct accepted endpoint cells other than the origin's cell.  Against the true ray from the sensor to the point
 * this shifts a ray by at most half a voxel.
 *
 * The cells of a ray.  The ray from cell o to cell e crosses the cells c != o, e whose OPEN box meets the segment between the centres of o and e; a
 * segment that only touches an edge or a corner of a cell does not cross it.  The integer walk that enumerates exactly this set, in order: with
 * n_a = |e_a - o_a|, s_a = sign(e_a - o_a), k = (0, 0, 0), cur = o, repeat
 *   1. among the axes with k_a < n_a find the least (2 k_a + 1) / (2 n_a), compared as (2 k_a + 1) n_b < (2 k_b + 1) n_a (products below 2^43: exact);
 *   2. step every axis tied at the minimum: k_a += 1, cur_a += s_a;
 *   3. stop when cur == e; otherwise cur is a crossed cell.
 * The walk of (o, e) is the reverse of the walk of (e, o).  Right after the k-th crossing of the longest axis a (1 <= k <= n_a) every other axis has
 * k_b = min(n_b, ((2 k - 1) n_b + n_a) div (2 n_a)): a walk can start in the middle of a ray.
 *
 * What a carve changes.  Per map voxel id the block keeps four int32 words: hits, misses, last_hit, last_missed.
 *   hit     a map voxel that is an endpoint cell of this carve (the origin's cell included, where a point lies in it):
 *           if last_hit < stamp then hits += 1 and last_hit = stamp;
 *   missed  then, a map voxel that some ray crosses at Chebyshev distance > margin from that ray's end cell and that was not hit in this carve
 *           (last_hit != stamp): if last_missed < stamp then misses += 1 and last_missed = stamp.
 * So a voxel counts at most once per carve, and a hit beats a miss inside one carve (rays graze the near surface on their way to the far one).  hits
 * counts carves, not points.  The same carve again with the same stamp changes no voxel's words.  Set semantics over integers: the result is a
 * function of the inputs alone.  A dead map (flags != 0) is neither marked nor walked.
 *
 * The block begins with PSAM_CARVE_HEADER_INTS int32 words, which the caller may read back:
 *   0 max_voxels   1 carves so far (calls that raised the stamp)   2 the highest stamp   3 the last carve's origin has a cell
 *   4 .. 8 of the last call: rays, accepted points, rejected points, voxels whose hits it raised, voxels whose misses it raised   9 zero
 *   10, 11 one uint64: the crossed cells beyond the margin, summed over the rays of the last call (a function of the inputs)   12 .. 15 zero
 *
 * psam_carve_clear.  Zeroes every voxel's words and the header, sets word 0.
 * psam_carve_scan.  One carve; ws: psam_carve_workspace_bytes(M) bytes, 16-byte aligned; 0 < M <= 2^28.  Four launches.
 * psam_carve_fields.  hits, misses, last_hit, last_missed [V] int32, each may be NULL (not all); 0 < V <= max_voxels; voxels the map added after the
 *   last carve read 0. */
#define PSAM_CARVE_HEADER_INTS 16
size_t psam_carve_bytes(int32_t max_voxels);
int32_t psam_carve_clear(void* carve, size_t carve_bytes, int32_t max_voxels, psam_stream_t stream);
size_t psam_carve_workspace_bytes(int32_t M);
int32_t psam_carve_scan(const void* map, size_t map_bytes, int32_t max_voxels, int32_t max_pairs, void* carve, size_t carve_bytes, const float* xyz,
                        int32_t M, const float* pose, const float* origin, int32_t margin, int32_t stamp, void* ws, size_t ws_bytes, psam_stream_t stream);
int32_t psam_carve_fields(const void* carve, size_t carve_bytes, int32_t max_voxels, int32_t V, int32_t* hits, int32_t* misses, int32_t* last_hit,
                          int32_t* last_missed, psam_stream_t stream);

/* ---------------------------------------------------------------- scan map tracking */

/* One step of point-to-point ICP of a scan against a scan map (ScanMap.track_step, ScanMap.track): per query the nearest map voxel -- its mean
 * position -- within a radius, found by probing the map's own voxel table, fused with psam_align_step's twenty sums over those pairs.  No cloud is read
 * out of the map and no index is built.  The map block is only read.  The call allocates nothing, uses no atomics and does not synchronise with the host.
 *
 * map, map_bytes, max_voxels, max_pairs: the block as every psam_map_* entry takes it.  V: voxel ids below V are candidates (0 < V <= max_voxels;
 * normally the map's own V; ids the map has not given out are never found).  skip: NULL, or ceil(V / 64) words over voxel ids in the layout of
 * psam_mask_pack: a voxel whose bit is set is no candidate.  min_count >= 1: a voxel observed fewer times is no candidate.  reach in 1 .. 4.
 * qry [M, 3], qry_bits, pose (12 floats in HOST memory, scan frame -> map frame, or NULL: the query as given): psam_align_step's.
 *     takes part        query i, if qry_bits is NULL or its bit i is set; bits past M are ignored
 *     posed coordinate  p = ((P[a][0] x + P[a][1] y) + P[a][2] z) + P[a][3] per axis, every fp32 operation rounded on its own (psam_map_add's)
 *     cell              the query has a cell iff psam_map_add would accept p (colour apart): cell_a = floorf((p_a - (-1)) * inv_h) in [0, 2^21) and
 *                       -1 <= p_a <= 1 on every axis, inv_h the map header's.  Exactly the points psam_map_locate accepts
 *     candidates        the map voxels v whose cell is one of the (2 reach + 1)^3 cells around cell(p) (a cell with a coordinate below 0 or at or
 *                       above 2^21 is skipped), with v < V, count(v) >= min_count, the bit of v in skip clear, and
 *                       q = (dx dx + dy dy) + dz dz <= r2 in fp32, each operation rounded on its own, NaN false; d = p - s, s the voxel's mean position
 *                       with the bits psam_map_cloud gives it.  The cube of cells IS the definition: no cell is dropped by a geometric bound
 *     pair              the candidate lowest in (q, v).  Neither the probe order nor the schedule enters any output
 *     nearest [M]       (may be NULL) the pair's voxel id, -1 without one
 * sums [PSAM_ALIGN_SUMS] f64 on the device: psam_align_step's twenty words with s the voxel's mean, x the query AS GIVEN (not posed): every term exact
 *   in fp64, the additions in psam_align_step's fixed order (a function of M alone), [19] the number of participating queries that have a cell.
 *   The same inputs give the same twenty words from run to run.
 * ws: psam_track_workspace_bytes(M) = psam_align_workspace_bytes(M) bytes (0 for M outside (0, 2^28]), 8-byte aligned.
 * Every refusal comes before any launch and leaves sums and nearest untouched: a null map, qry, sums or ws, M outside (0, 2^28], V outside
 * (0, max_voxels], bad capacities, reach outside 1 .. 4, min_count < 1, r2 not finite and positive, a pose that is not finite: -1; a misaligned
 * pointer (map 16 bytes; sums, ws, skip and qry_bits 8; qry and nearest 4): -2; a short map block or ws: -3. */
#define PSAM_TRACK_MAX_REACH 4
size_t psam_track_workspace_bytes(int32_t M);
int32_t psam_track_step(const void* map, size_t map_bytes, int32_t max_voxels, int32_t max_pairs, int32_t V, const uint64_t* skip, int32_t min_count,
                        int32_t reach, float r2, const float* qry, int32_t M, const uint64_t* qry_bits, const float* pose, int32_t* nearest,
                        double* sums, void* ws, size_t ws_bytes, psam_stream_t stream);

/* One step of point-to-PLANE ICP of a scan against a scan map (ScanMap.track_plane_step, ScanMap.track with normals): psam_track_step's pair per
 * query, fused with psam_plane_step's thirty-two sums over the used pairs.  The map block is only read; no atomics, no allocation, no host
 * synchronisation.
 *
 * Every argument of psam_track_step means what it means there.  normals [V, 3] f32 (non-null, 4-byte aligned): one normal per voxel id, taken as
 * given -- not normalised, either sign; psam_scanmap_normals' output fits.
 *     pair, nearest     psam_track_step's, bit for bit: the same posed coordinate p, cell, cube, skip, min_count, r2 and order (q, v)
 *     used pair         psam_plane_step's: nn = (n_x n_x + n_y n_y) + n_z n_z in fp32 finite and > 0
 *     terms             psam_plane_step's with p the POSED coordinate's fp32 words (the query itself without a pose), s the pair's fp32 mean
 *                       (psam_map_cloud's bits) and n = normals[pair], all converted to fp64: d = p - s; r = (d_x n_x + d_y n_y) + d_z n_z;
 *                       c = p x n; J = (c, n)
 * sums [PSAM_PLANE_SUMS] f64 on the device: psam_plane_step's words in psam_plane_step's fixed order of addition (a function of M alone); [30] the
 *   paired queries whose pair is not used, [31] the participating queries that have a cell.  The same inputs give the same words from run to run.
 * ws: psam_scanmap_plane_workspace_bytes(M) = psam_plane_workspace_bytes(M) bytes (0 for M outside (0, 2^28]), 8-byte aligned.
 * Refusals: psam_track_step's codes in its order, before any launch, sums and nearest untouched; normals counts among the pointers that may not be
 * null (-1) and must be 4-byte aligned (-2). */
size_t psam_scanmap_plane_workspace_bytes(int32_t M);
int32_t psam_scanmap_plane_step(const void* map, size_t map_bytes, int32_t max_voxels, int32_t max_pairs, int32_t V, const float* normals,
                              const uint64_t* skip, int32_t min_count, int32_t reach, float r2, const float* qry, int32_t M, const uint64_t* qry_bits,
                              const float* pose, int32_t* nearest, double* sums, void* ws, size_t ws_bytes, psam_stream_t stream);

/* ---------------------------------------------------------------- scan map normals */

/* One surface normal and curvature per voxel of a scan map (ScanMap.normals), from the map's own block: the eigenvector of the smallest eigenvalue of
 * the scatter matrix of the MEANS of the voxels around it.  The map block is only read; there is no workspace, no atomics, no allocation and no host
 * synchronisation.
 *
 * map, map_bytes, max_voxels, max_pairs, V, skip, min_count: psam_track_step's.
 *     allowed voxel     u is allowed iff u < V, count(u) >= min_count and its bit in skip is clear (skip may be NULL)
 *     neighbourhood     of voxel id v < V: the allowed voxels in the (2 reach + 1)^3 cells around v's own cell (key_of_id[v]); a cell with a coordinate
 *                       below 0 or at or above 2^21 is skipped.  reach is 1 or 2: 27 or 125 cells.  If v itself is not allowed its neighbourhood is
 *                       empty: count 0, normal (0, 0, 0), curvature 0, scatter 0
 *     point of a voxel  its mean with the bits psam_map_cloud gives it (the s psam_track_step pairs with), in fixed point:
 *                       q_a = floor((double)s_a * 2^20) + 2^20, an integer in [0, 2^21]
 *     scatter           n the number of voxels of the neighbourhood, s = sum q, P = sum q q^T, S = n P - s s^T, all integers, exact: n <= 125 and
 *                       q <= 2^21 give P_ab < 2^49, n P_ab < 2^56, s_a s_b < 2^56, so S fits a signed 64-bit word.  S goes to fp64 once, rounded to
 *                       nearest even.  Neither the order of the cube nor the schedule enters any output
 *     normal            n < min_voxels (min_voxels >= 1): (0, 0, 0) and curvature 0, exactly.  Otherwise psam_normals_voxel's solve on S: scaled by a
 *                       power of two, cyclic Jacobi in fp64, the eigenvector of the smallest eigenvalue (ties: the lowest axis) normalised and
 *                       rounded to fp32, curvature l0 / (l0 + l1 + l2), and the sign without a viewpoint: the component of largest magnitude
 *                       (ties: the lowest axis) is positive, decided on the stored fp32 values
 * count [V] i32, normal [V, 3] f32, curvature [V] f32; scatter [V, 6] f64 (may be NULL): xx, xy, xz, yy, yz, zz of S.
 * Every refusal comes before any launch and leaves the outputs untouched: a null map, count, normal or curvature, V outside (0, max_voxels], bad
 * capacities, reach outside 1 .. 2, min_voxels < 1, min_count < 1: -1; a misaligned pointer (map 16 bytes; skip and scatter 8; count, normal and
 * curvature 4): -2; a short map block: -3. */
#define PSAM_SCANMAP_NORMALS_MAX_REACH 2
int32_t psam_scanmap_normals(const void* map, size_t map_bytes, int32_t max_voxels, int32_t max_pairs, int32_t V, const uint64_t* skip, int32_t min_count,
                         int32_t reach, int32_t min_voxels, int32_t* count, double* scatter, float* normal, float* curvature, psam_stream_t stream);

/* ---------------------------------------------------------------- scan map relocalisation */

/* The score of a global pose search against a scan map (ScanMap.track_score, ScanMap.relocalize): under each of P candidate poses, the number
 * of queries that land on the map -- all P poses from one call.  The map block is only read; the call allocates nothing and does not synchronise
 * with the host.
 *
 * map, map_bytes, max_voxels, max_pairs, V, skip, min_count, reach, r2, qry [M, 3]: psam_track_step's.  poses [P, 12] f32 in DEVICE memory, one
 * pose per row, row-major 3 x 4, scan frame -> map frame; 0 < P <= 2^20.  The entry cannot look at them: the host validates them before the upload.
 *     candidates        of query i under pose p: psam_track_step's, bit for bit -- the same posed coordinate, cell and acceptance test, the same
 *                       (2 reach + 1)^3 cells (a cell off the grid is skipped; no cell is dropped by a geometric bound), v < V,
 *                       count(v) >= min_count, the bit of v in skip clear, q = (dx dx + dy dy) + dz dz <= r2 in fp32 against the voxel's mean with
 *                       the bits psam_map_cloud gives it, NaN false
 *     counts [P] i32    counts[p] = the number of queries with at least one candidate under pose p
 *                       == (int)psam_track_step's sums[0] under pose p with the same r2, reach, skip and min_count and no qry_bits.
 *                       A query without a cell scores nothing; a pose that is not finite gives NaN coordinates, no cell and a count of 0
 * counts is cleared on the stream first and then raised by integer atomic additions (one per wave and pose, below 2^28 in all): the words are a
 * function of the inputs alone, the same from run to run.
 * ws: psam_relocalize_workspace_bytes(V) = 16 V bytes (0 for V outside (0, 2^28]), 16-byte aligned: one float4 per voxel id, its mean, or NaN for
 * a voxel that is no candidate by min_count or skip.  It is rebuilt by every call and means nothing afterwards.
 * Every refusal comes before any launch and leaves counts untouched: a null map, qry, poses, counts or ws, M outside (0, 2^28], V outside
 * (0, max_voxels], bad capacities, reach outside 1 .. 4, min_count < 1, r2 not finite and positive, P outside (0, 2^20]: -1; a misaligned pointer
 * (map and ws 16 bytes; skip 8; qry, poses and counts 4): -2; a short map block or ws: -3. */
#define PSAM_RELOCALIZE_POSES 4      /* poses per workgroup: a chunk of the grid (query tiles x pose chunks) */
size_t psam_relocalize_workspace_bytes(int32_t V);
int32_t psam_relocalize_score(const void* map, size_t map_bytes, int32_t max_voxels, int32_t max_pairs, int32_t V, const uint64_t* skip, int32_t min_count,
                              int32_t reach, float r2, const float* qry, int32_t M, const float* poses, int32_t P, int32_t* counts, void* ws,
                              size_t ws_bytes, psam_stream_t stream);

/* ---------------------------------------------------------------- scan map views */

/* The scan map as a camera inside it sees it (ScanMap.view): one ray per pixel, walked through the map's own voxel table in exact integers, ends on
 * the first voxel it meets.  The answer has the format of psam_view_splat's -- keys [height, width] u64, (bits(depth) << 32) | index, all ones where a
 * pixel is empty -- with the VOXEL ID as the index, so psam_view_pick, psam_view_paint_ids and psam_view_paint_rows take it as it is, with N = V.
 * Against point splats of psam_map_cloud it has no holes between voxels, nothing shows through a wall, and the voxels that every other reader leaves
 * out (skip, min_count: psam_track_step's) are seen through.  The map block is only read; the call allocates nothing, does not synchronise with the
 * host, and gives the same words from run to run: one thread owns one pixel and nothing is accumulated.
 *
 * map, map_bytes, max_voxels, max_pairs, V, skip, min_count: psam_track_step's.  inv_h: the value the map was cleared with (psam_map_clear); a
 * block whose header holds another one, and a dead map (flags != 0), give all pixels empty.  pose, fx, fy, cx, cy, width, height, znear: the camera of
 * psam_view_splat, its pose from the map's frame to the camera's.  eye: 3 floats in HOST memory, the camera's centre in the map's frame,
 * e = -R^T t, which the caller computes in fp64 from the twelve pose words and rounds to fp32 once.
 *     pairable voxel    v < V, count(v) >= min_count, the bit of v in skip clear (skip may be NULL)
 *     eye cell          o_a = floorf((e_a - (-1)) * inv_h) with -1 <= e_a <= 1 and o_a in [0, 2^21): a map point's cell and acceptance test
 *                       (psam_map_add's, colour apart).  An eye the map does not accept gives all pixels empty
 *     grid              the cells 0 .. cmax on every axis, cmax = min((int)floorf(2 * inv_h), 2^21 - 1): the largest cell a coordinate of 1 can have
 *     ray of (px, py)   fp32, every operation rounded on its own:
 *                         a = ((float)px + 0.5f - cx) / fx;  b = ((float)py + 0.5f - cy) / fy
 *                         d_k = (R[0][k] * a + R[1][k] * b) + R[2][k], k = 0, 1, 2        the camera's direction (a, b, 1) taken back by R^T
 *                         m = max_k |d_k|; the pixel is empty unless every d_k is finite and m > 0
 *                         N_k = (int)rintf((d_k / m) * 2097152.0f)                        the longest axis is exactly +-2^21
 *                       The ray is psam_carve_scan's ray between cell centres from o to the cell o + N, which lies outside the grid: the walk of
 *                       "scan map carving" with n_a = |N_a|, s_a = -1 where N_a < 0, tied axes stepping together; in its difference form
 *                       D_ab = (2 k_a + 1) n_b - (2 k_b + 1) n_a stays below 2^44 in magnitude because the walk ends inside the grid (below)
 *     end of the walk   the crossed cells are visited in order; o itself is not among them.  The walk ends at the first of
 *                         (i)  a cell with a coordinate outside 0 .. cmax: the pixel is empty.  The grid and the segment are convex, so a ray never
 *                              returns, and at most 3 (cmax + 1) cells are visited
 *                         (ii) a cell that holds a pairable voxel v whose mean s (psam_map_cloud's bits) has the depth
 *                              c = ((P[2][0] s_x + P[2][1] s_y) + P[2][2] s_z) + P[2][3] (psam_view_splat's) with c >= near and c < inf:
 *                              key = ((u64)bits(c) << 32) | v
 *                       A voxel that is not pairable, or whose mean lies in front of near, is passed through
 * Every ray starts at the centre of the eye's cell: the picture is that of a camera moved by at most half a voxel.
 * ws: psam_mapview_ws_bytes(inv_h) bytes (0 for an inv_h that is not finite and positive; at most 2.2 MB), 16-byte aligned: one bit per brick of
 * (2^s)^3 cells, s = 3 while that gives at most 257 bricks per axis (voxels down to 2^-10) and the least larger s beyond; set, by a launch over the V
 * voxel ids, where the brick holds a pairable voxel.  A cell whose brick bit is clear is stepped over without a look into the table: a lookup is
 * skipped, never a step.  The bitmap is rebuilt by every call and means nothing afterwards.
 * flags: 0, or for measurement PSAM_MAP_VIEW_NO_GATE (every cell is looked up; ws is not touched) and PSAM_MAP_VIEW_NO_LDS (the bitmap is read from
 * global memory even where it would fit the workgroup's shared memory).  No flag changes a word of keys.
 * stats: NULL, or 2 u64 words in DEVICE memory to which the call ADDS the cells its rays visited inside the grid and the table lookups they made.
 * Every refusal comes before any launch and leaves keys untouched: a null map, pose, eye, keys or ws, bad capacities, V outside (0, max_voxels] (an
 * empty map has no view), inv_h, fx, fy, near not finite and positive, cx, cy or a pose word not finite, width or height outside [1, 8192], an eye
 * outside [-1, 1]^3 or NaN, min_count < 1, unknown flags: -1; a misaligned pointer (map and ws 16 bytes; skip, keys and stats 8): -2; a short map
 * block or ws: -3. */
#define PSAM_MAP_VIEW_NO_GATE 1
#define PSAM_MAP_VIEW_NO_LDS 2
size_t psam_mapview_ws_bytes(float inv_h);
int32_t psam_mapview(const void* map, size_t map_bytes, int32_t max_voxels, int32_t max_pairs, int32_t V, float inv_h, const float* pose, float fx,
                      float fy, float cx, float cy, int32_t width, int32_t height, float znear, const float* eye, const uint64_t* skip,
                      int32_t min_count, int32_t flags, uint64_t* keys, uint64_t* stats, void* ws, size_t ws_bytes, psam_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* POINTSAM_HIP_H */
