"""Thin torch-tensor wrappers over the C ABI (include/pointsam_hip.h).

PyTorch is plumbing here: it owns device memory and the HIP stream; every computation is a kernel of
libpointsam_hip.so launched on ``torch.cuda.current_stream()``.  Inputs must be CUDA(HIP) fp32 / int64
tensors; there is no CPU path.
"""
import ctypes
import math
import torch

from . import _lib
from ._lib import check

ACT_NONE, ACT_GELU, ACT_RELU, ACT_SWIGLU = 0, 1, 2, 3

# Measurement hook (bench.py): when GEMM_PROFILE is a list, every GEMM_PROFILE_EVERY-th GEMM launch is bracketed by two
# HIP events on the launch stream and (start, end, flops, M, N, K) is appended.  Sampling keeps the perturbation of the
# timed region small (an event pair costs ~20 us of host time and the host issues ~400 launches per 14 ms step: bracketing every
# launch cost 17 %, every 7th still 7 %); bench.py samples every 3rd launch of the LAST step of the timed region only.
GEMM_PROFILE = None
GEMM_PROFILE_EVERY = 29
# Streams whose kernels must not overlap a sampled launch (BatchPipeline with several batches in flight): the sampled launch
# waits for what they have enqueued so far and they wait for its end, so the events bracket the kernel running ALONE.
GEMM_PROFILE_OTHERS = ()
GEMM_PROFILE_AFTER = 0     # launches (since the counter was reset) to skip before sampling starts
_gemm_counter = 0


def _sample_now():
    return GEMM_PROFILE is not None and _gemm_counter > GEMM_PROFILE_AFTER and _gemm_counter % GEMM_PROFILE_EVERY == 0


def _sampled_launch(launch, record):
    """Brackets one launch with HIP events on the launch stream (exclusive of GEMM_PROFILE_OTHERS) and records them."""
    cur = torch.cuda.current_stream()
    for o in GEMM_PROFILE_OTHERS:
        cur.wait_stream(o)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    launch()
    e.record()
    for o in GEMM_PROFILE_OTHERS:
        o.wait_event(e)
    record(s, e)


# GEMM arithmetic: "f32" = v_mfma_f32_32x32x2_f32 everywhere (exact fp32 products); "bf16x6" = large GEMMs on the bf16
# matrix pipe with the exact 3-way operand split (fp32-accurate, see csrc/gemm_split.hip), small ones stay on "f32".
# The mode is a CONTEXT variable (per thread / per asyncio task), entered by every model method for its own precision: two models of different
# precision -- or a threaded server -- do not see each other's setting.  `ops.GEMM_MODE` still reads the current value (module __getattr__).
import contextvars
_GEMM_MODE_VAR = contextvars.ContextVar("point_sam_amd_gemm_mode", default="f32")


def current_gemm_mode() -> str:
    return _GEMM_MODE_VAR.get()


def __getattr__(name):
    if name == "GEMM_MODE":
        return _GEMM_MODE_VAR.get()
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


class _OpsModule(__import__("types").ModuleType):
    """`ops.GEMM_MODE = ...` (the pre-round-4 interface) would create a real module attribute that shadows __getattr__ for good: every later read of
    ops.GEMM_MODE would then return that stale value while the launches follow the context variable.  Assignment is refused; use `with ops.gemm_mode(m):`."""

    def __setattr__(self, name, value):
        if name == "GEMM_MODE":
            raise AttributeError("ops.GEMM_MODE is read-only (it reflects a context variable): use `with ops.gemm_mode(mode):`")
        super().__setattr__(name, value)


import sys as _sys
_sys.modules[__name__].__class__ = _OpsModule


# Key split of the fp16-pipe attention for single-cloud shapes (csrc/attention.hip, psam_attention_f16x3_ex2): 4 = up to four workgroups per
# (query block, head), combined in the kernel -- the latency of ONE stream of work; 1 = off, what the multi-stream pipelines use (their other streams
# fill the idle CUs and the split's extra work costs throughput: 133 -> 129 sessions/s at cfg #5, while the encoder latency drops 8.7 -> 8.1 ms).
_ATTN_KEYSPLIT_VAR = contextvars.ContextVar("point_sam_amd_attn_keysplit", default=4)


def current_attention_keysplit() -> int:
    return _ATTN_KEYSPLIT_VAR.get()


class attention_keysplit:
    """Context manager: cap of the attention's key split for the enclosed launches (1 = never split)."""

    def __init__(self, n: int):
        self.n = max(1, int(n))

    def __enter__(self):
        self.token = _ATTN_KEYSPLIT_VAR.set(self.n)

    def __exit__(self, *exc):
        _ATTN_KEYSPLIT_VAR.reset(self.token)


# Arrival-counter blocks (include/pointsam_hip.h, PSAM_COUNTER_BYTES): kernels with an in-kernel fix-up (split-K GEMM, key-split attention, skinny Linear +
# LayerNorm) count their workgroups in through device memory the CALLER owns -- the library allocates nothing and keeps no per-stream state (round 6).
# This host keeps one zeroed block per (device, stream) for eager launches (launches on one stream are ordered, so they may share it) and lets a scope
# bring its own: every GraphPipeline slot captures its graphs on a block of its own (`use_counters`), so any two graphs may be in flight together and a
# graph may replay on any stream.  A capture outside such a scope on a stream that never launched eagerly gets a fresh block inside the capture
# (zeroed by a node of that graph on every replay).
COUNTER_BYTES = 65536
_COUNTERS = {}
_COUNTERS_VAR = contextvars.ContextVar("point_sam_amd_counters", default=None)


def new_counters(device) -> torch.Tensor:
    return torch.zeros(COUNTER_BYTES // 4, dtype=torch.int32, device=device)


def arrival_counters(device) -> torch.Tensor:
    """The arrival-counter block of the enclosing `use_counters` scope, else the current stream's."""
    t = _COUNTERS_VAR.get()
    if t is not None:
        if t.device != torch.device(device) and not (t.device.type == "cuda" and torch.device(device).index is None):
            raise _lib.PointSamHipError(f"use_counters: the block lives on {t.device}, the launch is on {device}")
        return t
    dev = torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(dev).cuda_stream)
    t = _COUNTERS.get(key)
    if t is None:
        t = new_counters(dev)
        if not torch.cuda.is_current_stream_capturing():
            _COUNTERS[key] = t
    return t


class use_counters:
    """Context manager: the enclosed launches count in through `block` (a new_counters() tensor) instead of the current stream's block."""

    def __init__(self, block: torch.Tensor):
        if block.dtype != torch.int32 or block.numel() * 4 < COUNTER_BYTES or not block.is_cuda or not block.is_contiguous():
            raise ValueError("use_counters: need a contiguous int32 device tensor of COUNTER_BYTES bytes (ops.new_counters)")
        self.block = block

    def __enter__(self):
        self.token = _COUNTERS_VAR.set(self.block)
        return self.block

    def __exit__(self, *exc):
        _COUNTERS_VAR.reset(self.token)


SPLIT_MIN_M, SPLIT_MIN_N, SPLIT_MIN_K = 256, 128, 128
SKINNY_MAX_M = 64      # up to this many rows nn.Linear runs on the skinny kernel (exact fp32 products, like "f32")
GEMM_MODES = ("f32", "bf16x6", "f16x3")
# "f16x3" = large 2-D GEMMs against a prepared static weight (F16Weight) on the fp16 matrix pipe: power-of-two row scales + 2-way
# fp16 split, 3 partial products (fp32-grade: same measured error vs fp64 as the f32 kernel, csrc/gemm_f16x3p.hip); batched and
# small ones stay on "f32".


class gemm_mode:
    """Context manager selecting the GEMM arithmetic for the enclosed launches."""

    def __init__(self, mode):
        if mode not in GEMM_MODES:
            raise ValueError(f"unknown GEMM mode {mode!r}; expected one of {GEMM_MODES}")
        self.mode = mode

    def __enter__(self):
        self.token = _GEMM_MODE_VAR.set(self.mode)

    def __exit__(self, *exc):
        _GEMM_MODE_VAR.reset(self.token)


def _gemm_call(fn_args, flops, M, N, K, what):
    global _gemm_counter
    L = _lib.load()
    split = current_gemm_mode() == "bf16x6" and M >= SPLIT_MIN_M and N >= SPLIT_MIN_N and K >= SPLIT_MIN_K
    fn = L.psam_gemm_bf16x6 if split else L.psam_gemm_f32
    _gemm_counter += 1
    if not _sample_now():
        check(fn(*fn_args), what)
        return
    _sampled_launch(lambda: check(fn(*fn_args), what), lambda s, e: GEMM_PROFILE.append((s, e, flops, M, N, K, "bf16x6" if split else "f32")))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


def _chk(t, dtype=torch.float32, name="tensor"):
    if not t.is_cuda:
        raise _lib.PointSamHipError(f"{name} must live on the GPU: the HIP path has no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


# ------------------------------------------------------------------------------------------ tokenizer
def fps(xyz: torch.Tensor, num_samples: int):
    """[B,N,3] -> (fps_idx [B,G] int64, centers [B,G,3]).  common.py:91-92."""
    _chk(xyz, name="xyz")
    B, N, _ = xyz.shape
    L = _lib.load()
    nbytes = L.psam_fps_workspace_bytes(B, N, num_samples)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=xyz.device)
    idx = torch.empty(B, num_samples, dtype=torch.int64, device=xyz.device)
    centers = torch.empty(B, num_samples, 3, dtype=torch.float32, device=xyz.device)
    check(L.psam_fps(xyz.data_ptr(), B, N, num_samples, idx.data_ptr(), centers.data_ptr(), ws.data_ptr(), nbytes, _stream()), "psam_fps")
    return idx, centers


def knn(centers: torch.Tensor, xyz: torch.Tensor, k: int) -> torch.Tensor:
    """[B,G,3], [B,N,3] -> knn_idx [B,G,K] int64 ascending by (d2, index).  common.py:27-56,97."""
    _chk(centers, name="centers"); _chk(xyz, name="xyz")
    B, G, _ = centers.shape
    N = xyz.shape[1]
    out = torch.empty(B, G, k, dtype=torch.int64, device=xyz.device)
    check(_lib.load().psam_knn(centers.data_ptr(), xyz.data_ptr(), B, G, N, k, out.data_ptr(), _stream()), "psam_knn")
    return out


def three_nn(xyz: torch.Tensor, centers: torch.Tensor, eps: float = 1e-8):
    """-> (idx3 [B,N,3] int64, w3 [B,N,3]).  common.py:238-255."""
    _chk(xyz, name="xyz"); _chk(centers, name="centers")
    B, N, _ = xyz.shape
    G = centers.shape[1]
    idx = torch.empty(B, N, 3, dtype=torch.int64, device=xyz.device)
    w = torch.empty(B, N, 3, dtype=torch.float32, device=xyz.device)
    check(_lib.load().psam_three_nn(xyz.data_ptr(), centers.data_ptr(), B, N, G, eps, idx.data_ptr(), w.data_ptr(), _stream()), "psam_three_nn")
    return idx, w


def group_gather(xyz, feats, centers, knn_idx, radius=None, width=None):
    """feats [B*rep,N,C] -> [B*rep,G,K,3+C].  common.py:99-120 / 126-187.  width (>= 3 + C): rows zero-padded to that many columns."""
    _chk(xyz); _chk(feats); _chk(centers); _chk(knn_idx, torch.int64)
    B, N, _ = xyz.shape
    rep = feats.shape[0] // B
    G, K = knn_idx.shape[1:]
    C = feats.shape[-1]
    width = width or 3 + C
    out = torch.empty(B * rep, G, K, width, dtype=torch.float32, device=xyz.device)
    check(_lib.load().psam_group_gather_ld(xyz.data_ptr(), feats.data_ptr(), centers.data_ptr(), knn_idx.data_ptr(), B, rep, N, G, K, C,
                                           float(radius or 0.0), out.data_ptr(), width, _stream()), "psam_group_gather")
    return out


def patch_l1(xyz, feats, centers, knn_idx, W, bias, lnw, lnb, eps, out=None, radius=None, center_idx=None, scale_out=None):
    """Fused gather + Linear(Cin,128) + LayerNorm + GELU -> [B*rep*G*K, 128].  common.py:486-489.
    center_idx [B,G] (FPS indices): centralize_features (Cin = 3 + 2C, common.py:116-118); scale_out [rows]: the rows leave g8-packed
    for the f16x3 GEMM (linear(..., x_scale=scale_out, x_packed=True))."""
    _chk(xyz); _chk(feats); _chk(centers); _chk(knn_idx, torch.int64); _chk(W)
    B, N, _ = xyz.shape
    rep = feats.shape[0] // B
    G, K = knn_idx.shape[1:]
    C = feats.shape[-1]
    cin = 3 + C * (2 if center_idx is not None else 1)
    assert W.shape == (128, cin), (W.shape, cin)
    if center_idx is not None:
        _chk(center_idx, torch.int64, "center_idx")
    rows = B * rep * G * K
    if out is None:
        out = torch.empty(rows, 128, dtype=torch.float32, device=xyz.device)
    check(_lib.load().psam_patch_l1_ex(xyz.data_ptr(), feats.data_ptr(), centers.data_ptr(), knn_idx.data_ptr(), _p(center_idx), W.data_ptr(),
                                       bias.data_ptr(), lnw.data_ptr(), lnb.data_ptr(), eps, B, rep, N, G, K, C, float(radius or 0.0), out.data_ptr(),
                                       _p(scale_out), _stream()), "psam_patch_l1")
    return out


def nn_group_feats(xyz, centers, nn_idx, feats=None, logits=None, width=8):
    """Voronoi variant: per-point rows relative to the nearest centre, zero-padded to `width` columns (csrc/rowops.hip nn_group_feats_kernel).
    feats [B,N,C]: NNGrouper.forward (common.py:203-211) -> [B*N, width]; logits [Z,N]: MaskEncoderNN's input (prompt_encoder.py:281-287) -> [Z*N, width]."""
    _chk(xyz); _chk(centers); _chk(nn_idx, torch.int64)
    B, N, _ = xyz.shape
    G = centers.shape[1]
    if logits is None:
        _chk(feats)
        C, rep, mode = feats.shape[-1], 1, 0
    else:
        _chk(logits)
        C, rep, mode = 0, logits.shape[0] // B, 1
    assert width % 4 == 0 and width >= (4 + C if mode == 0 else 5)
    out = torch.empty(B * rep * N, width, dtype=torch.float32, device=xyz.device)
    check(_lib.load().psam_nn_group_feats(xyz.data_ptr(), centers.data_ptr(), nn_idx.data_ptr(), _p(feats), _p(logits), B, rep, N, G, C, mode, out.data_ptr(),
                                          width, _stream()), "psam_nn_group_feats")
    return out


def scatter_amax(x, idx, out_rows, rows_per_set, set_stride, idx_rep=1, include_self=False):
    """Max-pool of the rows of x [R, C] into out [out_rows, C]: row r goes to idx[(r // rows_per_set // idx_rep), r % rows_per_set] + (r //
    rows_per_set) * set_stride (torch scatter_reduce 'amax'; see include/pointsam_hip.h psam_scatter_amax)."""
    xp, ldx = _row_view(x, "x"); _chk(idx, torch.int64)
    R, C = x.shape
    out = torch.empty(out_rows, C, dtype=torch.float32, device=x.device)
    check(_lib.load().psam_scatter_amax(xp, ldx, idx.data_ptr(), R, C, rows_per_set, set_stride, idx_rep, out.data_ptr(), out_rows, int(bool(include_self)),
                                        _stream()), "psam_scatter_amax")
    return out


def group_max(x: torch.Tensor, K: int, out=None):
    """[groups*K, C] -> [groups, C]."""
    _chk(x)
    rows, C = x.shape
    groups = rows // K
    if out is None:
        out = torch.empty(groups, C, dtype=torch.float32, device=x.device)
    check(_lib.load().psam_group_max(x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), groups, K, C, _stream()), "psam_group_max")
    return out


# ------------------------------------------------------------------------------------------ dense
def _row_view(t, name):
    """2-D fp32 view with unit inner stride -> (ptr, ld)."""
    if t.dtype != torch.float32 or not t.is_cuda or t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name}: need a 2-D CUDA fp32 tensor with unit inner stride, got {t.dtype} {tuple(t.shape)} {t.stride()}")
    return t.data_ptr(), t.stride(0)


def row_scale_f16(x, K=None, out=None):
    """Per-row power-of-two scales for the f16x3 GEMM (row maximum of x[:, :K] into [2^14, 2^15))."""
    xp, ldx = _row_view(x, "x")
    rows = x.shape[0]
    if out is None:
        out = torch.empty(rows, dtype=torch.float32, device=x.device)
    check(_lib.load().psam_row_scale_f16(xp, ldx, rows, x.shape[1] if K is None else K, out.data_ptr(), _stream()), "psam_row_scale_f16")
    return out


def _kpad(K: int) -> int:
    return (K + 31) // 32 * 32


def pack_rows_g8(x, scale, K=None, out=None):
    """g8-packed form of the row-scaled x[:, :K] (csrc/gemm_f16x3p.hip): per 8 consecutive k [hi x8 | lo x8] fp16 in the 32-bit
    containers; K is zero-padded to the next multiple of 32 (the GEMM's slab)."""
    xp, ldx = _row_view(x, "x")
    rows = x.shape[0]
    K = x.shape[1] if K is None else K
    if out is None:
        out = torch.empty(rows, _kpad(K), dtype=torch.float32, device=x.device)
    op, ldo = _row_view(out, "out")
    check(_lib.load().psam_pack_rows_f16x2_g8(xp, ldx, scale.data_ptr(), rows, K, op, ldo, _stream()), "psam_pack_rows_f16x2_g8")
    return out


def scale_pack_rows_g8(x, K=None, out=None, scale=None):
    """(packed, scale): row scales and the g8-packed form of fp32 rows in ONE pass (K <= 6144, K % 4 == 0)."""
    xp, ldx = _row_view(x, "x")
    rows = x.shape[0]
    K = x.shape[1] if K is None else K
    if out is None:
        out = torch.empty(rows, _kpad(K), dtype=torch.float32, device=x.device)
    if scale is None:
        scale = torch.empty(rows, dtype=torch.float32, device=x.device)
    op, ldo = _row_view(out, "out")
    check(_lib.load().psam_scale_pack_rows_g8(xp, ldx, rows, K, op, ldo, scale.data_ptr(), _stream()), "psam_scale_pack_rows_g8")
    return out, scale


class F16Weight:
    """A static nn.Linear weight [N, K] prepared ONCE for the "f16x3" GEMM (csrc/gemm_f16x3p.hip): per-row power-of-two scales and the
    g8-packed, K-padded (multiple of 32) hi|lo fp16 form.  Owned by the model that built it (no process-global cache); the fp32
    original stays available for launches below the split thresholds."""

    def __init__(self, W: torch.Tensor):
        _row_view(W, "W")
        self.fp32 = W
        self.N, self.K = W.shape
        self.Kp = _kpad(self.K)
        self._scale = self._packed = None      # packed on first use: weights that only ever run through a coarse C-ABI stage (psam_eva_block & co. hold
                                                # their own packed blob) never get this second copy

    def _materialise(self):
        if torch.cuda.is_current_stream_capturing():
            raise _lib.PointSamHipError("F16Weight: first use inside a graph capture (run one eager pass first, as GraphPipeline does)")
        self._scale = row_scale_f16(self.fp32)
        self._packed = pack_rows_g8(self.fp32, self._scale)
        assert self._packed.shape[1] == self.Kp
        torch.cuda.current_stream(self.fp32.device).synchronize()      # other streams may use it right after (the pipelines run several)

    @property
    def scale(self):
        if self._scale is None:
            self._materialise()
        return self._scale

    @property
    def packed(self):
        if self._packed is None:
            self._materialise()
        return self._packed

    @staticmethod
    def eligible(N: int, K: int) -> bool:
        return N >= SPLIT_MIN_N and K >= SPLIT_MIN_K

    @property
    def shape(self):
        return (self.N, self.K)


def _f16x3p_call(fn_args, flops, M, N, K, fuse=None):
    global _gemm_counter
    import ctypes
    L = _lib.load()
    _gemm_counter += 1
    fn_args = fn_args[:-1] + (ctypes.byref(fuse) if fuse is not None else None, fn_args[-1])
    if not _sample_now():
        check(L.psam_gemm_f16x3p_ex(*fn_args), "psam_gemm_f16x3p")
        return
    _sampled_launch(lambda: check(L.psam_gemm_f16x3p_ex(*fn_args), "psam_gemm_f16x3p"), lambda s, e: GEMM_PROFILE.append((s, e, flops, M, N, K, "f16x3")))


_SPLITK = {}


def splitk_factor(M: int, N: int, K: int, act: int) -> int:
    """Split-K factor the library suggests for a packed-operand GEMM shape (1: none); a pure function of the shape and the device."""
    key = (M, N, K, act, torch.cuda.current_device())
    ks = _SPLITK.get(key)
    if ks is None:
        ks = _SPLITK[key] = int(_lib.load().psam_gemm_f16x3p_splitk(M, N, K, act))
    return ks


def fuse_supported(M: int, N: int) -> bool:
    """Shapes for which the fused GEMM extras (packed output, LayerNorm partials, folded LayerNorm) exist."""
    return M % 256 == 0 and N % 128 == 0


def row_ln_bound(gamma, beta) -> float:
    """Bound on |LayerNorm(x) * gamma + beta| over a row of len(gamma) columns: a normalised element is at most sqrt(n - 1).
    (GELU / ReLU after it only shrink magnitudes.)  The k2 of a packed output behind a row-LayerNorm epilogue."""
    n = gamma.numel()
    return float((n - 1) ** 0.5 * gamma.abs().max().item() + beta.abs().max().item())


def fused_row_ln(N: int) -> bool:
    """Whether linear(..., row_ln=...) exists for N output columns (psam_gemm_f16x3p_fused_row_ln): 256 always, 512 with the register epilogue."""
    return bool(_lib.load().psam_gemm_f16x3p_fused_row_ln(int(N)))


def linear128_ln_gelu_supported(rows: int, K: int, N: int, rowgroup: int) -> bool:
    """Shapes of linear128_ln_gelu_pack (csrc/patch_rowln.hip): 128 -> 512 columns on whole 64-row blocks, one bias row per 32-row tile."""
    return K == 128 and N == 512 and rows > 0 and rows % 64 == 0 and rowgroup > 0 and rowgroup % 32 == 0


def linear128_ln_gelu_pack(x, x_scale, fw, rowbias, rowgroup, gamma, beta, eps, bound, out, scale_out):
    """out = g8(GELU(LayerNorm(x @ fw^T + rowbias[row // rowgroup]) * gamma + beta)), scale_out[row] = the power-of-two scale of `bound`
    (>= 1.001 * row_ln_bound(gamma, beta)): PatchEncoder's per-row half of conv2.0, conv2.1 and its GELU in one kernel
    (psam_linear128_ln_gelu_pack).  x [rows, 128] g8-packed with x_scale, fw an F16Weight [512, 128], out [rows, 512] containers."""
    xp, ldx = _row_view(x, "x")
    rbp, ldrb = _row_view(rowbias, "rowbias")
    op, ldo = _row_view(out, "out")
    check(_lib.load().psam_linear128_ln_gelu_pack(xp, ldx, x_scale.data_ptr(), fw.packed.data_ptr(), fw.packed.stride(0), fw.scale.data_ptr(), rbp, ldrb, int(rowgroup),
                                                  gamma.data_ptr(), beta.data_ptr(), float(eps), float(bound), x.shape[0], fw.N, op, ldo,
                                                  scale_out.data_ptr(), _stream()), "psam_linear128_ln_gelu_pack")
    return out


def stat_segs(N: int) -> int:
    return (N // 2 + 31) // 32


def ln_stats_finalize(stats, cols, eps):
    """[M, segs, 2] per-segment (mean, centred sum of squares) -> (mean [M], rstd [M]) of a LayerNorm over `cols` columns."""
    M, segs, _ = stats.shape
    mean = torch.empty(M, dtype=torch.float32, device=stats.device)
    rstd = torch.empty(M, dtype=torch.float32, device=stats.device)
    check(_lib.load().psam_ln_stats_finalize(stats.data_ptr(), M, segs, cols, eps, mean.data_ptr(), rstd.data_ptr(), _stream()), "psam_ln_stats_finalize")
    return mean, rstd


def linear(x, W, bias=None, act=ACT_NONE, residual=None, out=None, rowbias=None, rowgroup=0, K=None, x_scale=None, x_packed=False,
           pack_out=None, stats=None, ln_fold=None, group_max_out=None, group_max_k=0, no_store=False, row_ln=None, hyper=None):
    """y = act(x @ W[:, :K]^T + bias + rowbias[row // rowgroup]) + residual.  x [M,>=K], W [N,>=K] row views, or W an F16Weight
    (prepared static weight).
    "f16x3" mode with an F16Weight and M above the threshold runs the packed-operand GEMM (csrc/gemm_f16x3p.hip): x is either already
    g8-packed by its producer (x_packed=True with x_scale: LayerNorm / scale_pack_rows_g8 output, [M, >= K padded to 32]) or is
    scaled and packed here in one extra pass.  Fused extras of that GEMM (fuse_supported shapes; include/pointsam_hip.h psam_gemm_fuse_t):
    pack_out=(scale_out [M], k1, k2) or (scale_out [M], bound [M]): `out` receives g8-packed rows + their bound-derived scales; stats=(buf [M, stat_segs(N), 2], cols):
    LayerNorm partials of the SwiGLU-gated rows; ln_fold=(mean [M], rstd [M], c [N]): LayerNorm of x folded into the GEMM;
    group_max_out [M / group_max_k, N] (group_max_k 32 | 64): per-column max over consecutive row groups of the output, no_store: the
    [M, N] output itself is not written (out may then be None).  N == 256 only: row_ln=(gamma, beta, eps): LayerNorm of every output
    row before the activation (with pack_out pass k1 = 0, k2 = row_ln_bound(gamma, beta));
    hyper=(hyper [Z, C, 256], masks [Z, C, rows_per_z], rows_per_z): masks[z, c, n] = <hyper[z, c], out[z * rows_per_z + n]>."""
    fw = None
    if isinstance(W, F16Weight):
        fw, W = W, W.fp32
    xp, ldx = _row_view(x, "x")
    wp, ldw = _row_view(W, "W")
    M = x.shape[0]
    N = W.shape[0]
    if K is None:
        K = W.shape[1]
        assert x_packed or x.shape[1] == K, (x.shape, W.shape)
    elif fw is not None and K != fw.K:
        fw = None
    fused = pack_out is not None or stats is not None or ln_fold is not None or group_max_out is not None or row_ln is not None or hyper is not None
    if no_store and (group_max_out is not None or hyper is not None) and out is None:
        op, ldo = (group_max_out if group_max_out is not None else hyper[1]).data_ptr(), N       # never dereferenced
    else:
        if out is None:
            out = torch.empty(M, N // 2 if act == ACT_SWIGLU else N, dtype=torch.float32, device=x.device)
        op, ldo = _row_view(out, "out")
    rp, ldr = (0, 0) if residual is None else _row_view(residual, "residual")
    rbp, ldrb = (0, 0) if rowbias is None else _row_view(rowbias, "rowbias")
    if current_gemm_mode() == "f16x3" and fw is not None and M >= SPLIT_MIN_M:
        if x_packed:
            if x_scale is None or x.shape[1] < fw.Kp or (ldx & 7) or (xp & 31):
                raise ValueError("x_packed needs x_scale and g8-packed rows padded to a multiple of 32 columns, 32-byte aligned")
            xa, sa = x, x_scale
        else:
            xa, sa = scale_pack_rows_g8(x, K)
        fuse = None
        hyper_parts = None
        if not fused and rowbias is None and act != ACT_SWIGLU and N % 4 == 0 and ldo % 4 == 0 and ldr % 4 == 0:
            ks = splitk_factor(M, N, fw.Kp, act)
            if ks > 1:      # few tiles, long K: partial planes + a fixed-order reduction (psam_gemm_fuse_t.splitk)
                ws = torch.empty(ks, M * N, dtype=torch.float32, device=x.device)
                fuse = _lib.GemmFuse()
                fuse.splitk_ws, fuse.splitk_plane, fuse.splitk = ws.data_ptr(), M * N, ks
                fuse.counters = arrival_counters(x.device).data_ptr()      # in-kernel fix-up instead of a reduction launch
        if fused:
            fuse = _lib.GemmFuse()
            fuse.no_store = int(bool(no_store))
            if group_max_out is not None:
                fuse.gmax_out, fuse.gmax_ld, fuse.gmax_k = group_max_out.data_ptr(), group_max_out.stride(0), int(group_max_k)
            if row_ln is not None:
                fuse.row_ln_g, fuse.row_ln_b, fuse.row_ln_eps = row_ln[0].data_ptr(), row_ln[1].data_ptr(), float(row_ln[2])
            if hyper is not None:
                hy, mk, rpz = hyper
                if not (hy.is_contiguous() and mk.is_contiguous() and hy.shape[-1] == N and mk.shape[:2] == hy.shape[:2] and mk.shape[2] == rpz):
                    raise ValueError("hyper [Z, C, N] / masks [Z, C, rows_per_z] must be contiguous and consistent")
                fuse.hyper, fuse.masks, fuse.hyper_c, fuse.hyper_rows = hy.data_ptr(), mk.data_ptr(), int(hy.shape[1]), int(rpz)
                planes = _lib.load().psam_gemm_f16x3p_hyper_planes(N, int(row_ln is not None))
                if planes > 1:      # partial products per 64-column wave tile: N / 64 planes, added below in a fixed order
                    hyper_parts = torch.empty(planes, mk.numel(), dtype=torch.float32, device=mk.device)
                    fuse.masks, fuse.hyper_pstride = hyper_parts.data_ptr(), mk.numel()
            if pack_out is not None and len(pack_out) == 2:      # (scale_out, per-row bound of the output): see psam_gemm_fuse_t.out_bound
                fuse.out_scale, fuse.out_bound, fuse.pack_out = pack_out[0].data_ptr(), pack_out[1].data_ptr(), 1
            elif pack_out is not None:
                fuse.out_scale, fuse.out_k1, fuse.out_k2, fuse.pack_out = pack_out[0].data_ptr(), float(pack_out[1]), float(pack_out[2]), 1
            if stats is not None:
                fuse.stats, fuse.stat_cols = stats[0].data_ptr(), int(stats[1])
            if ln_fold is not None:
                fuse.ln_mean, fuse.ln_rstd, fuse.ln_c = ln_fold[0].data_ptr(), ln_fold[1].data_ptr(), ln_fold[2].data_ptr()
        _f16x3p_call((xa.data_ptr(), xa.stride(0), sa.data_ptr(), fw.packed.data_ptr(), fw.packed.stride(0), fw.scale.data_ptr(), op, ldo, _p(bias),
                      rp, ldr, rbp, ldrb, rowgroup, M, N, fw.Kp, 1.0, act, _stream()), 2.0 * M * N * K, M, N, K, fuse)
        if hyper_parts is not None:
            check(_lib.load().psam_sum_planes(hyper_parts.data_ptr(), hyper_parts.shape[0], hyper_parts.shape[1], hyper_parts.shape[1],
                                              hyper[1].data_ptr(), _stream()), "psam_sum_planes")
        return out
    if fused:
        raise ValueError("fused GEMM extras exist only on the f16x3 packed-operand path")
    if x_packed:
        raise ValueError("x_packed activations can only feed an f16x3 GEMM with a prepared F16Weight (M above the split threshold)")
    if (M <= SKINNY_MAX_M and K % 16 == 0 and rowbias is None and act in (ACT_NONE, ACT_GELU, ACT_RELU) and (ldx | ldw) % 4 == 0
            and (xp | wp) % 16 == 0):
        # a handful of rows (the decoder's output tokens): N / 16 workgroups, whole-K load rounds (csrc/gemm.hip linear_skinny_kernel)
        check(_lib.load().psam_linear_skinny(xp, ldx, wp, ldw, _p(bias), rp, ldr, op, ldo, M, N, K, act, _stream()), "psam_linear_skinny")
        return out
    _gemm_call((xp, ldx, 0, 0, wp, ldw, 0, 0, op, ldo, 0, 0, _p(bias), rp, ldr, 0, 0, rbp, ldrb, rowgroup, M, N, K, 1, 1, 1.0, act, _stream()),
               2.0 * M * N * K, M, N, K, "psam_gemm_f32")
    return out


def gemm_batched(A, W, out, M, N, K, lda, ldw, ldc, sA, sW, sC, batch, alpha=1.0):
    """out[z] = alpha * A[z] @ W[z]^T (raw strided-batched form; tensors give base pointers only)."""
    _gemm_call((A.data_ptr(), lda, sA, 0, W.data_ptr(), ldw, sW, 0, out.data_ptr(), ldc, sC, 0, 0, 0, 0, 0, 0, 0, 0, 0, M, N, K, batch, 1, alpha,
                ACT_NONE, _stream()), 2.0 * M * N * K * batch, M, N, K, "psam_gemm_f32(batched)")
    return out


def layernorm_can_pack(cols: int) -> bool:
    return 256 <= cols <= 4096


def packed_cols(cols: int) -> int:
    """Columns of the buffer that receives a g8-packed row of `cols` values (zero-padded to the GEMM's 32-k slab)."""
    return _kpad(cols)


def layernorm(x, w, b, eps, act=ACT_NONE, residual=None, out=None, scale_out=None, pack=False, bound_out=None):
    """y = act(LN(x + residual)) over the last dim of a 2-D row view.  scale_out ([rows] fp32, optional) receives the f16x3
    row scales of y (what row_scale_f16(y) would compute), for the GEMM that consumes y.  pack=True: out receives the g8-packed
    form of the scaled rows instead of fp32 (linear(..., x_scale=scale_out, x_packed=True)); out needs packed_cols(cols) columns
    of room per row for the zero padding (or exactly cols when cols % 8 == 0 and the padding already holds zeros).
    bound_out=(buf [rows], c2, c1, c0) (with pack): buf[r] = c2 t^2 + c1 t + c0, t = ||y[r]||_2 -- the per-row output bound of the GEMM that
    consumes y (linear(..., pack_out=(scale_out, buf)))."""
    xp, ldx = _row_view(x, "x")
    rows, cols = x.shape
    if out is None:
        out = torch.empty(rows, _kpad(cols) if pack else cols, dtype=torch.float32, device=x.device)
    op, ldo = _row_view(out, "out")
    rp, ldr = (0, 0) if residual is None else _row_view(residual, "residual")
    if bound_out is not None:
        bb, c2, c1, c0 = bound_out
        check(_lib.load().psam_layernorm_ex2(xp, ldx, rp, ldr, w.data_ptr(), b.data_ptr(), op, ldo, rows, cols, eps, act, _p(scale_out), 1 if pack else 0,
                                             bb.data_ptr(), float(c2), float(c1), float(c0), _stream()), "psam_layernorm")
        return out
    check(_lib.load().psam_layernorm_ex(xp, ldx, rp, ldr, w.data_ptr(), b.data_ptr(), op, ldo, rows, cols, eps, act, _p(scale_out), 1 if pack else 0,
                                        _stream()), "psam_layernorm")
    return out


def swiglu_ln(gx, xoff, H, w, b, eps, out):
    gp, ldg = _row_view(gx, "gx")
    op, ldo = _row_view(out, "out")
    check(_lib.load().psam_swiglu_ln(gp, ldg, xoff, w.data_ptr(), b.data_ptr(), op, ldo, gx.shape[0], H, eps, _stream()), "psam_swiglu_ln")
    return out


def _f16x3_head_dim(hd: int) -> bool:
    """Head dims of psam_attention_f16x3: 64, or a multiple of 8 in (64, 128] (zero-padded to 128 inside the kernel: the giant encoder's 88)."""
    return hd == 64 or (64 < hd <= 128 and hd % 8 == 0)


def attention_can_pack(hd: int) -> bool:
    return current_gemm_mode() == "f16x3" and _f16x3_head_dim(hd)


def attention(q, k, v, out, B, H, Lq, Lk, hd, scale, pack=None):
    """q/k/v/out: 2-D row views [B*L, >=H*hd] (may be column slices of a fused qkv buffer).
    pack=(a_scale [B*Lk], k1, k2, o_scale [B*Lq]) ("f16x3", hd 64 / 128, self-attention): out receives the g8-packed rows for the output
    projection and o_scale their (bound-derived, per-cloud) scales -- linear(out, W, x_scale=o_scale, x_packed=True)."""
    qp, ldq = _row_view(q, "q"); kp, ldk = _row_view(k, "k"); vp, ldv = _row_view(v, "v"); op, ldo = _row_view(out, "out")
    L = _lib.load()
    args = (qp, ldq, Lq * ldq, kp, ldk, Lk * ldk, vp, ldv, Lk * ldv, op, ldo, Lq * ldo, B, H, Lq, Lk, hd, scale)
    if pack is not None and not attention_can_pack(hd):
        raise ValueError("packed attention output needs the f16x3 kernel (head dim 64, or a multiple of 8 in (64, 128])")
    if pack is not None or (current_gemm_mode() == "f16x3" and _f16x3_head_dim(hd)):
        a_scale, k1, k2, o_scale = pack if pack is not None else (None, 0.0, 0.0, None)
        ks = current_attention_keysplit()
        nb = int(L.psam_attention_f16x3_keysplit_ws_bytes(B, H, Lq, Lk, hd, ks)) if ks > 1 else 0
        ks_ws = torch.empty(nb, dtype=torch.uint8, device=out.device) if nb else None      # single-cloud shape: key split with in-kernel combine (scratch and
        check(L.psam_attention_f16x3_ex2(*args, _p(a_scale), float(k1), float(k2), _p(o_scale), ks if nb else 1, _p(ks_ws), nb,      # counter block are the caller's)
                                         arrival_counters(out.device).data_ptr() if nb else None, _stream()), "psam_attention")
        return out
    check(L.psam_attention_f32(*args, _stream()), "psam_attention")
    return out


def attention_packed_supported(hd: int, rows: int, width: int) -> bool:
    """Self-attention straight from the qkv GEMM's packed output: head dim 64, and the qkv GEMM must be able to pack ([rows, 3 * width])."""
    return current_gemm_mode() == "f16x3" and hd == 64 and fuse_supported(rows, 3 * width)


def attention_packed(qkv_packed, scale_rows, out, out_scale, B, H, L, hd, scale, v_bound):
    """qkv_packed [B*L, >= 3*H*hd] g8-packed q | k | v with one common power-of-two scale (scale_rows [B*L], all equal): the output of
    linear(..., pack_out=(scale_rows, 0.0, bound)).  out [B*L, >= H*hd] receives the g8-packed attention output, out_scale [B*L] its
    (constant) scale f16_row_scale(v_bound): linear(out, W_proj, x_scale=out_scale, x_packed=True)."""
    qp, ld = _row_view(qkv_packed, "qkv_packed")
    op, ldo = _row_view(out, "out")
    check(_lib.load().psam_attention_packed(qp, ld, scale_rows.data_ptr(), op, ldo, out_scale.data_ptr(), B, H, L, hd, float(scale), float(v_bound), _stream()),
          "psam_attention_packed")
    return out


class _Stage:
    """What the stages prepared for a coarse entry of csrc/blocks.hip share.  ENTRY names the entry (psam_x); psam_x_prepared_bytes, psam_x_prepare and
    psam_x_ws_bytes go with it.  A stage binds its weights (state-dict tensors, w: name -> contiguous fp32 device tensor) and keeps them alive, has the
    library pack them ONCE into `blob` and fill `plan`, and sizes the workspace of a call."""
    ENTRY = None

    def __init__(self):
        self.keep = []

    def _bind(self, w, name) -> int:
        t = w[name]
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{name}: contiguous fp32 expected")
        self.keep.append(t)
        return t.data_ptr()

    def _prepare(self, wt, plan, *dims):
        L = _lib.load()
        self.plan = plan
        self.blob = torch.empty(int(getattr(L, self.ENTRY + "_prepared_bytes")(*dims)), dtype=torch.uint8, device=self.keep[0].device)
        check(getattr(L, self.ENTRY + "_prepare")(ctypes.byref(wt), ctypes.byref(plan), self.blob.data_ptr(), self.blob.numel(), _stream()), self.ENTRY + "_prepare")

    def _ws(self, ws, device, *shape):
        """ws if it is large enough for a call of this shape, a new workspace otherwise."""
        need = int(getattr(_lib.load(), self.ENTRY + "_ws_bytes")(*shape))
        return ws if ws is not None and ws.numel() >= need else torch.empty(need, dtype=torch.uint8, device=device)


class _EvaStage(_Stage):
    """One transformer block of the patch encoder; prefix 'pc_encoder.transformer.blocks.i'.  NAMES: field of the weight struct -> tensor; EXTRA: further
    fields -> value."""
    EXTRA = {}

    def __init__(self, w, prefix: str, dim: int, heads: int, hidden: int, eps: float):
        super().__init__()
        wt = self.WEIGHTS()
        for slot, n in self.NAMES.items():
            setattr(wt, slot, self._bind(w, f"{prefix}.{n}"))
        for slot, v in dict(self.EXTRA, dim=int(dim), heads=int(heads), hidden=int(hidden), eps=float(eps)).items():
            setattr(wt, slot, v)
        self.dim, self.hidden = int(dim), int(hidden)
        self._prepare(wt, self.PLAN(), dim, hidden)

    def _rows(self, x, B: int, L: int, ws):
        _chk(x, name="x")
        if x.shape != (B * L, self.dim) or not x.is_contiguous():
            raise ValueError("x must be a contiguous [B*L, dim] tensor")
        return self._ws(ws, x.device, B * L, self.dim, self.hidden)


class EvaBlock(_EvaStage):
    """One EVA02 (SwiGLU) transformer block prepared for psam_eva_block (csrc/blocks.hip): packed weights + bounds, built once at load by the
    library itself (psam_eva_block_prepare) from the state-dict tensors.  w: name -> fp32 device tensor; prefix 'pc_encoder.transformer.blocks.i'."""
    ENTRY, WEIGHTS, PLAN = "psam_eva_block", _lib.EvaBlockWeights, _lib.EvaBlockPlan
    NAMES = dict(norm1_w="norm1.weight", norm1_b="norm1.bias", q_w="attn.q_proj.weight", q_b="attn.q_proj.bias", k_w="attn.k_proj.weight",
                 v_w="attn.v_proj.weight", v_b="attn.v_proj.bias", proj_w="attn.proj.weight", proj_b="attn.proj.bias", norm2_w="norm2.weight",
                 norm2_b="norm2.bias", fc1_g_w="mlp.fc1_g.weight", fc1_g_b="mlp.fc1_g.bias", fc1_x_w="mlp.fc1_x.weight", fc1_x_b="mlp.fc1_x.bias",
                 mlp_norm_w="mlp.norm.weight", mlp_norm_b="mlp.norm.bias", fc2_w="mlp.fc2.weight", fc2_b="mlp.fc2.bias")

    @staticmethod
    def supported(dim: int, heads: int, hidden: int) -> bool:
        # 256..4096: the packed LayerNorm (layernorm_can_pack); % 128: the fused epilogues of the q|k|v GEMM and fc2 (fuse_supported); what psam_eva_block_prepare accepts
        hp = (hidden + 31) // 32 * 32
        return heads > 0 and dim % heads == 0 and dim // heads == 64 and 256 <= dim <= 4096 and dim % 128 == 0 and hidden > 0 and hp % 64 == 0 and hp >= 128

    def run(self, x, B: int, L: int, ws=None):
        """x [B*L, dim] fp32, updated in place."""
        ws = self._rows(x, B, L, ws)
        check(_lib.load().psam_eva_block(ctypes.byref(self.plan), self.blob.data_ptr(), x.data_ptr(), B, L, ws.data_ptr(), ws.numel(), _stream()), "psam_eva_block")
        return x


class EvaGeluBlock(_EvaStage):
    """One block of the giant encoder (fused qkv with q / v bias, GELU MLP; timm eva_giant_patch14_560) prepared for psam_eva_gelu_block
    (csrc/blocks.hip).  w: name -> fp32 device tensor; prefix 'pc_encoder.transformer.blocks.i'."""
    PRECISION_F16X3 = 2
    ENTRY, WEIGHTS, PLAN = "psam_eva_gelu_block", _lib.EvaGeluBlockWeights, _lib.EvaGeluBlockPlan
    NAMES = dict(norm1_w="norm1.weight", norm1_b="norm1.bias", qkv_w="attn.qkv.weight", q_bias="attn.q_bias", v_bias="attn.v_bias", proj_w="attn.proj.weight",
                 proj_b="attn.proj.bias", norm2_w="norm2.weight", norm2_b="norm2.bias", fc1_w="mlp.fc1.weight", fc1_b="mlp.fc1.bias", fc2_w="mlp.fc2.weight",
                 fc2_b="mlp.fc2.bias")
    EXTRA = dict(precision=PRECISION_F16X3)

    @staticmethod
    def supported(dim: int, heads: int, hidden: int) -> bool:
        if heads <= 0 or dim % heads:
            return False
        hd = dim // heads      # what psam_eva_gelu_block_prepare accepts
        return 256 <= dim <= 4096 and dim % 32 == 0 and hidden >= 128 and hidden % 32 == 0 and (hd == 64 or (64 < hd <= 128 and hd % 8 == 0))

    def run(self, x, B: int, L: int, ws=None):
        """x [B*L, dim] fp32, updated in place."""
        ws = self._rows(x, B, L, ws)
        # the key-split cap is per CONTEXT (a latency caller next to a multi-stream pipeline on the same model): a private copy of the plan (a small
        # POD the library reads during the call only) carries it; the shared plan is never written after _prepare
        plan = _lib.EvaGeluBlockPlan.from_buffer_copy(self.plan)
        plan.attn_keysplit = current_attention_keysplit()
        check(_lib.load().psam_eva_gelu_block(ctypes.byref(plan), self.blob.data_ptr(), x.data_ptr(), B, L, ws.data_ptr(), ws.numel(), arrival_counters(x.device).data_ptr(),
                                              _stream()), "psam_eva_gelu_block")
        return x


class CPatchEncoder(_Stage):
    """A PatchEncoder (common.py:477-506) prepared for psam_patch_encoder (csrc/blocks.hip).  prefix: 'pc_encoder.patch_embed.patch_encoder' |
    'mask_encoder.patch_encoder'."""
    ENTRY = "psam_patch_encoder"

    def __init__(self, w, prefix: str, eps: float):
        super().__init__()
        wt = _lib.PatchEncoderWeights()
        for slot, n in (("c10", "conv1.0"), ("c11", "conv1.1"), ("c13", "conv1.3"), ("c20", "conv2.0"), ("c21", "conv2.1"), ("c23", "conv2.3")):
            setattr(wt, slot + "_w", self._bind(w, f"{prefix}.{n}.weight")); setattr(wt, slot + "_b", self._bind(w, f"{prefix}.{n}.bias"))
        c10, c20, c23 = w[prefix + ".conv1.0.weight"], w[prefix + ".conv2.0.weight"], w[prefix + ".conv2.3.weight"]
        wt.cin, wt.h0, wt.h1, wt.cout, wt.eps = int(c10.shape[1]), int(c10.shape[0]), int(c20.shape[0]), int(c23.shape[0]), float(eps)
        self.h0, self.h1, self.cout = wt.h0, wt.h1, wt.cout
        self._prepare(wt, _lib.PatchEncoderPlan(), wt.h0, wt.h1, wt.cout)

    @staticmethod
    def supported(h0: int, h1: int, cout: int) -> bool:
        return h0 == 128 and 256 <= h1 <= 4096 and h1 % 128 == 0 and cout >= 128 and cout % 128 == 0

    def run(self, xyz, feats, centers, knn_idx, radius=None, center_idx=None, ws=None):
        _chk(xyz); _chk(feats); _chk(centers); _chk(knn_idx, torch.int64)
        B, N, _ = xyz.shape
        rep = feats.shape[0] // B
        G, K = knn_idx.shape[1:]
        groups = B * rep * G
        out = torch.empty(groups, self.cout, dtype=torch.float32, device=xyz.device)
        ws = self._ws(ws, xyz.device, groups * K, groups, self.h0, self.h1)
        check(_lib.load().psam_patch_encoder(ctypes.byref(self.plan), self.blob.data_ptr(), xyz.data_ptr(), feats.data_ptr(), centers.data_ptr(), knn_idx.data_ptr(),
                                             _p(center_idx), B, rep, N, G, K, feats.shape[-1], float(radius or 0.0), out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
              "psam_patch_encoder")
        return out


class CUpscale(_Stage):
    """The mask decoder's upscaling + hyper-network products prepared for psam_upscale_masks (csrc/blocks.hip; mask_decoder.py:146-176)."""
    ENTRY = "psam_upscale_masks"

    def __init__(self, w, eps: float):
        super().__init__()
        wt = _lib.UpscaleWeights()
        for slot, n in (("u0", "0"), ("u1", "1"), ("u3", "3")):
            setattr(wt, slot + "_w", self._bind(w, f"mask_decoder.output_upscaling.{n}.weight")); setattr(wt, slot + "_b", self._bind(w, f"mask_decoder.output_upscaling.{n}.bias"))
        wt.dim, wt.eps = int(w["mask_decoder.output_upscaling.0.weight"].shape[0]), float(eps)
        self.dim = wt.dim
        self._prepare(wt, _lib.UpscalePlan(), wt.dim)

    def run(self, keys, idx3, w3, hyper, masks, rep, Z, N, G, C, ws=None):
        _chk(keys); _chk(idx3, torch.int64); _chk(w3); _chk(hyper); _chk(masks)
        ws = self._ws(ws, keys.device, Z, N, G, C, self.dim)
        check(_lib.load().psam_upscale_masks(ctypes.byref(self.plan), self.blob.data_ptr(), keys.data_ptr(), idx3.data_ptr(), w3.data_ptr(), hyper.data_ptr(), rep, Z, N, G, C,
                                             masks.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "psam_upscale_masks")
        return masks


class CTwoWay(_Stage):
    """The decoder's TwoWayTransformer prepared for psam_twoway_decoder (csrc/blocks.hip; transformer.py:61-100).  w: name -> fp32 tensor."""
    ENTRY = "psam_twoway_decoder"

    def __init__(self, w, prefix: str, depth: int, dim: int, heads: int, mlp: int, downsample: int, eps: float):
        super().__init__()
        if depth > _lib.TWOWAY_MAX_DEPTH:
            raise ValueError("psam_twoway_decoder: depth > PSAM_TWOWAY_MAX_DEPTH")

        def attn(dst, p):
            for slot, n in (("q", "q_proj"), ("k", "k_proj"), ("v", "v_proj"), ("o", "out_proj")):
                setattr(dst, slot + "_w", self._bind(w, f"{p}.{n}.weight")); setattr(dst, slot + "_b", self._bind(w, f"{p}.{n}.bias"))

        self.layers = (_lib.TwoWayLayerW * depth)()
        for i in range(depth):
            lp, lw = f"{prefix}.layers.{i}", self.layers[i]
            attn(lw.self_attn, lp + ".self_attn"); attn(lw.t2i, lp + ".cross_attn_token_to_image"); attn(lw.i2t, lp + ".cross_attn_image_to_token")
            for j in (1, 2, 3, 4):
                setattr(lw, f"n{j}_w", self._bind(w, f"{lp}.norm{j}.weight")); setattr(lw, f"n{j}_b", self._bind(w, f"{lp}.norm{j}.bias"))
            for j in (1, 2):
                setattr(lw, f"m{j}_w", self._bind(w, f"{lp}.mlp.lin{j}.weight")); setattr(lw, f"m{j}_b", self._bind(w, f"{lp}.mlp.lin{j}.bias"))
        wt = _lib.TwoWayWeights()
        wt.depth, wt.dim, wt.heads, wt.mlp, wt.downsample, wt.eps = depth, dim, heads, mlp, downsample, float(eps)
        wt.layers = ctypes.cast(self.layers, ctypes.POINTER(_lib.TwoWayLayerW))
        attn(wt.final_attn, prefix + ".final_attn_token_to_image")
        wt.nf_w, wt.nf_b = self._bind(w, prefix + ".norm_final_attn.weight"), self._bind(w, prefix + ".norm_final_attn.bias")
        self.dim, self.mlp = dim, mlp
        self._prepare(wt, _lib.TwoWayPlan(), depth, dim, mlp, downsample)

    def run(self, tokens, keys, pos, rep, Z, T, G, ws=None):
        """tokens [Z*T, E], keys [Z*G, E] (updated in place), pos [Z/rep, G, E] -> queries [Z*T, E]."""
        _chk(tokens); _chk(keys); _chk(pos)
        queries = torch.empty(Z * T, self.dim, dtype=torch.float32, device=tokens.device)
        ws = self._ws(ws, tokens.device, Z, T, G, self.dim, self.mlp)
        check(_lib.load().psam_twoway_decoder(ctypes.byref(self.plan), self.blob.data_ptr(), tokens.data_ptr(), keys.data_ptr(), pos.data_ptr(), rep, Z, T, G, queries.data_ptr(),
                                              ws.data_ptr(), ws.numel(), arrival_counters(tokens.device).data_ptr(), _stream()), "psam_twoway_decoder")
        return queries, keys


class TwoWayLayerWeights:
    """The weight pointers of one TwoWayAttentionBlock's token side (or of the final token -> image attention: final=True) as a
    psam_twoway_tokens_t skeleton (csrc/experiments/twoway.hip); keeps the tensors alive.  w: name -> fp32 tensor; prefix: e.g.
    'mask_decoder.transformer.layers.0' or, with final=True, 'mask_decoder.transformer' (final_attn_token_to_image / norm_final_attn)."""

    def __init__(self, w, prefix: str, final: bool = False):
        self.final = final
        self.keep = []
        a = self.args = _lib.TwoWayTokens()
        def put(slot, name):
            t = w[name]
            if t.dtype != torch.float32 or not t.is_contiguous() or t.data_ptr() % 16:
                raise ValueError(f"{name}: the two-way token kernel needs contiguous, 16-byte aligned fp32 weights")
            self.keep.append(t)
            setattr(a, slot, t.data_ptr())
            return t
        if final:
            att, norm = prefix + ".final_attn_token_to_image", prefix + ".norm_final_attn"
        else:
            att, norm = prefix + ".cross_attn_token_to_image", prefix + ".norm2"
            for s, n in (("sq", "q_proj"), ("sk", "k_proj"), ("sv", "v_proj"), ("so", "out_proj")):
                put(s + "_w", f"{prefix}.self_attn.{n}.weight"); put(s + "_b", f"{prefix}.self_attn.{n}.bias")
            put("n1_g", prefix + ".norm1.weight"); put("n1_b", prefix + ".norm1.bias")
            m1 = put("m1_w", prefix + ".mlp.lin1.weight"); put("m1_b", prefix + ".mlp.lin1.bias")
            put("m2_w", prefix + ".mlp.lin2.weight"); put("m2_b", prefix + ".mlp.lin2.bias")
            put("n3_g", prefix + ".norm3.weight"); put("n3_b", prefix + ".norm3.bias")
            put("ik_w", prefix + ".cross_attn_image_to_token.k_proj.weight"); put("ik_b", prefix + ".cross_attn_image_to_token.k_proj.bias")
            put("iv_w", prefix + ".cross_attn_image_to_token.v_proj.weight"); put("iv_b", prefix + ".cross_attn_image_to_token.v_proj.bias")
            a.mlp = int(m1.shape[0])
        cq = put("cq_w", att + ".q_proj.weight"); put("cq_b", att + ".q_proj.bias")
        put("co_w", att + ".out_proj.weight"); put("co_b", att + ".out_proj.bias")
        put("n2_g", norm + ".weight"); put("n2_b", norm + ".bias")
        self.embed, self.inner = int(cq.shape[1]), int(cq.shape[0])
        a.mode = 1 if final else 0

    @staticmethod
    def supported(E: int, inner_cross: int, heads: int, Z: int, T: int, G: int) -> bool:
        return E == 256 and inner_cross == 128 and heads in (1, 2, 4, 8, 16, 32) and Z * T <= 64 and max(T, G) <= 4096


def _need_experiments(what: str):
    if not _lib.has_experiments():
        raise _lib.PointSamHipError(f"{what} is a measured-and-rejected path: build the library with PSAM_BUILD_EXPERIMENTS=1 (python -m point_sam_amd.build)")


def twoway_tokens_ws(mlp: int, device) -> torch.Tensor:
    _need_experiments("psam_twoway_tokens")
    return torch.empty(int(_lib.load().psam_twoway_tokens_ws_floats(int(mlp))), dtype=torch.float32, device=device)


def twoway_tokens(lw: TwoWayLayerWeights, queries, pe, kimg, vimg, Z, T, G, heads, eps, ws, ktok=None, vtok=None, skip_pe=False):
    """One launch for the token side of a two-way layer (csrc/experiments/twoway.hip; transformer.py:144-175): queries [Z*T, 256] updated in place; pe the
    token embeddings (query_pe); kimg / vimg [Z*G, 128] row views of the patch tokens' k / v projections; ktok / vtok [Z*T, 128] receive the
    k / v projections for the image -> token attention (not for the final attention)."""
    import ctypes
    _need_experiments("psam_twoway_tokens")
    a = lw.args
    _chk(queries, name="queries"); _chk(pe, name="pe")
    kp, ldk = _row_view(kimg, "kimg"); vp, ldv = _row_view(vimg, "vimg")
    a.Z, a.T, a.G, a.heads, a.skip_pe, a.eps = int(Z), int(T), int(G), int(heads), int(bool(skip_pe)), float(eps)
    a.queries, a.pe = queries.data_ptr(), pe.data_ptr()
    a.kimg, a.ldk, a.sk, a.vimg, a.ldv, a.sv = kp, ldk, G * ldk, vp, ldv, G * ldv
    a.ktok, a.vtok = (0, 0) if lw.final else (ktok.data_ptr(), vtok.data_ptr())
    a.ws, a.ws_floats = ws.data_ptr(), ws.numel()
    check(_lib.load().psam_twoway_tokens(ctypes.byref(a), _stream()), "psam_twoway_tokens")
    return queries


class Mlp3Weights:
    """Three Linear layers (ReLU between) of M stacked MLPs for psam_mlp3: w? [M, out, in] (the reference's layout), b? [M, out]."""

    def __init__(self, layers):
        # layers: list over MLPs of [(W1, b1), (W2, b2), (W3, b3)] with W [out, in]
        st = lambda i: (torch.stack([m[i][0] for m in layers]).contiguous(), torch.stack([m[i][1] for m in layers]).contiguous())
        (self.w1, self.b1), (self.w2, self.b2), (self.w3, self.b3) = st(0), st(1), st(2)
        self.M, self.dh, self.din = self.w1.shape
        self.dout = self.w3.shape[1]
        if self.w2.shape[1:] != (self.dh, self.dh) or self.w3.shape[2] != self.dh:
            raise ValueError("Mlp3Weights: layer shapes do not chain")


def mlp3(x, ldx, sx, mw: Mlp3Weights, out, ldo, so, Z):
    """out[z, m] = W3_m relu(W2_m relu(W1_m x[z, m] + b1) + b2) + b3: row (z, m) of x at x.data_ptr() + 4 * (z * ldx + m * sx) (fp32
    elements), of out at + 4 * (z * ldo + m * so).  One launch for all M MLPs and Z rows (mask_decoder.py:171-180,189-211)."""
    for t in (x, out):
        if not (t.is_cuda and t.dtype == torch.float32):
            raise _lib.PointSamHipError("mlp3: operands must be fp32 tensors on the GPU (there is no CPU fallback)")
    check(_lib.load().psam_mlp3(x.data_ptr(), ldx, sx, mw.w1.data_ptr(), mw.b1.data_ptr(), mw.w2.data_ptr(), mw.b2.data_ptr(), mw.w3.data_ptr(),
                                mw.b3.data_ptr(), out.data_ptr(), ldo, so, Z, mw.M, mw.din, mw.dh, mw.dout, _stream()), "psam_mlp3")
    return out


def mlp3_pair(xa, ldxa, sxa, mwa: Mlp3Weights, outa, ldoa, soa, xb, ldxb, sxb, mwb: Mlp3Weights, outb, ldob, sob, Z):
    """mlp3 of stack a and of stack b over the same Z rows in ONE launch (the hyper-networks and the IoU head, mask_decoder.py:167-182): the same
    bits as two mlp3 calls."""
    for t in (xa, outa, xb, outb):
        if not (t.is_cuda and t.dtype == torch.float32):
            raise _lib.PointSamHipError("mlp3_pair: operands must be fp32 tensors on the GPU (there is no CPU fallback)")
    def args(x, ldx, sx, mw, out, ldo, so):
        return _lib.Mlp3Args(x.data_ptr(), mw.w1.data_ptr(), mw.b1.data_ptr(), mw.w2.data_ptr(), mw.b2.data_ptr(), mw.w3.data_ptr(), mw.b3.data_ptr(), out.data_ptr(),
                             ldx, sx, ldo, so, mw.M, mw.din, mw.dh, mw.dout)
    a, b = args(xa, ldxa, sxa, mwa, outa, ldoa, soa), args(xb, ldxb, sxb, mwb, outb, ldob, sob)
    check(_lib.load().psam_mlp3_pair(ctypes.byref(a), ctypes.byref(b), Z, _stream()), "psam_mlp3_pair")
    return outa, outb


def skinny_ln_supported(M, N, K) -> bool:
    """linear_skinny_ln's shapes."""
    return 0 < M <= SKINNY_MAX_M and N == 256 and K % 16 == 0


def linear_skinny_ln(x, W, bias, ln_w, ln_b, eps, residual=None, out=None):
    """out [M, 256] = LayerNorm(x W^T + bias + residual) * ln_w + ln_b for M <= 64 rows in ONE launch (csrc/gemm.hip linear_skinny_ln_kernel: the last
    workgroup to finish its columns normalises the rows) -- the `queries = norm(queries + out_proj(attn))` steps of the decoder (transformer.py:153-176)."""
    for t, n in ((ln_w, "ln_w"), (ln_b, "ln_b")):
        _chk(t, name=n)
    M, K = x.shape
    N = W.shape[0]
    xp, ldx = _row_view(x, "x"); wp, ldw = _row_view(W, "W")
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=x.device)
    op, ldo = _row_view(out, "out")
    rp, ldr = (0, 0) if residual is None else _row_view(residual, "residual")
    L = _lib.load()
    tmp = torch.empty(L.psam_linear_skinny_ln_tmp_floats(M, K), dtype=torch.float32, device=x.device)
    check(L.psam_linear_skinny_ln(xp, ldx, wp, ldw, _p(bias), rp, ldr, ln_w.data_ptr(), ln_b.data_ptr(), eps, tmp.data_ptr(), op, ldo, M, N, K,
                                  arrival_counters(x.device).data_ptr(), _stream()), "psam_linear_skinny_ln")
    return out


def _skinny_jobs(what, x, jobs, outs):
    """psam_skinny_jobs_t of jobs = [(W, bias | None, xadd | None, act), ..] over the rows of x -> (js, outs, ldx, ldxadd, ldw).  outs: None, or one
    [M, N_i] row view per job to write into (any row stride)."""
    xp, ldx = _row_view(x, "x")
    M = x.shape[0]
    if not 1 <= len(jobs) <= len(_lib.SkinnyJobs().job) or (outs is not None and len(outs) != len(jobs)):
        raise ValueError(f"{what}: one to {len(_lib.SkinnyJobs().job)} jobs, and an output per job")
    js = _lib.SkinnyJobs()
    js.n = len(jobs)
    ys, ldw, ldxa = [], None, None
    for i, (W, bias, xadd, act) in enumerate(jobs):
        wp, lw = _row_view(W, "W")
        if ldw not in (None, lw):
            raise ValueError(f"{what}: the weights must share their row stride")
        ldw = lw
        y = torch.empty(M, W.shape[0], dtype=torch.float32, device=x.device) if outs is None else outs[i]
        yp, ldy = _row_view(y, "out")
        if tuple(y.shape) != (M, W.shape[0]):
            raise ValueError(f"{what}: output {i} must be [{M}, {W.shape[0]}], got {tuple(y.shape)}")
        ys.append(y)
        ap = 0
        if xadd is not None:
            ap, la = _row_view(xadd, "xadd")
            if ldxa not in (None, la):
                raise ValueError(f"{what}: the addends must share their row stride")
            ldxa = la
        js.job[i] = _lib.SkinnyJob(xp, ap, wp, _p(bias), yp, ldy, W.shape[0], act)
    return js, ys, ldx, ldx if ldxa is None else ldxa, ldw


def linear_rows_multi(x, jobs, xadd_rows_per_set=1, xadd_rep=1, outs=None):
    """[y_i] = [act_i((x + xadd_i) W_i^T + bias_i)] for jobs = [(W, bias | None, xadd | None, act), ..] over the same rows of x in ONE launch, exact fp32
    products (csrc/gemm.hip linear_rows_multi_kernel: 32 x 64 tiles; a few hundred to a few thousand rows).  xadd_i: sets of xadd_rows_per_set rows, set
    (row // (xadd_rep * xadd_rows_per_set)) is added to row `row` (the decoder's key_pe).  outs: row views to write into instead of new tensors."""
    js, ys, ldx, ldxa, ldw = _skinny_jobs("linear_rows_multi", x, jobs, outs)
    M, K = x.shape
    check(_lib.load().psam_linear_rows_multi(ctypes.byref(js), ldx, ldxa, xadd_rows_per_set, xadd_rep, ldw, M, K, _stream()), "psam_linear_rows_multi")
    return ys


def linear_skinny_multi(x, jobs, outs=None):
    """[y_i] = [act_i((x + xadd_i) W_i^T + bias_i)] for jobs = [(W, bias | None, xadd | None, act), ..] (linear_rows_multi's tuples; xadd_i [M, K], row for
    row) over the same M <= 64 rows of x in ONE launch (csrc/gemm.hip linear_skinny_multi_kernel: the q / k / v projections of a decoder attention): per
    job the bits of linear() on the pre-added input."""
    js, ys, ldx, ldxa, ldw = _skinny_jobs("linear_skinny_multi", x, jobs, outs)
    M, K = x.shape
    check(_lib.load().psam_linear_skinny_multi(ctypes.byref(js), ldx, ldxa, ldw, M, K, _stream()), "psam_linear_skinny_multi")
    return ys


def linear_ln256(x, W, bias, ln_w, ln_b, eps, residual=None, out=None):
    """out [M, 256] = LayerNorm(x W^T + bias + residual) * ln_w + ln_b for any M and a short K (K % 16 == 0, K <= 512) in one launch (csrc/gemm.hip
    linear_ln256_kernel: a workgroup per 16 whole rows, exact fp32 products) -- `keys = norm4(keys + out_proj(attn))`, transformer.py:170-175."""
    for t, n in ((ln_w, "ln_w"), (ln_b, "ln_b")):
        _chk(t, name=n)
    M, K = x.shape
    N = W.shape[0]
    xp, ldx = _row_view(x, "x"); wp, ldw = _row_view(W, "W")
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=x.device)
    op, ldo = _row_view(out, "out")
    rp, ldr = (0, 0) if residual is None else _row_view(residual, "residual")
    check(_lib.load().psam_linear_ln256(xp, ldx, wp, ldw, _p(bias), rp, ldr, ln_w.data_ptr(), ln_b.data_ptr(), eps, op, ldo, M, N, K, _stream()), "psam_linear_ln256")
    return out


def attention_small(q, k, v, out, Z, H, Lq, Lk, hd, scale):
    qp, ldq = _row_view(q, "q"); kp, ldk = _row_view(k, "k"); vp, ldv = _row_view(v, "v"); op, ldo = _row_view(out, "out")
    check(_lib.load().psam_attention_small(qp, ldq, Lq * ldq, kp, ldk, Lk * ldk, vp, ldv, Lk * ldv, op, ldo, Lq * ldo, Z, H, Lq, Lk, hd, scale,
                                           _stream()), "psam_attention_small")
    return out


# ------------------------------------------------------------------------------------------ encodings etc.
def pos_l1(centers, W, bias, out=None):
    _chk(centers)
    rows = centers.numel() // 3
    if out is None:
        out = torch.empty(rows, 128, dtype=torch.float32, device=centers.device)
    check(_lib.load().psam_pos_l1(centers.data_ptr(), W.data_ptr(), bias.data_ptr(), out.data_ptr(), rows, _stream()), "psam_pos_l1")
    return out


def fourier_pe(coords, gauss, out, rows_per_batch, batch_stride, labels=None, emb0=None, emb1=None, flag=None):
    """coords [..., 3] -> writes [sin,cos] (+label embedding) rows into ``out`` (see header for the row mapping)."""
    _chk(coords)
    rows = coords.numel() // 3
    F = gauss.shape[1]
    if labels is not None:
        _chk(labels, torch.int64, "labels")
    check(_lib.load().psam_fourier_pe(coords.data_ptr(), gauss.data_ptr(), F, _p(labels), _p(emb0), _p(emb1), out.data_ptr(), rows, rows_per_batch,
                                      batch_stride, _p(flag), _stream()), "psam_fourier_pe")
    return out


def add_bcast(a, rep, b, out, Z, R, C, sa=None, sb=None, ldb=None, so=None):
    sa = R * C if sa is None else sa
    so = R * C if so is None else so
    if b is None:
        sb, ldb = 0, 0
    else:
        sb = R * C if sb is None else sb
        ldb = C if ldb is None else ldb
    check(_lib.load().psam_add_bcast(a.data_ptr(), sa, rep, _p(b), sb, ldb, out.data_ptr(), so, Z, R, C, _stream()), "psam_add_bcast")
    return out


def interp3(src, idx3, w3, out, rep, scale_out=None, ln=None, act=ACT_NONE):
    """src [Z,G,C], idx3/w3 [B,N,3] -> out [Z,N,C]; scale_out [Z*N] (C == 256): out receives the g8-packed rows + their scales;
    ln=(gamma, beta, eps) (C == 256): LayerNorm and the activation `act` applied to every interpolated row."""
    Z, G, C = src.shape
    N = idx3.shape[1]
    g, b, eps = ln if ln is not None else (None, None, 0.0)
    check(_lib.load().psam_interp3_ex(src.data_ptr(), idx3.data_ptr(), w3.data_ptr(), out.data_ptr(), rep, Z, N, G, C, _p(scale_out), _p(g), _p(b),
                                      float(eps), int(act), _stream()), "psam_interp3")
    return out


# ------------------------------------------------------------------------------------------ click simulation (eval protocol)
def error_regions(gt: torch.Tensor, logits):
    """gt [Z,N] uint8/bool, logits [Z,N] f32 or None -> (fn, fp) uint8 [Z,N].  common.py:388-405."""
    gt = _chk(gt.to(torch.uint8), torch.uint8, "gt")
    if logits is not None:
        _chk(logits, name="logits")
    fn, fp = torch.empty_like(gt), torch.empty_like(gt)
    check(_lib.load().psam_error_regions(gt.data_ptr(), _p(logits), fn.data_ptr(), fp.data_ptr(), gt.numel(), _stream()), "psam_error_regions")
    return fn, fp


def border_farthest(xyz: torch.Tensor, region: torch.Tensor):
    """xyz [B,N,3], region [Z,N] uint8 -> (idx [Z] int64, dist2 [Z]); -1 where the region or its complement is empty.
    common.py:443-474."""
    _chk(xyz, name="xyz")
    region = _chk(region.to(torch.uint8), torch.uint8, "region")
    B, N, _ = xyz.shape
    Z = region.shape[0]
    L = _lib.load()
    nbytes = L.psam_border_farthest_workspace_bytes(Z, N)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=xyz.device)
    idx = torch.empty(Z, dtype=torch.int64, device=xyz.device)
    dist = torch.empty(Z, dtype=torch.float32, device=xyz.device)
    check(L.psam_border_farthest(xyz.data_ptr(), region.data_ptr(), B, Z // B, N, idx.data_ptr(), dist.data_ptr(), ws.data_ptr(), nbytes, _stream()),
          "psam_border_farthest")
    return idx, dist


# ------------------------------------------------------------------------------------------ mask proposals (csrc/masks.hip)
# A mask is a row of W = ceil(N / 64) 64-bit words (bit n % 64 of word n / 64 is point n, bits past N are zero).  The words travel as torch.int64:
# same bits as the library's uint64_t, and indexing / comparison / shifts exist for that dtype on every torch build.
def mask_words(N: int) -> int:
    return (N + 63) // 64


def mask_pack(logits: torch.Tensor, thr: float = 0.0, off: float = 1.0, out=None, row: int = 0):
    """logits [K, N] f32 (or [Z, C, N], rows K = Z * C) -> (bits [K, W] int64, area, area_hi, area_lo [K] int32): bit = logit > thr (NaN false);
    area_hi / area_lo count logit > fl32(thr + off) / logit > fl32(thr - off).  out = (bits, area, area_hi, area_lo) of a larger buffer and
    `row`: the K rows land at rows row .. row + K - 1 of it (chunks of one cloud's candidates)."""
    _chk(logits, name="logits")
    N = logits.shape[-1]
    K = logits.numel() // max(N, 1)
    W = mask_words(N)
    if out is None:
        if row != 0:
            raise ValueError("mask_pack: a destination row needs the destination buffers (out=)")
        out = (torch.empty(K, W, dtype=torch.int64, device=logits.device),) + tuple(torch.empty(K, dtype=torch.int32, device=logits.device) for _ in range(3))
    bits, area, area_hi, area_lo = out
    _chk(bits, torch.int64, "bits")
    for t in (area, area_hi, area_lo):
        _chk(t, torch.int32, "area")
    if bits.dim() != 2 or bits.shape[1] != W or row < 0 or row + K > bits.shape[0] or min(area.numel(), area_hi.numel(), area_lo.numel()) < bits.shape[0]:
        raise ValueError(f"mask_pack: rows {row} .. {row + K - 1} of width {W} do not fit bits {tuple(bits.shape)} / areas [{area.numel()}]")
    check(_lib.load().psam_mask_pack(logits.data_ptr(), N, K, N, float(thr), float(off), row, bits.data_ptr(), area.data_ptr(), area_hi.data_ptr(),
                                     area_lo.data_ptr(), _stream()), "psam_mask_pack")
    return bits, area, area_hi, area_lo


def mask_valid(area, area_hi, area_lo, score, N: int, min_points: int, max_area_frac: float, pred_iou_thr: float, stab_thr: float) -> torch.Tensor:
    """-> valid [K] uint8: area >= min_points, area < max_area_frac * N, score >= pred_iou_thr (NaN false), area_lo > 0 and
    area_hi >= stab_thr * area_lo (products in fp64: exact)."""
    for t in (area, area_hi, area_lo):
        _chk(t, torch.int32, "area")
    _chk(score, name="score")
    K = area.numel()
    if not (area_hi.numel() == area_lo.numel() == score.numel() == K):
        raise ValueError("mask_valid: the areas and the scores must have one entry per candidate")
    valid = torch.empty(K, dtype=torch.uint8, device=area.device)
    check(_lib.load().psam_mask_valid(area.data_ptr(), area_hi.data_ptr(), area_lo.data_ptr(), score.data_ptr(), K, N, int(min_points),
                                      float(max_area_frac), float(pred_iou_thr), float(stab_thr), valid.data_ptr(), _stream()), "psam_mask_valid")
    return valid


def mask_intersections(a: torch.Tensor, b: torch.Tensor = None) -> torch.Tensor:
    """a [Ka, W], b [Kb, W] int64 words -> inter [Ka, Kb] int32 = popcount(a_i & b_j).  b None (or the same tensor): a against itself, the upper
    triangle computed and mirrored."""
    _chk(a, torch.int64, "a")
    b = a if b is None else _chk(b, torch.int64, "b")
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise ValueError(f"mask_intersections: {tuple(a.shape)} against {tuple(b.shape)}")
    inter = torch.empty(a.shape[0], b.shape[0], dtype=torch.int32, device=a.device)
    check(_lib.load().psam_mask_intersections(a.data_ptr(), b.data_ptr(), a.shape[0], b.shape[0], a.shape[1], inter.data_ptr(), _stream()),
          "psam_mask_intersections")
    return inter


def mask_nms(order, valid, area, inter, iou_thr: float) -> torch.Tensor:
    """Greedy suppression on the device: order [K] int32 (a permutation, best first), valid [K] uint8, area [K] int32, inter [K, K] int32 ->
    keep [K] uint8.  Candidate i is kept iff valid[i] and no already kept j has inter_ij > iou_thr * (area_i + area_j - inter_ij) (fp64)."""
    _chk(order, torch.int32, "order"); _chk(valid, torch.uint8, "valid"); _chk(area, torch.int32, "area"); _chk(inter, torch.int32, "inter")
    K = order.numel()
    if valid.numel() != K or area.numel() != K or tuple(inter.shape) != (K, K):
        raise ValueError(f"mask_nms: K = {K}, valid [{valid.numel()}], area [{area.numel()}], inter {tuple(inter.shape)}")
    L = _lib.load()
    nbytes = L.psam_mask_nms_workspace_bytes(K)
    ws = torch.empty(max(nbytes, 16) // 8 + 1, dtype=torch.int64, device=order.device)
    keep = torch.empty(K, dtype=torch.uint8, device=order.device)
    check(L.psam_mask_nms(order.data_ptr(), valid.data_ptr(), area.data_ptr(), inter.data_ptr(), K, float(iou_thr), keep.data_ptr(), ws.data_ptr(),
                          ws.numel() * 8, _stream()), "psam_mask_nms")
    return keep


def mask_paint(bits, order, keep, N: int) -> torch.Tensor:
    """bits [K, W], order [K] int32, keep [K] uint8 -> labels [N] int32: the rank (0 = best, among the kept masks in `order`) of the best kept mask
    that contains the point, -1 where none does."""
    _chk(bits, torch.int64, "bits"); _chk(order, torch.int32, "order"); _chk(keep, torch.uint8, "keep")
    K = order.numel()
    if bits.dim() != 2 or bits.shape[0] != K or bits.shape[1] != mask_words(N) or keep.numel() != K:
        raise ValueError(f"mask_paint: K = {K}, N = {N}, bits {tuple(bits.shape)}, keep [{keep.numel()}]")
    L = _lib.load()
    nbytes = L.psam_mask_paint_workspace_bytes(K)
    ws = torch.empty(max(nbytes, 16) // 4 + 1, dtype=torch.int32, device=bits.device)
    labels = torch.empty(N, dtype=torch.int32, device=bits.device)
    check(L.psam_mask_paint(bits.data_ptr(), order.data_ptr(), keep.data_ptr(), K, N, labels.data_ptr(), ws.data_ptr(), ws.numel() * 4, _stream()),
          "psam_mask_paint")
    return labels


def mask_unpack(bits: torch.Tensor, N: int) -> torch.Tensor:
    """bits [k, W] int64 words -> [k, N] bool (plain torch; for inspection and tests, not on a hot path)."""
    sh = torch.arange(64, device=bits.device, dtype=torch.int64)
    return ((bits.unsqueeze(-1) >> sh) & 1).to(torch.bool).reshape(bits.shape[0], -1)[:, :N]


# ------------------------------------------------------------------------------------------ full-resolution scenes (csrc/scene.hip)
def _voxel_setup(name: str, voxel_size, optional: bool, M: int, dev):
    """What voxel_downsample and crop_downsample (`name`: voxel / crop) share -> (inv_h fp32, workspace).  optional: voxel_size None = no reduction,
    inv_h 0."""
    import numpy as np
    inv_h = np.float32(0)
    if not (optional and voxel_size is None):
        h = np.float32(voxel_size)
        if not (np.isfinite(h) and h > 0):
            raise ValueError(f"{name}_downsample: voxel_size must be finite and positive{' (None: no reduction)' if optional else ''}, got {voxel_size!r}")
        inv_h = np.float32(1) / h                          # fp32, as the header defines it
        if not (np.isfinite(inv_h) and inv_h > 0):
            raise ValueError(f"{name}_downsample: 1 / voxel_size is not a positive fp32 number for voxel_size {voxel_size!r}")
    nbytes = getattr(_lib.load(), f"psam_{name}_downsample_workspace_bytes")(M)
    if nbytes == 0:
        raise ValueError(f"{name}_downsample: {M} points exceed the 2^28 the table is built for")
    return inv_h, torch.empty(nbytes // 8 + 2, dtype=torch.int64, device=dev)      # torch allocations are at least 16-byte aligned


def _expand_rows(name: str, src, inv, fill, out):
    """scene_expand_rows (fill None: the entry point takes none) and crop_expand_rows."""
    if not src.is_cuda:
        raise _lib.PointSamHipError("src must live on the GPU: the HIP path has no CPU fallback")
    if src.dtype not in (torch.float32, torch.int32):
        raise TypeError(f"{name}: rows of 32-bit words (float32 / int32), got {src.dtype}")
    _chk(inv, torch.int64, "inv")
    pattern = () if fill is None else (_fill_pattern(fill, src.dtype),)
    Nw, M = src.shape[-1], inv.numel()
    lead = tuple(src.shape[:-1])
    rows = src.reshape(-1, Nw) if src.dim() != 2 else src
    if rows.stride(1) != 1 and Nw > 1:
        rows = rows.contiguous()
    R = rows.shape[0]
    if R < 1 or Nw < 1 or M < 1:
        raise ValueError(f"{name}: empty input: src {tuple(src.shape)}, inv [{M}]")
    src_ld = rows.stride(0) if R > 1 else Nw
    if src_ld < Nw:
        rows, src_ld = rows.contiguous(), Nw
    if out is None:
        dst = torch.empty(R, M, dtype=src.dtype, device=src.device)
    else:
        dst = out
        if dst.dtype != src.dtype or dst.dim() != 2 or tuple(dst.shape) != (R, M) or (M > 1 and dst.stride(1) != 1) or (R > 1 and dst.stride(0) < M):
            raise ValueError(f"{name}: out must be [{R}, {M}] {src.dtype} with unit column stride, got {tuple(dst.shape)} {dst.dtype}")
    dst_ld = dst.stride(0) if R > 1 else M
    check(getattr(_lib.load(), "psam_" + name)(rows.data_ptr(), src_ld, inv.data_ptr(), R, Nw, M, *pattern, dst.data_ptr(), dst_ld, _stream()), "psam_" + name)
    return dst if out is not None else dst.reshape(lead + (M,))


def _expand_bits(name: str, arg: str, bits, inv, Nw: int, area: bool):
    """scene_expand_bits and crop_expand_bits; arg: what the caller calls `bits`."""
    _chk(bits, torch.int64, arg); _chk(inv, torch.int64, "inv")
    M = inv.numel()
    if bits.dim() != 2 or Nw < 1 or bits.shape[1] != mask_words(Nw) or M < 1:
        raise ValueError(f"{name}: {arg} {tuple(bits.shape)} for Nw = {Nw}, inv [{M}]")
    K = bits.shape[0]
    bits_f = torch.empty(K, mask_words(M), dtype=torch.int64, device=bits.device)
    area_f = torch.empty(K, dtype=torch.int32, device=bits.device) if area else None
    if K > 0:
        check(getattr(_lib.load(), "psam_" + name)(bits.data_ptr(), inv.data_ptr(), K, Nw, M, bits_f.data_ptr(), _p(area_f), _stream()), "psam_" + name)
    return bits_f, area_f


def _voxel_call(xyz, voxel_size, origin, full: bool):
    import numpy as np
    if xyz.dim() == 3 and xyz.shape[0] == 1:
        xyz = xyz[0]
    _chk(xyz, name="xyz")
    if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] < 1:
        raise ValueError(f"voxel_downsample: xyz must be [M, 3] with M >= 1 (one scene), got {tuple(xyz.shape)}")
    M, dev = xyz.shape[0], xyz.device
    inv_h, ws = _voxel_setup("voxel", voxel_size, False, M, dev)
    org = (ctypes.c_float * 3)(*[float(v) for v in origin])
    keep_idx = torch.empty(M, dtype=torch.int64, device=dev) if full else None
    inv = torch.empty(M, dtype=torch.int64, device=dev) if full else None
    cf = torch.empty(2, dtype=torch.int32, device=dev)    # count, flag: read together, the call's one host synchronisation
    check(_lib.load().psam_voxel_downsample(xyz.data_ptr(), M, ctypes.addressof(org), float(inv_h), _p(keep_idx), _p(inv), cf.data_ptr(),
                                            cf.data_ptr() + 4, ws.data_ptr(), ws.numel() * 8, _stream()), "psam_voxel_downsample")
    count, flag = cf.tolist()
    if flag != 0:
        raise ValueError(f"voxel_downsample: a coordinate is not finite, or its cell at voxel size {float(np.float32(voxel_size))} from origin "
                         f"{tuple(float(v) for v in origin)} falls outside [0, 2^21)")
    return count, keep_idx, inv


def voxel_downsample(xyz: torch.Tensor, voxel_size: float, origin=(-1.0, -1.0, -1.0)):
    """xyz [M, 3] f32 -> (keep_idx [count] int64, inv [M] int64).  Cell = floor((x - origin) * fl32(1 / voxel_size)) per axis in fp32; keep_idx = the
    lowest point index of every occupied voxel, increasing; inv[i] = the position in keep_idx of point i's representative (inv[keep_idx[j]] == j).
    ValueError for a non-finite coordinate or a cell outside [0, 2^21).  One host synchronisation: the read of the count."""
    count, keep_idx, inv = _voxel_call(xyz, voxel_size, origin, True)
    return keep_idx[:count], inv


def voxel_count(xyz: torch.Tensor, voxel_size: float, origin=(-1.0, -1.0, -1.0)) -> int:
    """The number of occupied voxels (the length of voxel_downsample's keep_idx) without writing the index arrays."""
    return _voxel_call(xyz, voxel_size, origin, False)[0]


def scene_expand_rows(src: torch.Tensor, inv: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """src [..., Nw] f32 or int32 (the leading dimensions are R rows with one stride; last stride 1), inv [M] int64 -> [..., M] of the same dtype:
    out[r, i] = src[r, inv[i]] bit for bit.  out: a [R, M] destination with its own row stride."""
    return _expand_rows("scene_expand_rows", src, inv, None, out)


def scene_expand_bits(bits_w: torch.Tensor, inv: torch.Tensor, Nw: int, area: bool = True):
    """bits_w [K, ceil(Nw / 64)] int64 words (mask_pack's layout), inv [M] int64 -> (bits_f [K, ceil(M / 64)] int64, area_f [K] int32 or None):
    bit i of a full row = bit inv[i] of the working row; bits past M are zero; area_f = the full rows' popcounts."""
    return _expand_bits("scene_expand_bits", "bits_w", bits_w, inv, Nw, area)


# ------------------------------------------------------------------------------------------ scene crops (csrc/crops.hip)
def _crop_call(xyz, rgb, center, radius, voxel_size, full: bool):
    import numpy as np
    if xyz.dim() == 3 and xyz.shape[0] == 1:
        xyz = xyz[0]
    _chk(xyz, name="xyz")
    if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] < 1:
        raise ValueError(f"crop_downsample: xyz must be [M, 3] with M >= 1 (one scene), got {tuple(xyz.shape)}")
    if full:
        if rgb.dim() == 3 and rgb.shape[0] == 1:
            rgb = rgb[0]
        _chk(rgb, name="rgb")
        if tuple(rgb.shape) != tuple(xyz.shape):
            raise ValueError(f"crop_downsample: rgb must be {tuple(xyz.shape)} like xyz, got {tuple(rgb.shape)}")
    c = np.asarray([float(v) for v in center], dtype=np.float32) if len(center) == 3 else None
    if c is None or not np.isfinite(c).all():
        raise ValueError(f"crop_downsample: center must be three finite fp32 numbers, got {center!r}")
    if isinstance(radius, bool) or not isinstance(radius, (int, float, np.floating)):
        raise ValueError(f"crop_downsample: radius must be a number, got {radius!r}")
    r = np.float32(radius)
    with np.errstate(over="ignore", divide="ignore"):
        r2, inv_r = r * r, np.float32(1) / r               # fp32, as the header defines them
    if not (np.isfinite(r) and r > 0 and np.isfinite(r2) and r2 > 0 and np.isfinite(inv_r)):
        raise ValueError(f"crop_downsample: radius must be positive with fp32 r * r and 1 / r finite and positive, got {radius!r}")
    M, dev = xyz.shape[0], xyz.device
    inv_h, ws = _voxel_setup("crop", voxel_size, True, M, dev)
    org = (ctypes.c_float * 3)(*[float(v) for v in c])
    keep_idx = torch.empty(M, dtype=torch.int64, device=dev) if full else None
    inv = torch.empty(M, dtype=torch.int64, device=dev) if full else None
    wxyz = torch.empty(M, 3, dtype=torch.float32, device=dev) if full else None
    wrgb = torch.empty(M, 3, dtype=torch.float32, device=dev) if full else None
    res = torch.empty(3, dtype=torch.int32, device=dev)   # count, members, flag: read together, the call's one host synchronisation
    check(_lib.load().psam_crop_downsample(xyz.data_ptr(), _p(rgb if full else None), M, ctypes.addressof(org), float(r2), float(inv_r), float(inv_h),
                                           _p(keep_idx), _p(inv), _p(wxyz), _p(wrgb), res.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream()),
          "psam_crop_downsample")
    count, members, flag = res.tolist()
    if flag != 0:
        raise ValueError(f"crop_downsample: a cell of the ball at voxel size {voxel_size!r} (crop units) falls outside [0, 2^21)")
    return count, members, keep_idx, inv, wxyz, wrgb


def crop_downsample(xyz: torch.Tensor, rgb: torch.Tensor, center, radius: float, voxel_size: float = None):
    """The ball |x - center| <= radius of a scan as a cloud of its own.  xyz, rgb [M, 3] f32 -> (keep_idx [count] int64, inv [M] int64,
    wxyz [count, 3], wrgb [count, 3], members).  In fp32, every operation rounded on its own: d = x - c, q = (dx dx + dy dy) + dz dz, a point is a
    member iff q <= r * r (a non-finite point is none); u = clamp(d * (1 / r), -1, 1); cell = floor((u + 1) * fl32(1 / voxel_size)), voxel_size in
    crop units.  keep_idx = the lowest MEMBER index of every occupied voxel, increasing (voxel_size None: every member); inv[i] = the position in
    keep_idx of member i's representative, -1 off the ball; wxyz = u of the representatives, wrgb = rgb[keep_idx].  count may be 0 (an empty ball).
    ValueError for a non-finite centre, radius <= 0, or a cell outside [0, 2^21).  One host synchronisation: the read of the counts.  The four
    outputs are sized for M points while the kernels run; the returned tensors are copies of the count rows actually written."""
    count, members, keep_idx, inv, wxyz, wrgb = _crop_call(xyz, rgb, center, radius, voxel_size, True)
    return keep_idx[:count].clone(), inv, wxyz[:count].clone(), wrgb[:count].clone(), members


def crop_count(xyz: torch.Tensor, center, radius: float, voxel_size: float = None):
    """-> (count, members): the lengths crop_downsample would return, without writing the index arrays or the gathered cloud."""
    return _crop_call(xyz, None, center, radius, voxel_size, False)[:2]


def _fill_pattern(fill, dtype) -> int:
    import struct
    if dtype == torch.float32:
        return struct.unpack("<I", struct.pack("<f", float(fill)))[0]
    if isinstance(fill, bool) or not isinstance(fill, int) or not -2 ** 31 <= fill < 2 ** 31:
        raise ValueError(f"crop_expand_rows: the fill of int32 rows must be an int32 value, got {fill!r}")
    return fill & 0xFFFFFFFF


def crop_expand_rows(src: torch.Tensor, inv: torch.Tensor, fill, out: torch.Tensor = None) -> torch.Tensor:
    """scene_expand_rows for a crop: out[r, i] = src[r, inv[i]] bit for bit where inv[i] >= 0, `fill` (a value of src's dtype: -inf for logits, -1 for
    labels) elsewhere.  src [..., Nw] f32 or int32, inv [M] int64 -> [..., M]."""
    return _expand_rows("crop_expand_rows", src, inv, fill, out)


def crop_expand_bits(bits: torch.Tensor, inv: torch.Tensor, Nw: int, area: bool = True):
    """scene_expand_bits for a crop: bits [K, ceil(Nw / 64)] int64 words, inv [M] int64 -> (bits_f [K, ceil(M / 64)] int64, area_f [K] int32 or None):
    bit i of a full row = bit inv[i] of the crop's row where inv[i] >= 0, zero elsewhere and past M; area_f = the full rows' popcounts."""
    return _expand_bits("crop_expand_bits", "bits", bits, inv, Nw, area)


# ------------------------------------------------------------------------------------------ interpolated scene masks (csrc/scene_interp.hip)
def scene_interp_plan(xyz: torch.Tensor, inv: torch.Tensor, wxyz: torch.Tensor, nbr: torch.Tensor, center=None, radius: float = None, eps: float = 1e-8):
    """xyz [M, 3] f32 (the scan), inv [M] int64, wxyz [Nw, 3] f32 (the working cloud as encoded), nbr [Nw, 26] int32 (region_neighbors on the grid the
    working cloud was built on) -> (idx3 [M, 3] int32, w3 [M, 3] f32): per scan point the up to three nearest, by (squared distance, rank), of the
    representatives of its voxel and of the 26 voxels around it, and their inverse-distance weights (common.py:238-255's arithmetic on the grid's
    candidates; include/pointsam_hip.h has the definition).  center / radius: a crop's -- the query coordinate is then the crop's normalised one and
    points with inv == -1 get idx3 = -1, w3 = 0.  No host synchronisation."""
    import numpy as np
    if xyz.dim() == 3 and xyz.shape[0] == 1:
        xyz = xyz[0]
    _chk(xyz, name="xyz"); _chk(inv, torch.int64, "inv"); _chk(wxyz, name="wxyz"); _chk(nbr, torch.int32, "nbr")
    if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] < 1 or inv.dim() != 1 or inv.numel() != xyz.shape[0]:
        raise ValueError(f"scene_interp_plan: xyz must be [M, 3] and inv [M], got {tuple(xyz.shape)} and {tuple(inv.shape)}")
    if wxyz.dim() != 2 or wxyz.shape[1] != 3 or wxyz.shape[0] < 1 or tuple(nbr.shape) != (wxyz.shape[0], 26):
        raise ValueError(f"scene_interp_plan: wxyz must be [Nw, 3] and nbr [Nw, 26], got {tuple(wxyz.shape)} and {tuple(nbr.shape)}")
    if (center is None) != (radius is None):
        raise ValueError("scene_interp_plan: center and radius are a crop's: give both or neither")
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not 0 <= eps < float("inf"):
        raise ValueError(f"scene_interp_plan: eps must be finite and not negative, got {eps!r}")
    org, inv_r = None, 0.0
    if center is not None:
        c = np.asarray([float(v) for v in center], dtype=np.float32) if len(center) == 3 else None
        if c is None or not np.isfinite(c).all():
            raise ValueError(f"scene_interp_plan: center must be three finite fp32 numbers, got {center!r}")
        if isinstance(radius, bool) or not isinstance(radius, (int, float, np.floating)):
            raise ValueError(f"scene_interp_plan: radius must be a number, got {radius!r}")
        r = np.float32(radius)
        with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
            inv_r = np.float32(1) / r                      # fp32, as crop_downsample computes it
        if not (np.isfinite(r) and r > 0 and np.isfinite(inv_r) and inv_r > 0):
            raise ValueError(f"scene_interp_plan: radius must be positive with a finite fp32 inverse, got {radius!r}")
        org = (ctypes.c_float * 3)(*[float(v) for v in c])
    M, Nw, dev = xyz.shape[0], wxyz.shape[0], xyz.device
    idx3 = torch.empty(M, 3, dtype=torch.int32, device=dev)
    w3 = torch.empty(M, 3, dtype=torch.float32, device=dev)
    check(_lib.load().psam_interp_scene_plan(xyz.data_ptr(), M, inv.data_ptr(), wxyz.data_ptr(), nbr.data_ptr(), Nw,
                                             None if org is None else ctypes.addressof(org), float(inv_r), float(eps), idx3.data_ptr(), w3.data_ptr(),
                                             _stream()), "psam_interp_scene_plan")
    return idx3, w3


def _interp_chk(src, idx3, w3, what: str):
    """-> (rows [R, Nw] with unit column stride, src_ld, lead, Nw, M)."""
    _chk(idx3, torch.int32, "idx3"); _chk(w3, name="w3")
    if not src.is_cuda:
        raise _lib.PointSamHipError("src must live on the GPU: the HIP path has no CPU fallback")
    if src.dtype != torch.float32:
        raise TypeError(f"{what}: rows of float32, got {src.dtype}")
    if idx3.dim() != 2 or idx3.shape[1] != 3 or tuple(w3.shape) != tuple(idx3.shape):
        raise ValueError(f"{what}: idx3 and w3 must both be [M, 3], got {tuple(idx3.shape)} and {tuple(w3.shape)}")
    Nw, M = src.shape[-1], idx3.shape[0]
    lead = tuple(src.shape[:-1])
    rows = src.reshape(-1, Nw) if src.dim() != 2 else src
    if rows.stride(1) != 1 and Nw > 1:
        rows = rows.contiguous()
    R = rows.shape[0]
    if R < 1 or Nw < 1 or M < 1:
        raise ValueError(f"{what}: empty input: src {tuple(src.shape)}, idx3 {tuple(idx3.shape)}")
    src_ld = rows.stride(0) if R > 1 else Nw
    if src_ld < Nw:
        rows, src_ld = rows.contiguous(), Nw
    return rows, src_ld, lead, Nw, M


def scene_interp_rows(src: torch.Tensor, idx3: torch.Tensor, w3: torch.Tensor, fill=None, out: torch.Tensor = None) -> torch.Tensor:
    """src [..., Nw] f32 (the leading dimensions are R rows with one stride; last stride 1), a plan (idx3, w3) [M, 3] -> [..., M] f32: per scan point
    the blend w0 l0 + w1 l1 (+ w2 l2) of its sources l_j = src[r, idx3[i, j]]; a point with a single source receives that word bit for bit, an off
    point (a crop's) `fill` (None: 0.0).  An idx3 entry outside [0, Nw) is unused.  out: a [R, M] destination with its own row stride."""
    rows, src_ld, lead, Nw, M = _interp_chk(src, idx3, w3, "scene_interp_rows")
    R = rows.shape[0]
    if out is None:
        dst = torch.empty(R, M, dtype=torch.float32, device=src.device)
    else:
        dst = out
        if dst.dtype != src.dtype or dst.dim() != 2 or tuple(dst.shape) != (R, M) or (M > 1 and dst.stride(1) != 1) or (R > 1 and dst.stride(0) < M):
            raise ValueError(f"scene_interp_rows: out must be [{R}, {M}] {src.dtype} with unit column stride, got {tuple(dst.shape)} {dst.dtype}")
    dst_ld = dst.stride(0) if R > 1 else M
    check(_lib.load().psam_interp_scene_rows(rows.data_ptr(), src_ld, idx3.data_ptr(), w3.data_ptr(), R, Nw, M, 0.0 if fill is None else float(fill),
                                             dst.data_ptr(), dst_ld, _stream()), "psam_interp_scene_rows")
    return dst if out is not None else dst.reshape(lead + (M,))


def scene_interp_bits(src: torch.Tensor, idx3: torch.Tensor, w3: torch.Tensor, thr: float = 0.0, area: bool = True):
    """mask_pack of scene_interp_rows without the [K, M] floats in between: src [..., Nw] f32 (K rows), a plan [M, 3] -> (bits_f [K, ceil(M / 64)] int64,
    area_f [K] int32 or None): bit i = blend > thr (NaN false, an off point 0); bits past M are zero; area_f = the rows' popcounts."""
    rows, src_ld, _, Nw, M = _interp_chk(src, idx3, w3, "scene_interp_bits")
    K = rows.shape[0]
    bits_f = torch.empty(K, mask_words(M), dtype=torch.int64, device=src.device)
    area_f = torch.empty(K, dtype=torch.int32, device=src.device) if area else None
    check(_lib.load().psam_interp_scene_bits(rows.data_ptr(), src_ld, idx3.data_ptr(), w3.data_ptr(), K, Nw, M, float(thr), bits_f.data_ptr(), _p(area_f),
                                             _stream()), "psam_interp_scene_bits")
    return bits_f, area_f


# ------------------------------------------------------------------------------------------ masks carried to another cloud (csrc/transfer.hip)
class TransferIndex:
    """The sources of a radius search, indexed by cells of the radius' size (transfer_index): `ws` is the library's workspace (layout private),
    `src_xyz` [N, 3] the sources it was built from (kept alive: the plan reads them), `radius`, `inv_h` = fl32(1 / radius) and `r2` =
    fl32(radius * radius) fp32 values, `origin` three fp32 values."""
    __slots__ = ("ws", "src_xyz", "radius", "inv_h", "r2", "origin")

    def __init__(self, ws, src_xyz, radius, inv_h, r2, origin):
        self.ws, self.src_xyz, self.radius, self.inv_h, self.r2, self.origin = ws, src_xyz, radius, inv_h, r2, origin

    @property
    def num_source(self) -> int:
        return self.src_xyz.shape[0]


def transfer_radius(radius):
    """-> (r, inv_h, r2) as fp32 values: r = fl32(radius), inv_h = fl32(1 / r), r2 = fl32(r * r).  ValueError unless all three are finite and positive."""
    import numpy as np
    if isinstance(radius, bool) or not isinstance(radius, (int, float, np.floating, np.integer)):
        raise ValueError(f"transfer: radius must be a number, got {radius!r}")
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        r = np.float32(radius)
        inv_h = np.float32(1) / r
        r2 = np.float32(r * r)
    if not (np.isfinite(r) and r > 0 and np.isfinite(inv_h) and inv_h > 0 and np.isfinite(r2) and r2 > 0):
        raise ValueError(f"transfer: radius must be finite and positive with a finite positive fp32 inverse and square, got {radius!r}")
    return r, inv_h, r2


def transfer_pose(pose):
    """A 3 x 4 or 4 x 4 array-like (query frame -> source frame) -> its twelve fp32 words, row-major 3 x 4; None stays None.  ValueError for another
    shape, a value that is not finite, or a 4 x 4 whose last row is not (0, 0, 0, 1)."""
    import numpy as np
    if pose is None:
        return None
    if isinstance(pose, torch.Tensor):
        pose = pose.detach().cpu().numpy()
    try:
        P = np.asarray(pose, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"transfer: pose must be a 3 x 4 or 4 x 4 array of numbers, got {pose!r}") from None
    if P.shape not in ((3, 4), (4, 4)):
        raise ValueError(f"transfer: pose must be 3 x 4 or 4 x 4, got shape {P.shape}")
    words, bad_row, bad_value = _pose_words(P)
    if bad_row:
        raise ValueError(f"transfer: the last row of a 4 x 4 pose must be (0, 0, 0, 1), got {P[3].tolist()}")
    if bad_value:
        raise ValueError("transfer: pose must be finite in fp32")
    return words


def _pose_words(A):
    """[..., 3 or 4, 4] fp64 -> (the fp32 words [..., 12] of the upper 3 x 4; where a fourth row is not (0, 0, 0, 1); where a word is not finite)."""
    import numpy as np
    with np.errstate(over="ignore"):
        words = A[..., :3, :].astype(np.float32).reshape(A.shape[:-2] + (12,))
    bad_row = (A[..., 3, :] != np.array([0.0, 0.0, 0.0, 1.0])).any(-1) if A.shape[-2] == 4 else np.zeros(A.shape[:-2], dtype=bool)
    return words, bad_row, ~np.isfinite(words).all(-1)


def _pose_arg(words):
    """transfer_pose's words (twelve contiguous fp32) -> (their ctypes copy, kept alive by the caller for the call; its address), or (None, None)
    without a pose.  One buffer copy: converting the words one by one cost more than the rest of a step's argument handling."""
    if words is None:
        return None, None
    P = (ctypes.c_float * 12).from_buffer_copy(words)
    return P, ctypes.addressof(P)


def _transfer_query(what: str, index, xyz, radius=None):
    """The checks every user of an index shares, in one order, before any device work: the index, the query cloud, an optional smaller radius
    -> (xyz [M, 3], r2)."""
    if not isinstance(index, TransferIndex):
        raise TypeError(f"{what}: index must be a TransferIndex (ops.transfer_index), got {type(index).__name__}")
    xyz = _transfer_cloud(xyz, f"{what}: xyz")
    r2 = index.r2
    if radius is not None:
        r, _, r2 = transfer_radius(radius)
        if r > index.radius:
            raise ValueError(f"{what}: radius {float(r)} exceeds the index's {float(index.radius)}: the search covers the 27 cells around a query only")
    return xyz, r2


def _transfer_args(index, r2):
    """-> (the origin's ctypes array, kept alive by the caller for the call; the seven leading arguments of the C entries that search an index)."""
    org = (ctypes.c_float * 3)(*index.origin)
    return org, (index.src_xyz.data_ptr(), index.num_source, index.ws.data_ptr(), index.ws.numel() * 8, ctypes.addressof(org), float(index.inv_h), float(r2))


def _transfer_cloud(xyz, what: str):
    if not isinstance(xyz, torch.Tensor):
        raise TypeError(f"{what} must be a tensor, got {type(xyz).__name__}")
    if xyz.dim() == 3 and xyz.shape[0] == 1:
        xyz = xyz[0]
    if xyz.dim() != 2 or xyz.shape[1] != 3 or not 1 <= xyz.shape[0] <= 1 << 28:
        raise ValueError(f"{what} must be [n, 3] with 1 <= n <= 2^28, got {tuple(xyz.shape)}")
    if xyz.dtype != torch.float32:
        raise TypeError(f"{what}: expected {torch.float32}, got {xyz.dtype}")
    return xyz


def transfer_index(src_xyz: torch.Tensor, radius) -> TransferIndex:
    """src_xyz [N, 3] f32, radius -> a TransferIndex for transfer_plan: the sources in cells of size `radius` from origin = fl32(min of the sources per
    axis - radius) (include/pointsam_hip.h: masks carried to another cloud).  One device reduction and one host read (the sources' bounds).
    ValueError for sources that are not finite, a bad radius (transfer_radius), or an extent of 2^21 cells or more on an axis."""
    import numpy as np
    src_xyz = _transfer_cloud(src_xyz, "transfer_index: src_xyz")
    r, inv_h, r2 = transfer_radius(radius)
    lo, hi = torch.aminmax(src_xyz, dim=0)                     # a NaN propagates into both, an infinity into one
    bounds = torch.stack([lo, hi]).cpu().numpy()
    if not np.isfinite(bounds).all():
        raise ValueError("transfer_index: src_xyz must be finite")
    if ((bounds[1].astype(np.float64) - bounds[0].astype(np.float64)) / float(r) + 3 >= float(1 << 21)).any():
        raise ValueError(f"transfer_index: the sources span {bounds[0].tolist()} .. {bounds[1].tolist()}: 2^21 cells of size {float(r)} or more on an axis")
    with np.errstate(over="ignore"):
        origin = (bounds[0] - r).astype(np.float32)
    if not np.isfinite(origin).all():
        raise ValueError("transfer_index: min - radius is not finite in fp32")
    _chk(src_xyz, name="src_xyz")
    N = src_xyz.shape[0]
    L = _lib.load()
    ws = torch.empty(L.psam_transfer_index_workspace_bytes(N) // 8 + 2, dtype=torch.int64, device=src_xyz.device)      # torch allocations are at least 16-byte aligned
    org = (ctypes.c_float * 3)(*[float(v) for v in origin])
    check(L.psam_transfer_index_build(src_xyz.data_ptr(), N, ctypes.addressof(org), float(inv_h), ws.data_ptr(), ws.numel() * 8, _stream()),
          "psam_transfer_index_build")
    return TransferIndex(ws, src_xyz, r, inv_h, r2, tuple(float(v) for v in origin))


def transfer_plan(index: TransferIndex, xyz: torch.Tensor, pose=None, eps: float = 1e-8):
    """index (transfer_index), xyz [M, 3] f32 (the queries), pose (3 x 4 or 4 x 4 array-like, query frame -> source frame, or None) -> (idx3 [M, 3]
    int32, w3 [M, 3] f32) in scene_interp_plan's format: per query the up to three sources nearest to pose(xyz), by (squared distance, index), among
    those within the radius in its own and the 26 surrounding cells; a query without one gets idx3 = -1, w3 = 0.  scene_interp_rows /
    scene_interp_bits apply the plan.  No host synchronisation."""
    xyz, r2 = _transfer_query("transfer_plan", index, xyz)
    words = transfer_pose(pose)
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not 0 < eps < float("inf"):
        raise ValueError(f"transfer_plan: eps must be finite and positive, got {eps!r}")
    _chk(xyz, name="xyz")
    M, dev = xyz.shape[0], xyz.device
    idx3 = torch.empty(M, 3, dtype=torch.int32, device=dev)
    w3 = torch.empty(M, 3, dtype=torch.float32, device=dev)
    org, lead = _transfer_args(index, r2)
    P, pose_ptr = _pose_arg(words)
    check(_lib.load().psam_transfer_plan(*lead, xyz.data_ptr(), M, pose_ptr, float(eps), idx3.data_ptr(), w3.data_ptr(), _stream()), "psam_transfer_plan")
    return idx3, w3


# ------------------------------------------------------------------------------------------ pose between two clouds (csrc/align.hip)
ALIGN_SUMS = 20
PLANE_SUMS = 32      # PSAM_PLANE_SUMS (csrc/align_plane.hip)


def align_step(index: TransferIndex, xyz: torch.Tensor, pose=None, radius=None, bits: torch.Tensor = None, return_nearest: bool = False):
    """One ICP step (include/pointsam_hip.h: pose between two clouds): index (transfer_index), xyz [M, 3] f32 (the queries), pose as for transfer_plan
    -> sums [20] float64 on the device over the pairs (query, nearest source within `radius` of pose(query)): the count, sum q, sum x, sum s,
    sum x s^T, sum |x|^2, sum |s|^2, and the participating queries that have a cell; x is the query as given, not posed.  radius: None (the index's
    own) or a smaller one -- a larger one is a ValueError, the 27 cells would silently truncate the search.  bits: None, or [ceil(M / 64)] int64 words
    in mask_pack's layout: the queries that take part.  return_nearest: also nearest [M] int32, -1 without a pair.  No host synchronisation."""
    xyz, words, r2, bits = _align_arguments("align_step", index, xyz, pose, radius, bits)
    _chk(xyz, name="xyz")
    L = _lib.load()
    return _align_call(L.psam_align_step, L.psam_align_workspace_bytes, "psam_align_step", ALIGN_SUMS, index, xyz, words, r2, bits, return_nearest)


def _align_arguments(what: str, index, xyz, pose, radius, bits):
    """The checks align_step and align_plane_step share, in one order, before any device work: _transfer_query's, the pose and the bits
    -> (xyz [M, 3], the pose's fp32 words or None, r2, bits as one checked row or None)."""
    xyz, r2 = _transfer_query(what, index, xyz, radius)
    words = transfer_pose(pose)
    return xyz, words, r2, _packed_row(what, "bits", bits, xyz.shape[0], "queries")


def _packed_row(what: str, name: str, bits, n: int, of: str):
    """None, or one packed row over n items (mask_pack's layout) -> the row as [ceil(n / 64)] int64 words, checked."""
    if bits is None:
        return None
    if not isinstance(bits, torch.Tensor) or bits.dtype != torch.int64 or bits.dim() == 2 and bits.shape[0] != 1 or bits.dim() not in (1, 2) or \
            bits.shape[-1] != mask_words(n):
        raise ValueError(f"{what}: {name} must be one packed row of {mask_words(n)} int64 words for {n} {of}, got "
                         f"{(bits.dtype, tuple(bits.shape)) if isinstance(bits, torch.Tensor) else type(bits).__name__}")
    bits = bits.reshape(-1)
    _chk(bits, torch.int64, name=name)
    return bits


def _align_call(step, workspace_bytes, name: str, num_sums: int, index, xyz, words, r2, bits, return_nearest: bool, *extra):
    """What the two steps launch alike: the outputs, the workspace and the C entry `step` (`name` for its errors); extra: the device pointers that
    entry takes after src."""
    M, dev = xyz.shape[0], xyz.device
    sums = torch.empty(num_sums, dtype=torch.float64, device=dev)
    nearest = torch.empty(M, dtype=torch.int32, device=dev) if return_nearest else None
    ws = torch.empty(workspace_bytes(M) // 8, dtype=torch.float64, device=dev)
    org, (src, *lead) = _transfer_args(index, r2)
    P, pose_ptr = _pose_arg(words)
    check(step(src, *extra, *lead, xyz.data_ptr(), M, None if bits is None else bits.data_ptr(), pose_ptr, None if nearest is None else nearest.data_ptr(),
               sums.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream()), name)
    return (sums, nearest) if return_nearest else sums


def align_plane_step(index: TransferIndex, xyz: torch.Tensor, normals: torch.Tensor, pose=None, radius=None, bits: torch.Tensor = None,
                     return_nearest: bool = False):
    """One point-to-plane ICP step (include/pointsam_hip.h: pose between two clouds): align_step's arguments and pairs, plus normals [N, 3] f32 on the
    index's device, one per indexed source (voxel_normals' fit; taken as given, either sign) -> sums [32] float64 on the device over the USED pairs
    -- those whose normal has a finite, positive squared length: [0] their number, [1] sum q, [2] sum r r, [3..8] sum J r, [9..29] the upper triangle
    of sum J J^T row-major, [30] the paired queries whose pair was not used, [31] the participating queries that have a cell; r = (p - s) . n and
    J = (p x n, n) with p the POSED query.  align.solve_plane turns them into the next pose.  return_nearest: also nearest [M] int32, align_step's.
    No host synchronisation."""
    xyz, words, r2, bits = _align_arguments("align_plane_step", index, xyz, pose, radius, bits)
    if not isinstance(normals, torch.Tensor):
        raise TypeError(f"align_plane_step: normals must be a tensor, got {type(normals).__name__}")
    if normals.dim() != 2 or tuple(normals.shape) != (index.num_source, 3):
        raise ValueError(f"align_plane_step: normals must be [{index.num_source}, 3], one per indexed source, got {tuple(normals.shape)}")
    if normals.dtype != torch.float32:
        raise TypeError(f"align_plane_step: normals: expected {torch.float32}, got {normals.dtype}")
    if normals.device != index.src_xyz.device:
        raise ValueError(f"align_plane_step: normals are on {normals.device}, the index on {index.src_xyz.device}")
    _chk(xyz, name="xyz")
    _chk(normals, name="normals")
    L = _lib.load()
    return _align_call(L.psam_plane_step, L.psam_plane_workspace_bytes, "psam_plane_step", PLANE_SUMS, index, xyz, words, r2, bits, return_nearest,
                       normals.data_ptr())


ALIGN_SCORE_POSES = 4            # PSAM_ALIGN_SCORE_POSES: the poses one workgroup of psam_pose_score takes a tile of queries through
ALIGN_SCORE_MAX_POSES = 1 << 20


def transfer_poses(poses):
    """[P, 3, 4] or [P, 4, 4] array-like of host numbers -> [P, 12] fp32 words: every row as transfer_pose gives it, and transfer_pose's ValueError for
    the first row it refuses (a value that is not finite in fp32, a 4 x 4 whose last row is not (0, 0, 0, 1))."""
    import numpy as np
    if isinstance(poses, torch.Tensor):
        poses = poses.detach().cpu().numpy()
    try:
        A = np.asarray(poses, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("align_score: poses must be a [P, 3, 4] or [P, 4, 4] array of numbers") from None
    if A.ndim != 3 or A.shape[1:] not in ((3, 4), (4, 4)) or not 1 <= A.shape[0] <= ALIGN_SCORE_MAX_POSES:
        raise ValueError(f"align_score: poses must be [P, 3, 4] or [P, 4, 4] with 1 <= P <= 2^20, got shape {A.shape}")
    words, bad_row, bad_value = _pose_words(A)
    bad = bad_row | bad_value
    if bad.any():
        transfer_pose(A[int(np.argmax(bad))])                 # the first bad row, in transfer_pose's own words
        raise ValueError(f"align_score: pose {int(np.argmax(bad))} is not a rigid pose")
    return np.ascontiguousarray(words)


def align_score(index: TransferIndex, xyz: torch.Tensor, poses, radius=None):
    """The score of a pose search (include/pointsam_hip.h: pose between two clouds): index (transfer_index), xyz [M, 3] f32 (the queries), poses
    -> counts [P] int32 on the device: under pose p, the queries with at least one indexed source within `radius` of pose_p(query) -- exactly
    int(align_step(index, xyz, pose_p, radius)[0]) for every p, from ONE launch.  poses: [P, 3, 4] or [P, 4, 4] host numbers (an array-like or a
    tensor), every row checked as transfer_pose checks a pose (ValueError for a value that is not finite or a bad last row); or a [P, 12] float32
    tensor ON THE DEVICE, the rows' twelve words, which is taken AS VALIDATED -- the kernel cannot refuse a pose, one that is not finite scores 0.
    radius: None (the index's own) or a smaller one, a larger one is a ValueError as for align_step.  1 <= P <= 2^20.  No host synchronisation."""
    xyz, r2 = _transfer_query("align_score", index, xyz, radius)
    M, dev = xyz.shape[0], xyz.device
    if isinstance(poses, torch.Tensor) and poses.is_cuda and poses.dim() == 2:
        if poses.shape[1] != 12 or not 1 <= poses.shape[0] <= ALIGN_SCORE_MAX_POSES:
            raise ValueError(f"align_score: device poses must be [P, 12] with 1 <= P <= 2^20, got {tuple(poses.shape)}")
        words = _chk(poses, name="poses")
        _chk(xyz, name="xyz")
    else:
        host = transfer_poses(poses)
        _chk(xyz, name="xyz")
        words = torch.from_numpy(host).to(dev)
    P = words.shape[0]
    counts = torch.empty(P, dtype=torch.int32, device=dev)
    org, lead = _transfer_args(index, r2)
    check(_lib.load().psam_pose_score(*lead, xyz.data_ptr(), M, words.data_ptr(), P, counts.data_ptr(), _stream()), "psam_pose_score")
    return counts


# ------------------------------------------------------------------------------------------ camera views (csrc/views.hip)
VIEW_MAX_SIDE, VIEW_MAX_SPLAT, VIEW_MAX_WINDOW = 8192, 3, 16


def _view_int(value, lo: int, hi: int, what: str) -> int:
    if isinstance(value, bool) or not isinstance(value, int) or not lo <= value <= hi:
        raise ValueError(f"{what} must be an integer in {lo} .. {hi}, got {value!r}")
    return value


def _view_camera(camera, what: str):
    """-> (the pose's ctypes words, kept alive by the caller for the call; the nine camera arguments of the C entry points).  camera: a views.Camera, or
    anything with its attributes (pose_words: twelve fp32 words, fx, fy, cx, cy, width, height, near)."""
    try:
        words = [float(v) for v in camera.pose_words]
        args = (float(camera.fx), float(camera.fy), float(camera.cx), float(camera.cy), int(camera.width), int(camera.height), float(camera.near))
    except (AttributeError, TypeError):
        raise TypeError(f"{what}: camera must be a views.Camera, got {type(camera).__name__}") from None
    if len(words) != 12:
        raise ValueError(f"{what}: the camera's pose must have twelve words, got {len(words)}")
    P = (ctypes.c_float * 12)(*words)
    return P, (ctypes.addressof(P),) + args


def _view_keys(keys, what: str):
    """The shape of a view's keys; whether they live on the GPU is the caller's last check (_chk), after every check of a value."""
    if not isinstance(keys, torch.Tensor) or keys.dtype != torch.int64:
        raise TypeError(f"{what}: keys must be an int64 tensor (view_splat), got {getattr(keys, 'dtype', type(keys).__name__)}")
    if keys.dim() != 2 or not (1 <= keys.shape[0] <= VIEW_MAX_SIDE and 1 <= keys.shape[1] <= VIEW_MAX_SIDE):
        raise ValueError(f"{what}: keys must be [height, width] with sides in 1 .. {VIEW_MAX_SIDE}, got {tuple(keys.shape)}")
    return keys.shape[0], keys.shape[1]


def _view_tau(tau, what: str) -> float:
    import math
    if isinstance(tau, bool) or not isinstance(tau, (int, float)) or math.isnan(tau) or tau < 0:
        raise ValueError(f"{what}: tau must be a number >= 0, got {tau!r}")
    return float(tau)


def _view_bits(keys, bits, N: int, what: str):
    H, W = _view_keys(keys, what)
    if not isinstance(bits, torch.Tensor) or bits.dtype != torch.int64:
        raise TypeError(f"{what}: bits must be an int64 tensor, got {getattr(bits, 'dtype', type(bits).__name__)}")
    if isinstance(N, bool) or not isinstance(N, int) or not 1 <= N <= 1 << 28:
        raise ValueError(f"{what}: N must be an integer in 1 .. 2^28, got {N!r}")
    if bits.dim() != 2 or bits.shape[0] < 1 or bits.shape[1] != mask_words(N):
        raise ValueError(f"{what}: bits {tuple(bits.shape)} for N = {N}: need [K >= 1, {mask_words(N)}]")
    if bits.device != keys.device:
        raise ValueError(f"{what}: keys are on {keys.device}, bits on {bits.device}")
    _chk(keys, torch.int64, "keys"); _chk(bits, torch.int64, "bits")
    return H, W, bits.shape[0]


def view_splat(xyz: torch.Tensor, camera, splat: int = 1) -> torch.Tensor:
    """xyz [N, 3] (or [1, N, 3]) f32, camera (views.Camera), footprint `splat` in 0 .. 3 -> keys [height, width] int64 words: per pixel the minimum
    (bits(depth) << 32) | index over the in-view points whose pixel lies within `splat` of it on both axes, all ones (-1) where there is none
    (include/pointsam_hip.h: camera views).  Exact and independent of the order the points arrive in.  No host synchronisation."""
    xyz = _transfer_cloud(xyz, "view_splat: xyz")
    s = _view_int(splat, 0, VIEW_MAX_SPLAT, "view_splat: splat")
    P, cam = _view_camera(camera, "view_splat")
    _chk(xyz, name="xyz")
    keys = torch.empty(cam[6], cam[5], dtype=torch.int64, device=xyz.device)
    check(_lib.load().psam_view_splat(xyz.data_ptr(), xyz.shape[0], *cam, s, keys.data_ptr(), _stream()), "psam_view_splat")
    return keys


def view_pick(keys: torch.Tensor, pixels: torch.Tensor, window: int = 2) -> torch.Tensor:
    """keys [H, W] int64 (view_splat), pixels [P, 2] int32 (x, y) -> point_index [P] int32: the point of the non-empty pixel nearest to each click within
    `window` (0 .. 16) pixels on both axes, by (squared pixel distance, key); -1 where the window is empty.  No host synchronisation."""
    H, W = _view_keys(keys, "view_pick")
    w = _view_int(window, 0, VIEW_MAX_WINDOW, "view_pick: window")
    if not isinstance(pixels, torch.Tensor) or pixels.dim() != 2 or pixels.shape[1] != 2 or pixels.shape[0] < 1:
        raise ValueError(f"view_pick: pixels must be a tensor [P, 2] with P >= 1, got {tuple(getattr(pixels, 'shape', ()))}")
    _chk(keys, torch.int64, "keys"); _chk(pixels, torch.int32, "pixels")
    out = torch.empty(pixels.shape[0], dtype=torch.int32, device=keys.device)
    check(_lib.load().psam_view_pick(keys.data_ptr(), W, H, pixels.data_ptr(), pixels.shape[0], w, out.data_ptr(), _stream()), "psam_view_pick")
    return out


def view_paint_ids(keys: torch.Tensor, bits: torch.Tensor, N: int) -> torch.Tensor:
    """keys [H, W] int64 (view_splat of a cloud of N points), bits [K, ceil(N / 64)] int64 words (mask_pack's layout) -> ids [H, W] int32: the lowest
    row whose bit for the pixel's point is set, -1 where none is or the pixel is empty.  No host synchronisation."""
    H, W, K = _view_bits(keys, bits, N, "view_paint_ids")
    ids = torch.empty(H, W, dtype=torch.int32, device=keys.device)
    check(_lib.load().psam_view_paint_ids(keys.data_ptr(), W, H, bits.data_ptr(), K, N, ids.data_ptr(), _stream()), "psam_view_paint_ids")
    return ids


def view_paint_rows(keys: torch.Tensor, bits: torch.Tensor, N: int) -> torch.Tensor:
    """As view_paint_ids -> rows [K, H, W] uint8: row k's bit of every pixel's point, 0 at an empty pixel."""
    H, W, K = _view_bits(keys, bits, N, "view_paint_rows")
    rows = torch.empty(K, H, W, dtype=torch.uint8, device=keys.device)
    check(_lib.load().psam_view_paint_rows(keys.data_ptr(), W, H, bits.data_ptr(), K, N, rows.data_ptr(), _stream()), "psam_view_paint_rows")
    return rows


def view_lift_bits(xyz: torch.Tensor, camera, keys: torch.Tensor, images: torch.Tensor = None, tau: float = 0.0):
    """xyz [N, 3] f32, camera, keys [H, W] (view_splat of the same points and camera), images [K, H, W] uint8 or None, tau >= 0 ->
    (bits [K, ceil(N / 64)] int64 words of mask_pack's layout, area [K] int32): point i has bit k iff it is in view, its depth is at most its centre
    pixel's winning depth + tau, and images[k] is non-zero at that pixel.  images None: K = 1, every pixel set -- the points visible in the view.
    No host synchronisation."""
    xyz = _transfer_cloud(xyz, "view_lift_bits: xyz")
    H, W = _view_keys(keys, "view_lift_bits")
    P, cam = _view_camera(camera, "view_lift_bits")
    if (cam[6], cam[5]) != (H, W):
        raise ValueError(f"view_lift_bits: keys {tuple(keys.shape)} are not the camera's {cam[6]} x {cam[5]} (height x width)")
    tau = _view_tau(tau, "view_lift_bits")
    K = 1
    if images is not None:
        if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8:
            raise TypeError(f"view_lift_bits: images must be a uint8 tensor, got {getattr(images, 'dtype', type(images).__name__)}")
        if images.dim() != 3 or images.shape[0] < 1 or tuple(images.shape[1:]) != (H, W):
            raise ValueError(f"view_lift_bits: images must be [K >= 1, {H}, {W}], got {tuple(images.shape)}")
        K = images.shape[0]
        _chk(images, torch.uint8, "images")
    _chk(xyz, name="xyz"); _chk(keys, torch.int64, "keys")
    N = xyz.shape[0]
    bits = torch.empty(K, mask_words(N), dtype=torch.int64, device=xyz.device)
    area = torch.empty(K, dtype=torch.int32, device=xyz.device)
    check(_lib.load().psam_view_lift_bits(xyz.data_ptr(), N, *cam, keys.data_ptr(), _p(images), K, float(tau), bits.data_ptr(), area.data_ptr(), _stream()),
          "psam_view_lift_bits")
    return bits, area


# ------------------------------------------------------------------------------------------ RGB-D frames (csrc/frames.hip)
FRAME_MAX_PIXELS = 1 << 28


def _frame_number(value, what: str, allow_none: bool = False):
    """A finite positive number that stays finite and positive in fp32 -> that fp32 value as a float (None stays None where allowed)."""
    import numpy as np
    if value is None and allow_none:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float, np.floating, np.integer)):
        raise ValueError(f"{what} must be a number, got {value!r}")
    with np.errstate(over="ignore"):
        v = np.float32(value)
    if not (np.isfinite(v) and v > 0):
        raise ValueError(f"{what} must be finite and positive in fp32, got {value!r}")
    return float(v)


def _frame_cameras(cameras, F: int, H: int, W: int, what: str):
    """-> [(twelve pose words, fx, fy, cx, cy, near)] per frame, from views.Camera objects (or anything with their attributes) of the frames' size."""
    if not isinstance(cameras, (list, tuple)) or len(cameras) != F:
        raise ValueError(f"{what}: cameras must be a list of {F} views.Camera, one per frame, got {type(cameras).__name__}"
                         + (f" of {len(cameras)}" if isinstance(cameras, (list, tuple)) else ""))
    rows = []
    for f, cam in enumerate(cameras):
        try:
            words = [float(v) for v in cam.pose_words]
            row = words + [float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy), float(cam.near)]
            size = (int(cam.height), int(cam.width))
        except (AttributeError, TypeError):
            raise TypeError(f"{what}: cameras[{f}] must be a views.Camera, got {type(cam).__name__}") from None
        if len(words) != 12:
            raise ValueError(f"{what}: the pose of cameras[{f}] must have twelve words, got {len(words)}")
        if size != (H, W):
            raise ValueError(f"{what}: cameras[{f}] is {size[0]} x {size[1]} (height x width), the frames are {H} x {W}")
        rows.append(row)
    return rows


def _frame_shape(t, what: str):
    if t.dim() != 3 or t.shape[0] < 1 or not (1 <= t.shape[1] <= VIEW_MAX_SIDE and 1 <= t.shape[2] <= VIEW_MAX_SIDE) or t.numel() > FRAME_MAX_PIXELS:
        raise ValueError(f"{what} must be [F >= 1, height, width] with sides in 1 .. {VIEW_MAX_SIDE} and at most 2^28 pixels, got {tuple(t.shape)}")
    return tuple(t.shape)


def frames_unproject(depth: torch.Tensor, rgb: torch.Tensor, cameras, far, edge=None, depth_scale=None):
    """depth [F, H, W] f32, or uint16 with a `depth_scale`; rgb [F, H, W, 3] uint8 (0 .. 255), or f32 already in the trained convention; cameras: F
    views.Camera (pose world -> camera, width x height = W x H); far > every camera's near; edge None or > 0 -> (xyz_world [M, 3] f32, rgb [M, 3] f32,
    index [F, H, W] int32, M): the pixels with near <= depth <= far that the edge filter leaves (a pixel goes if a valid 4-neighbour differs by more
    than edge * its own depth), unprojected into the world frame, in ascending (f, y, x); index = a kept pixel's place in that order, -1 elsewhere
    (include/pointsam_hip.h: RGB-D frames).  Exact and run-to-run identical.  The outputs are allocated for F H W points and narrowed; reading M is
    the call's one host read.  ValueError if no pixel is kept."""
    if not isinstance(depth, torch.Tensor) or depth.dtype not in (torch.float32, torch.uint16):
        raise TypeError(f"frames_unproject: depth must be a float32 or uint16 tensor, got {getattr(depth, 'dtype', type(depth).__name__)}")
    F, H, W = _frame_shape(depth, "frames_unproject: depth")
    if not isinstance(rgb, torch.Tensor) or rgb.dtype not in (torch.float32, torch.uint8):
        raise TypeError(f"frames_unproject: rgb must be a uint8 or float32 tensor, got {getattr(rgb, 'dtype', type(rgb).__name__)}")
    if tuple(rgb.shape) != (F, H, W, 3):
        raise ValueError(f"frames_unproject: rgb must be [{F}, {H}, {W}, 3] for this depth, got {tuple(rgb.shape)}")
    u16 = depth.dtype == torch.uint16
    if u16 == (depth_scale is None):
        raise ValueError("frames_unproject: uint16 depth needs a depth_scale, float32 depth takes none" + f", got {depth.dtype} and depth_scale = {depth_scale!r}")
    scale = _frame_number(depth_scale, "frames_unproject: depth_scale", allow_none=True)
    zfar = _frame_number(far, "frames_unproject: far")
    e = _frame_number(edge, "frames_unproject: edge", allow_none=True)
    rows = _frame_cameras(cameras, F, H, W, "frames_unproject")
    for f, row in enumerate(rows):
        if not zfar > row[16]:
            raise ValueError(f"frames_unproject: far = {zfar} must be larger than the near = {row[16]} of cameras[{f}]")
    if rgb.device != depth.device:
        raise ValueError(f"frames_unproject: depth is on {depth.device}, rgb on {rgb.device}")
    _chk(depth, depth.dtype, "depth"); _chk(rgb, rgb.dtype, "rgb")
    dev, total = depth.device, F * H * W
    table = torch.tensor([row + [zfar] for row in rows], dtype=torch.float32).to(dev)          # [F, 18]
    xyz = torch.empty(total, 3, dtype=torch.float32, device=dev)
    col = torch.empty(total, 3, dtype=torch.float32, device=dev)
    index = torch.empty(F, H, W, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    L = _lib.load()
    ws = torch.empty(L.psam_frames_workspace_bytes(F, H, W) // 8 + 2, dtype=torch.int64, device=dev)      # torch allocations are at least 16-byte aligned
    check(L.psam_frames_unproject(depth.data_ptr(), int(u16), 0.0 if scale is None else scale, rgb.data_ptr(), int(rgb.dtype == torch.uint8), table.data_ptr(),
                                  F, H, W, 0.0 if e is None else e, xyz.data_ptr(), col.data_ptr(), index.data_ptr(), count.data_ptr(), ws.data_ptr(),
                                  ws.numel() * 8, _stream()), "psam_frames_unproject")
    M = int(count.item())                                      # the one host read
    if M == 0:
        raise ValueError(f"frames_unproject: no pixel of the {F} frames has a depth in [near, {zfar}]" + ("" if e is None else " that the edge filter keeps"))
    return xyz[:M], col[:M], index, M


def frames_finish(xyz_world: torch.Tensor, index: torch.Tensor, cameras, center, scale):
    """xyz_world [M, 3] f32 and index [F, H, W] int32 of frames_unproject, its cameras, center (three numbers) and scale > 0 -> (xyz [M, 3]: the SAME
    tensor, normalised in place to (p - center) / scale; keys [F, H, W] int64 words: (bits(depth) << 32) | index per kept pixel, the depth its own
    point's in the frame's normalised camera, all ones (-1) elsewhere; the normalised cameras: pose [R | (R center + t) / scale] and near / scale,
    computed in fp64 and rounded once, intrinsics unchanged).  keys[f] with cameras[f] is a view of the scan for view_pick, the paints and
    view_lift_bits, where a pixel's own point is visible at tau = 0.  No host synchronisation."""
    import numpy as np
    from .views import Camera
    xyz = _transfer_cloud(xyz_world, "frames_finish: xyz_world")
    if xyz.dim() != xyz_world.dim():
        raise ValueError(f"frames_finish: xyz_world must be [M, 3] (it is normalised in place), got {tuple(xyz_world.shape)}")
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int32:
        raise TypeError(f"frames_finish: index must be an int32 tensor (frames_unproject), got {getattr(index, 'dtype', type(index).__name__)}")
    F, H, W = _frame_shape(index, "frames_finish: index")
    M = xyz.shape[0]
    if M > F * H * W:
        raise ValueError(f"frames_finish: {M} points cannot come from {F} x {H} x {W} pixels")
    rows = _frame_cameras(cameras, F, H, W, "frames_finish")
    try:
        m = np.asarray(center.detach().cpu().numpy() if isinstance(center, torch.Tensor) else center, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"frames_finish: center must be three numbers, got {center!r}") from None
    with np.errstate(over="ignore"):
        m32 = m.astype(np.float32)
    if m32.shape != (3,) or not np.isfinite(m32).all():
        raise ValueError(f"frames_finish: center must be three numbers that are finite in fp32, got {center!r}")
    if isinstance(scale, torch.Tensor) and scale.numel() == 1:
        scale = float(scale)
    s = _frame_number(scale, "frames_finish: scale")
    # the normalised cameras, all frames at once: [R | (R m + t) / s] and near / s in fp64, rounded to fp32 once
    md = m32.astype(np.float64)
    cam64 = np.asarray(rows, dtype=np.float64)                                                  # [F, 17]
    P = cam64[:, :12].reshape(F, 3, 4).copy()
    P[:, :, 3] = (((P[:, :, 0] * md[0] + P[:, :, 1] * md[1]) + P[:, :, 2] * md[2]) + P[:, :, 3]) / s
    with np.errstate(over="ignore"):
        poses, near = P.reshape(F, 12).astype(np.float32), (cam64[:, 16] / s).astype(np.float32)
    bad = ~(np.isfinite(poses).all(1) & np.isfinite(near) & (near > 0))
    if bad.any():
        f = int(np.nonzero(bad)[0][0])
        raise ValueError(f"frames_finish: cameras[{f}] has no fp32 form in the normalised frame (pose {poses[f].tolist()}, near {float(near[f])})")
    normalised = [Camera.from_fp32(poses[f].copy(), row[12], row[13], row[14], row[15], W, H, float(near[f])) for f, row in enumerate(rows)]
    if index.device != xyz.device:
        raise ValueError(f"frames_finish: xyz_world is on {xyz.device}, index on {index.device}")
    _chk(xyz, name="xyz_world"); _chk(index, torch.int32, "index")
    table = torch.from_numpy(poses).to(xyz.device)                                              # [F, 12]
    keys = torch.empty(F, H, W, dtype=torch.int64, device=xyz.device)
    c = (ctypes.c_float * 3)(*[float(v) for v in m32])
    check(_lib.load().psam_frames_finish(xyz.data_ptr(), M, index.data_ptr(), table.data_ptr(), F, H, W, ctypes.addressof(c), s, keys.data_ptr(), _stream()),
          "psam_frames_finish")
    return xyz, keys, normalised


# ------------------------------------------------------------------------------------------ label fusion (csrc/fusion.hip)
FUSE_MAX_VIEWS, FUSE_MAX_ROWS = 4096, 1 << 20


def _fuse_views(cameras, keys, labels, what: str):
    """The views of a fusion call: keys [V, H, W] int64, labels [V, H, W] int32, V cameras of that size -> (V, H, W, the camera rows [V, 17] as a host
    fp32 array: 12 pose words, fx, fy, cx, cy, near).  Whether the tensors live on the GPU is the caller's last check (_chk)."""
    import numpy as np
    if not isinstance(keys, torch.Tensor) or keys.dtype != torch.int64:
        raise TypeError(f"{what}: keys must be an int64 tensor (frames_finish, or stacked view_splat), got {getattr(keys, 'dtype', type(keys).__name__)}")
    if keys.dim() != 3 or not (1 <= keys.shape[0] <= FUSE_MAX_VIEWS and 1 <= keys.shape[1] <= VIEW_MAX_SIDE and 1 <= keys.shape[2] <= VIEW_MAX_SIDE):
        raise ValueError(f"{what}: keys must be [V, height, width] with V in 1 .. {FUSE_MAX_VIEWS} and sides in 1 .. {VIEW_MAX_SIDE}, got {tuple(keys.shape)}")
    V, H, W = keys.shape
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int32:
        raise TypeError(f"{what}: labels must be an int32 tensor, got {getattr(labels, 'dtype', type(labels).__name__)}")
    if tuple(labels.shape) != (V, H, W):
        raise ValueError(f"{what}: labels must be [{V}, {H}, {W}] like the keys, got {tuple(labels.shape)}")
    rows = np.asarray(_frame_cameras(cameras, V, H, W, what), dtype=np.float64)
    with np.errstate(over="ignore"):
        table = rows.astype(np.float32)
    bad = ~(np.isfinite(table).all(1) & (table[:, 12] > 0) & (table[:, 13] > 0) & (table[:, 16] > 0))
    if bad.any():
        v = int(np.nonzero(bad)[0][0])
        raise ValueError(f"{what}: cameras[{v}] must be finite in fp32 with fx, fy and near positive, got {rows[v].tolist()}")
    if labels.device != keys.device:
        raise ValueError(f"{what}: keys are on {keys.device}, labels on {labels.device}")
    return V, H, W, table


def _fuse_row_base(row_base, V: int, what: str):
    """row_base: V + 1 integers on the host (a list, an array or a CPU tensor), the exclusive prefix of the views' region counts -> (int32 array, R)."""
    import numpy as np
    try:
        rb = np.asarray(row_base.detach().cpu().numpy() if isinstance(row_base, torch.Tensor) else row_base)
    except (TypeError, ValueError):
        rb = None
    if rb is None or rb.dtype.kind not in "iu" or rb.shape != (V + 1,):
        raise ValueError(f"{what}: row_base must be {V + 1} integers, the exclusive prefix of the {V} views' region counts, got {row_base!r}")
    rb = rb.astype(np.int64)
    if rb[0] != 0 or (np.diff(rb) < 0).any():
        raise ValueError(f"{what}: row_base must start at 0 and never decrease, got {rb.tolist()}")
    if rb[-1] > FUSE_MAX_ROWS:
        raise ValueError(f"{what}: row_base ends at {int(rb[-1])} region rows, more than the {FUSE_MAX_ROWS} a call takes")
    return rb.astype(np.int32), int(rb[-1])


def fuse_region_bits(xyz: torch.Tensor, cameras, keys: torch.Tensor, labels: torch.Tensor, row_base, tau: float):
    """xyz [N, 3] f32; V cameras with keys [V, H, W] int64 (the FrameSet's, or view_splat's of equal size stacked) and labels [V, H, W] int32; row_base:
    V + 1 host integers, the exclusive prefix of the views' region counts, R = row_base[V]; tau >= 0 -> (bits [R + V, ceil(N / 64)] int64 words of
    mask_pack's layout, area [R + V] int32).  Row row_base[v] + l holds the points visible in view v -- view_lift_bits' rule -- whose centre pixel carries
    the label l in [0, count_v); row R + v the points visible in view v at all (include/pointsam_hip.h: label fusion).  No host synchronisation."""
    xyz = _transfer_cloud(xyz, "fuse_region_bits: xyz")
    V, H, W, table = _fuse_views(cameras, keys, labels, "fuse_region_bits")
    rb, R = _fuse_row_base(row_base, V, "fuse_region_bits")
    t = _view_tau(tau, "fuse_region_bits")
    _chk(xyz, name="xyz"); _chk(keys, torch.int64, "keys"); _chk(labels, torch.int32, "labels")
    dev, N = xyz.device, xyz.shape[0]
    cam, base = torch.from_numpy(table).to(dev), torch.from_numpy(rb).to(dev)
    bits = torch.empty(R + V, mask_words(N), dtype=torch.int64, device=dev)
    area = torch.empty(R + V, dtype=torch.int32, device=dev)
    check(_lib.load().psam_fuse_region_bits(xyz.data_ptr(), N, cam.data_ptr(), V, H, W, keys.data_ptr(), labels.data_ptr(), base.data_ptr(), R, t,
                                            bits.data_ptr(), area.data_ptr(), _stream()), "psam_fuse_region_bits")
    return bits, area


def fuse_vote(xyz: torch.Tensor, cameras, keys: torch.Tensor, labels: torch.Tensor, tau: float, row_base=None, remap: torch.Tensor = None,
              min_votes: int = 1):
    """The inputs of fuse_region_bits; row_base None: every label >= 0 is a global id; with row_base, a label is valid in [0, count_v) and its global id is
    remap[row_base[v] + l] (remap [R] int32 on the device, an entry below 0 = no label), or l itself without a remap -> (label, votes, seen, labelled,
    dropped), [N] int32 each: per point the winner among the at most 8 distinct global labels its visible observations carry in ascending view order
    (ties: the lower label; -1 below min_votes), the winner's count, and the numbers of visible, labelled and dropped observations.  No host
    synchronisation."""
    xyz = _transfer_cloud(xyz, "fuse_vote: xyz")
    V, H, W, table = _fuse_views(cameras, keys, labels, "fuse_vote")
    rb, R = (None, 0) if row_base is None else _fuse_row_base(row_base, V, "fuse_vote")
    t = _view_tau(tau, "fuse_vote")
    if isinstance(min_votes, bool) or not isinstance(min_votes, int) or not 1 <= min_votes <= FUSE_MAX_VIEWS:
        raise ValueError(f"fuse_vote: min_votes must be an integer in 1 .. {FUSE_MAX_VIEWS}, got {min_votes!r}")
    if remap is not None:
        if rb is None:
            raise ValueError("fuse_vote: a remap needs the row_base that addresses it")
        if not isinstance(remap, torch.Tensor) or remap.dtype != torch.int32:
            raise TypeError(f"fuse_vote: remap must be an int32 tensor, got {getattr(remap, 'dtype', type(remap).__name__)}")
        if tuple(remap.shape) != (R,):
            raise ValueError(f"fuse_vote: remap must be [{R}], one entry per region row, got {tuple(remap.shape)}")
        if remap.device != keys.device:
            raise ValueError(f"fuse_vote: keys are on {keys.device}, remap on {remap.device}")
        if R == 0:
            remap = None                                           # nothing to address
        else:
            _chk(remap, torch.int32, "remap")
    _chk(xyz, name="xyz"); _chk(keys, torch.int64, "keys"); _chk(labels, torch.int32, "labels")
    dev, N = xyz.device, xyz.shape[0]
    cam = torch.from_numpy(table).to(dev)
    base = None if rb is None else torch.from_numpy(rb).to(dev)
    out = torch.empty(5, N, dtype=torch.int32, device=dev)
    check(_lib.load().psam_fuse_vote(xyz.data_ptr(), N, cam.data_ptr(), V, H, W, keys.data_ptr(), labels.data_ptr(), _p(base), _p(remap), R, t, min_votes,
                                     *(out[j].data_ptr() for j in range(5)), _stream()), "psam_fuse_vote")
    return tuple(out[j] for j in range(5))


def label_bits(labels: torch.Tensor, K: int):
    """labels [N] int32, K in 1 .. 2^20 -> (bits [K, ceil(N / 64)] int64 words of mask_pack's layout, area [K] int32): row k holds the points labelled
    k; a label outside [0, K) sets nothing.  No host synchronisation."""
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int32:
        raise TypeError(f"label_bits: labels must be an int32 tensor, got {getattr(labels, 'dtype', type(labels).__name__)}")
    if labels.dim() != 1 or not 1 <= labels.shape[0] <= 1 << 28:
        raise ValueError(f"label_bits: labels must be [N] with N in 1 .. 2^28, got {tuple(labels.shape)}")
    K = _view_int(K, 1, FUSE_MAX_ROWS, "label_bits: K")
    _chk(labels, torch.int32, "labels")
    N = labels.shape[0]
    bits = torch.empty(K, mask_words(N), dtype=torch.int64, device=labels.device)
    area = torch.empty(K, dtype=torch.int32, device=labels.device)
    check(_lib.load().psam_label_bits(labels.data_ptr(), N, K, bits.data_ptr(), area.data_ptr(), _stream()), "psam_label_bits")
    return bits, area


# ------------------------------------------------------------------------------------------ connected components of masks (csrc/regions.hip)
def _region_ws(nbytes: int, dev, what: str):
    if nbytes == 0:
        raise ValueError(f"{what}: the shape is outside what the kernels are built for (K <= 65535 rows per call, N, V <= 2^28)")
    return torch.empty(nbytes // 8 + 2, dtype=torch.int64, device=dev)      # torch allocations are at least 16-byte aligned


def _region_graph_chk(inv, nbr, what: str):
    _chk(inv, torch.int64, "inv"); _chk(nbr, torch.int32, "nbr")
    if inv.dim() != 1 or nbr.dim() != 2 or nbr.shape[1] != 26 or nbr.shape[0] < 1 or inv.numel() < 1:
        raise ValueError(f"{what}: inv must be [N] and nbr [V, 26], got {tuple(inv.shape)} and {tuple(nbr.shape)}")
    return inv.numel(), nbr.shape[0]


def region_neighbors(xyz: torch.Tensor, keep_idx: torch.Tensor, voxel_size: float, origin=(-1.0, -1.0, -1.0)) -> torch.Tensor:
    """xyz [N, 3] f32, keep_idx [V] int64 (voxel_downsample's, at the same voxel_size and origin) -> nbr [V, 26] int32: the rank of the occupied voxel
    at voxel v's cell + offset o, or -1; offsets over (dz, dy, dx) in {-1, 0, 1}^3, dz slowest, the centre skipped (offset 25 - o is the opposite of
    o).  No host synchronisation."""
    import numpy as np
    if xyz.dim() == 3 and xyz.shape[0] == 1:
        xyz = xyz[0]
    _chk(xyz, name="xyz"); _chk(keep_idx, torch.int64, "keep_idx")
    if xyz.dim() != 2 or xyz.shape[1] != 3 or keep_idx.dim() != 1 or not 1 <= keep_idx.numel() <= xyz.shape[0]:
        raise ValueError(f"region_neighbors: xyz must be [N, 3] and keep_idx [V] with 1 <= V <= N, got {tuple(xyz.shape)} and {tuple(keep_idx.shape)}")
    h = np.float32(voxel_size)
    inv_h = np.float32(1) / h if np.isfinite(h) and h > 0 else np.float32("nan")      # fp32, as the header defines it
    if not (np.isfinite(inv_h) and inv_h > 0):
        raise ValueError(f"region_neighbors: voxel_size must be finite and positive with a positive fp32 inverse, got {voxel_size!r}")
    org = (ctypes.c_float * 3)(*[float(v) for v in origin])
    V = keep_idx.numel()
    L = _lib.load()
    nbytes = L.psam_region_neighbors_workspace_bytes(V)
    ws = _region_ws(nbytes, xyz.device, "region_neighbors")
    nbr = torch.empty(V, 26, dtype=torch.int32, device=xyz.device)
    check(L.psam_region_neighbors(xyz.data_ptr(), keep_idx.data_ptr(), V, ctypes.addressof(org), float(inv_h), nbr.data_ptr(), ws.data_ptr(),
                                  ws.numel() * 8, _stream()), "psam_region_neighbors")
    return nbr


def region_labels(bits: torch.Tensor, inv: torch.Tensor, nbr: torch.Tensor, complement: bool = False) -> torch.Tensor:
    """bits [K, W] int64 words (mask_pack's layout), inv [N] int64, nbr [V, 26] int32 -> labels [K, N] int32: per point the id of its component
    within the row's mask (the lowest voxel rank in the component), -1 outside the set; complement: the set is the points not in the row."""
    _chk(bits, torch.int64, "bits")
    N, V = _region_graph_chk(inv, nbr, "region_labels")
    if bits.dim() != 2 or bits.shape[0] < 1 or bits.shape[1] != mask_words(N):
        raise ValueError(f"region_labels: bits {tuple(bits.shape)} for N = {N}")
    K = bits.shape[0]
    L = _lib.load()
    nbytes = L.psam_region_labels_workspace_bytes(K, N, V)
    ws = _region_ws(nbytes, bits.device, "region_labels")
    labels = torch.empty(K, N, dtype=torch.int32, device=bits.device)
    check(L.psam_region_labels(bits.data_ptr(), inv.data_ptr(), nbr.data_ptr(), K, N, V, 1 if complement else 0, labels.data_ptr(), ws.data_ptr(),
                               ws.numel() * 8, _stream()), "psam_region_labels")
    return labels


def region_clean_workspace_bytes(K: int, N: int, V: int, S: int) -> int:
    return _lib.load().psam_region_clean_workspace_bytes(K, N, V, S)


def region_clean(bits: torch.Tensor, inv: torch.Tensor, nbr: torch.Tensor, min_island: int = 0, min_hole: int = 0, select: torch.Tensor = None,
                 seeds: torch.Tensor = None):
    """bits [K, W] int64, inv [N] int64, nbr [V, 26] int32, select [K] uint8 or None (every row), seeds [K, S] int32 point indices (-1 = unused) or
    None -> (bits_out [K, W] int64, area [K] int32, changed [K] uint8).  Per selected row, in order: complement components below min_hole points join
    the mask; components below min_island points leave it, except the largest (ties: lowest id); if a seed is a member then, only the components
    holding one stay.  An empty row stays empty; an unselected row is copied."""
    _chk(bits, torch.int64, "bits")
    N, V = _region_graph_chk(inv, nbr, "region_clean")
    if bits.dim() != 2 or bits.shape[0] < 1 or bits.shape[1] != mask_words(N):
        raise ValueError(f"region_clean: bits {tuple(bits.shape)} for N = {N}")
    K, S = bits.shape[0], 0
    if select is not None:
        _chk(select, torch.uint8, "select")
        if select.numel() != K:
            raise ValueError(f"region_clean: select [{select.numel()}] for K = {K}")
    if seeds is not None:
        _chk(seeds, torch.int32, "seeds")
        if seeds.dim() != 2 or seeds.shape[0] != K:
            raise ValueError(f"region_clean: seeds {tuple(seeds.shape)} for K = {K}")
        S = seeds.shape[1]
    if min(int(min_island), int(min_hole)) < 0:
        raise ValueError("region_clean: min_island and min_hole must not be negative")
    L = _lib.load()
    nbytes = L.psam_region_clean_workspace_bytes(K, N, V, S)
    ws = _region_ws(nbytes, bits.device, "region_clean")
    out = torch.empty_like(bits)
    area = torch.empty(K, dtype=torch.int32, device=bits.device)
    changed = torch.empty(K, dtype=torch.uint8, device=bits.device)
    check(L.psam_region_clean(bits.data_ptr(), _p(select), inv.data_ptr(), nbr.data_ptr(), _p(seeds) if S > 0 else 0, K, N, V, S, int(min_island),
                              int(min_hole), out.data_ptr(), area.data_ptr(), changed.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream()),
          "psam_region_clean")
    return out, area, changed


# ------------------------------------------------------------------------------------------ instance geometry (csrc/geometry.hip)
INSTANCE_RANGE_WORDS = 256      # PSAM_INSTANCE_RANGE_WORDS: the words of a row one wave owns; a row of more words is split over several


def _geometry_chk(xyz, bits, what: str):
    if xyz.dim() == 3 and xyz.shape[0] == 1:
        xyz = xyz[0]
    _chk(xyz, name="xyz"); _chk(bits, torch.int64, "bits")
    if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] < 1:
        raise ValueError(f"{what}: xyz must be [N, 3] with N >= 1 (one cloud), got {tuple(xyz.shape)}")
    N = xyz.shape[0]
    if bits.dim() != 2 or bits.shape[0] < 1 or bits.shape[1] != mask_words(N):
        raise ValueError(f"{what}: bits {tuple(bits.shape)} for N = {N}: need [K >= 1, {mask_words(N)}]")
    if bits.device != xyz.device:
        raise ValueError(f"{what}: xyz is on {xyz.device}, bits on {bits.device}")
    return xyz, N, bits.shape[0]


def _geometry_ws(nbytes: int, dev, what: str):
    if nbytes == 0:
        raise ValueError(f"{what}: the shape is outside what the kernels are built for (K <= 65535 rows per call, N <= 2^28)")
    return torch.empty(nbytes // 8 + 2, dtype=torch.int64, device=dev)      # torch allocations are at least 16-byte aligned


def mask_moments(xyz: torch.Tensor, bits: torch.Tensor, rgb: torch.Tensor = None):
    """xyz [N, 3] (or [1, N, 3]) f32, bits [K, W] int64 words (mask_pack's layout; bits past N are ignored), rgb like xyz or None ->
    (count [K] int32, sums [K, 12] f64, lo [K, 3] f32, hi [K, 3] f32) per mask: the exact member count, the sums of x, y, z, xx, xy, xz, yy, yz, zz,
    r, g, b over the members (exact fp64 terms, fp64 additions in a fixed order: bitwise reproducible, and a row's result does not depend on the
    other rows), and the fp32 bounding box (+inf / -inf for an empty row).  Without rgb the colour sums are 0.  No host synchronisation."""
    xyz, N, K = _geometry_chk(xyz, bits, "mask_moments")
    if rgb is not None:
        if rgb.dim() == 3 and rgb.shape[0] == 1:
            rgb = rgb[0]
        _chk(rgb, name="rgb")
        if tuple(rgb.shape) != tuple(xyz.shape) or rgb.device != xyz.device:
            raise ValueError(f"mask_moments: rgb must be {tuple(xyz.shape)} on {xyz.device} like xyz, got {tuple(rgb.shape)} on {rgb.device}")
    L = _lib.load()
    ws = _geometry_ws(L.psam_instance_moments_workspace_bytes(K, N), xyz.device, "mask_moments")
    count = torch.empty(K, dtype=torch.int32, device=xyz.device)
    sums = torch.empty(K, 12, dtype=torch.float64, device=xyz.device)
    lo = torch.empty(K, 3, dtype=torch.float32, device=xyz.device)
    hi = torch.empty(K, 3, dtype=torch.float32, device=xyz.device)
    check(L.psam_instance_moments(xyz.data_ptr(), _p(rgb), bits.data_ptr(), K, N, count.data_ptr(), sums.data_ptr(), lo.data_ptr(), hi.data_ptr(),
                                  ws.data_ptr(), ws.numel() * 8, _stream()), "psam_instance_moments")
    return count, sums, lo, hi


def mask_extents(xyz: torch.Tensor, bits: torch.Tensor, origin: torch.Tensor, axes: torch.Tensor = None):
    """xyz [N, 3] (or [1, N, 3]) f32, bits [K, W] int64 words, origin [K, 3] f32, axes [K, 3, 3] f32 (rows are the axes; None: the identity) ->
    (lo [K, 3], hi [K, 3], r2max [K]) f32: the box of every mask's members in its frame, p_i = (d.x a_i0 + d.y a_i1) + d.z a_i2 with d = x - origin,
    and the largest (d.x d.x + d.y d.y) + d.z d.z, every fp32 operation rounded on its own; +inf / -inf / -inf for an empty row."""
    xyz, N, K = _geometry_chk(xyz, bits, "mask_extents")
    _chk(origin, name="origin")
    if tuple(origin.shape) != (K, 3) or origin.device != xyz.device:
        raise ValueError(f"mask_extents: origin must be [{K}, 3] on {xyz.device}, got {tuple(origin.shape)} on {origin.device}")
    if axes is not None:
        _chk(axes, name="axes")
        if tuple(axes.shape) != (K, 3, 3) or axes.device != xyz.device:
            raise ValueError(f"mask_extents: axes must be [{K}, 3, 3] on {xyz.device}, got {tuple(axes.shape)} on {axes.device}")
    L = _lib.load()
    ws = _geometry_ws(L.psam_instance_extents_workspace_bytes(K, N), xyz.device, "mask_extents")
    lo = torch.empty(K, 3, dtype=torch.float32, device=xyz.device)
    hi = torch.empty(K, 3, dtype=torch.float32, device=xyz.device)
    r2max = torch.empty(K, dtype=torch.float32, device=xyz.device)
    check(L.psam_instance_extents(xyz.data_ptr(), bits.data_ptr(), K, N, origin.data_ptr(), _p(axes), lo.data_ptr(), hi.data_ptr(), r2max.data_ptr(),
                                  ws.data_ptr(), ws.numel() * 8, _stream()), "psam_instance_extents")
    return lo, hi, r2max


# ------------------------------------------------------------------------------------------ normals and superpoints (csrc/normals.hip, csrc/superpoints.hip)
def _superpoint_ws(nbytes: int, dev, what: str):
    if nbytes == 0:
        raise ValueError(f"{what}: the shape is outside what the kernels are built for (K <= 65535 rows per call, N <= 2^28, V <= N, S <= N)")
    return torch.empty(nbytes // 8 + 2, dtype=torch.int64, device=dev)      # torch allocations are at least 16-byte aligned


def _superpoint_int(value, lo: int, hi: int, what: str) -> int:
    if isinstance(value, bool) or not isinstance(value, int) or not lo <= value <= hi:
        raise ValueError(f"{what} must be an integer in {lo} .. {hi}, got {value!r}")
    return value


def voxel_normals(xyz: torch.Tensor, inv: torch.Tensor, nbr: torch.Tensor, min_points: int = 5, viewpoint=None, scatter: bool = False):
    """xyz [N, 3] (or [1, N, 3]) f32 in [-1, 1], inv [N] int64, nbr [V, 26] int32 (voxel_downsample / region_neighbors at origin -1) ->
    (count [V] int32, normal [V, 3] f32, curvature [V] f32, scatter [V, 6] f64 or None) per occupied voxel, over the points of the voxel and of its
    26 neighbours: their number, the unit eigenvector of the smallest eigenvalue of the exact integer scatter matrix S = n P - s s^T of the
    fixed-point coordinates floor(p 2^20) + 2^20, and l0 / (l0 + l1 + l2).  A voxel with count < min_points gets (0, 0, 0) and 0.  Sign: the
    component of largest magnitude is positive (ties: the lowest axis), or with viewpoint (three numbers) n . (viewpoint - mean) >= 0.  scatter: also
    return S (xx, xy, xz, yy, yz, zz).  Identical bits from run to run and for any order of the points.  No host synchronisation."""
    if xyz.dim() == 3 and xyz.shape[0] == 1:
        xyz = xyz[0]
    _chk(xyz, name="xyz")
    N, V = _region_graph_chk(inv, nbr, "voxel_normals")
    if xyz.dim() != 2 or tuple(xyz.shape) != (N, 3):
        raise ValueError(f"voxel_normals: xyz must be [{N}, 3] like inv, got {tuple(xyz.shape)}")
    if not (xyz.device == inv.device == nbr.device):
        raise ValueError(f"voxel_normals: xyz is on {xyz.device}, inv on {inv.device}, nbr on {nbr.device}")
    min_points = _superpoint_int(min_points, 1, 2 ** 31 - 1, "voxel_normals: min_points")
    view = None
    if viewpoint is not None:
        w = [float(c) for c in (viewpoint.tolist() if isinstance(viewpoint, torch.Tensor) else viewpoint)]
        if len(w) != 3 or not all(math.isfinite(c) for c in w):
            raise ValueError(f"voxel_normals: viewpoint must be three finite numbers, got {viewpoint!r}")
        view = (ctypes.c_float * 3)(*w)
    L = _lib.load()
    ws = _superpoint_ws(L.psam_normals_voxel_workspace_bytes(N, V), xyz.device, "voxel_normals")
    count = torch.empty(V, dtype=torch.int32, device=xyz.device)
    normal = torch.empty(V, 3, dtype=torch.float32, device=xyz.device)
    curvature = torch.empty(V, dtype=torch.float32, device=xyz.device)
    S = torch.empty(V, 6, dtype=torch.float64, device=xyz.device) if scatter else None
    check(L.psam_normals_voxel(xyz.data_ptr(), inv.data_ptr(), nbr.data_ptr(), N, V, min_points, ctypes.addressof(view) if view is not None else None,
                               count.data_ptr(), _p(S), normal.data_ptr(), curvature.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream()),
          "psam_normals_voxel")
    return count, normal, curvature, S


def superpoint_labels(inv: torch.Tensor, nbr: torch.Tensor, count: torch.Tensor, normal: torch.Tensor, curvature: torch.Tensor, cos_angle: float,
                      max_curvature: float, min_points: int = 5, min_size: int = 0, absorb_rounds: int = 2):
    """inv [N] int64, nbr [V, 26] int32, and voxel_normals' count [V] int32, normal [V, 3] f32, curvature [V] f32 ->
    (voxel_label [V], point_label [N], size [V]: the first S entries, zeros behind them; num [1] = S), all int32 on the device.  Touching voxels join when
    both have count >= min_points and curvature <= max_curvature and |n . n'| >= cos_angle (fp64, (x x' + y y') + z z'); then, absorb_rounds times,
    a voxel of a superpoint below min_size points goes to the neighbouring superpoint of at least min_size with the most parallel normal (ties: the
    lower label); the labels in use are renumbered 0 .. S - 1 in the order of their lowest voxel rank.  A point without a cell gets -1.  Exact and
    identical from run to run.  No host synchronisation."""
    N, V = _region_graph_chk(inv, nbr, "superpoint_labels")
    _chk(count, torch.int32, "count"); _chk(normal, name="normal"); _chk(curvature, name="curvature")
    if tuple(count.shape) != (V,) or tuple(normal.shape) != (V, 3) or tuple(curvature.shape) != (V,):
        raise ValueError(f"superpoint_labels: count, normal, curvature must be [{V}], [{V}, 3], [{V}], got {tuple(count.shape)}, {tuple(normal.shape)}, "
                         f"{tuple(curvature.shape)}")
    if not (inv.device == nbr.device == count.device == normal.device == curvature.device):
        raise ValueError("superpoint_labels: every tensor must be on the same device")
    min_points = _superpoint_int(min_points, 1, 2 ** 31 - 1, "superpoint_labels: min_points")
    min_size = _superpoint_int(min_size, 0, 2 ** 31 - 1, "superpoint_labels: min_size")
    absorb_rounds = _superpoint_int(absorb_rounds, 0, 64, "superpoint_labels: absorb_rounds")
    cos_angle, max_curvature = float(cos_angle), float(max_curvature)
    if not -1.0 <= cos_angle <= 1.0 or not 0.0 <= max_curvature < float("inf"):
        raise ValueError(f"superpoint_labels: need cos_angle in [-1, 1] and a finite max_curvature >= 0, got {cos_angle!r} and {max_curvature!r}")
    L = _lib.load()
    ws = _superpoint_ws(L.psam_superpoints_workspace_bytes(N, V), inv.device, "superpoint_labels")
    voxel_label = torch.empty(V, dtype=torch.int32, device=inv.device)
    point_label = torch.empty(N, dtype=torch.int32, device=inv.device)
    size = torch.empty(V, dtype=torch.int32, device=inv.device)
    num = torch.empty(1, dtype=torch.int32, device=inv.device)
    check(L.psam_superpoints(inv.data_ptr(), nbr.data_ptr(), count.data_ptr(), normal.data_ptr(), curvature.data_ptr(), N, V, min_points, max_curvature,
                             cos_angle, min_size, absorb_rounds, voxel_label.data_ptr(), point_label.data_ptr(), size.data_ptr(), num.data_ptr(),
                             ws.data_ptr(), ws.numel() * 8, _stream()), "psam_superpoints")
    return voxel_label, point_label, size, num


def superpoint_snap_workspace_bytes(K: int, N: int, S: int) -> int:
    return _lib.load().psam_superpoint_snap_workspace_bytes(K, N, S)


def superpoint_snap(bits: torch.Tensor, point_label: torch.Tensor, size: torch.Tensor, q16: int):
    """bits [K, W] int64 words (mask_pack's layout), point_label [N] int32, size [S] int32 (superpoint_labels', cut to S) ->
    (bits_out [K, W] int64, area [K] int32, changed [K] uint8): bit i of row k is set iff point i has a label and the row holds more than
    q16 / 65536 of its superpoint's points, cnt * 65536 > q16 * size in integers.  q16 = 0: any touch; 32768: a strict majority."""
    _chk(bits, torch.int64, "bits"); _chk(point_label, torch.int32, "point_label"); _chk(size, torch.int32, "size")
    if point_label.dim() != 1 or size.dim() != 1 or point_label.numel() < 1 or size.numel() < 1:
        raise ValueError(f"superpoint_snap: point_label must be [N] and size [S], got {tuple(point_label.shape)} and {tuple(size.shape)}")
    N, S = point_label.numel(), size.numel()
    if bits.dim() != 2 or bits.shape[0] < 1 or bits.shape[1] != mask_words(N):
        raise ValueError(f"superpoint_snap: bits {tuple(bits.shape)} for N = {N}")
    if not (bits.device == point_label.device == size.device):
        raise ValueError(f"superpoint_snap: bits is on {bits.device}, point_label on {point_label.device}, size on {size.device}")
    q16 = _superpoint_int(q16, 0, 65535, "superpoint_snap: q16")
    K = bits.shape[0]
    L = _lib.load()
    ws = _superpoint_ws(L.psam_superpoint_snap_workspace_bytes(K, N, S), bits.device, "superpoint_snap")
    out = torch.empty_like(bits)
    area = torch.empty(K, dtype=torch.int32, device=bits.device)
    changed = torch.empty(K, dtype=torch.uint8, device=bits.device)
    check(L.psam_superpoint_snap(bits.data_ptr(), point_label.data_ptr(), size.data_ptr(), K, N, S, q16, out.data_ptr(), area.data_ptr(),
                                 changed.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream()), "psam_superpoint_snap")
    return out, area, changed


# ------------------------------------------------------------------------------------------ scan maps (csrc/scanmap.hip)
MAP_MAX = 1 << 28                # points per add, and both capacities
MAP_HEADER_INTS = 16             # PSAM_MAP_HEADER_INTS
MAP_FLAG_VOXELS, MAP_FLAG_PAIRS, MAP_FLAG_COUNTS = 1, 2, 4
# the header's words (include/pointsam_hip.h: scan map)
MAP_H_FLAGS, MAP_H_V, MAP_H_ADDS, MAP_H_PAIRS, MAP_H_NEW, MAP_H_ACCEPTED, MAP_H_REJECTED = 3, 4, 5, 6, 7, 8, 9


def map_inv_h(voxel_size):
    """-> fl32(1 / fl32(voxel_size)), as voxel_downsample forms it.  ValueError unless the size and its inverse are finite positive fp32 numbers."""
    import numpy as np
    if isinstance(voxel_size, bool) or not isinstance(voxel_size, (int, float, np.floating, np.integer)):
        raise ValueError(f"map: voxel_size must be a number, got {voxel_size!r}")
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        h = np.float32(voxel_size)
        inv_h = np.float32(1) / h
    if not (np.isfinite(h) and h > 0 and np.isfinite(inv_h) and inv_h > 0):
        raise ValueError(f"map: voxel_size must be finite and positive with a finite positive fp32 inverse, got {voxel_size!r}")
    return inv_h


def map_capacities(max_voxels, max_pairs=None):
    """-> (max_voxels, max_pairs), both integers in 1 .. 2^28; max_pairs None = 2 * max_voxels (at most 2^28)."""
    max_voxels = _superpoint_int(max_voxels, 1, MAP_MAX, "map: max_voxels")
    max_pairs = min(2 * max_voxels, MAP_MAX) if max_pairs is None else _superpoint_int(max_pairs, 1, MAP_MAX, "map: max_pairs")
    return max_voxels, max_pairs


def map_bytes(max_voxels: int, max_pairs: int) -> int:
    """The bytes of a map block (psam_map_bytes)."""
    max_voxels, max_pairs = map_capacities(max_voxels, max_pairs)
    return _lib.load().psam_map_bytes(max_voxels, max_pairs)


def _map_block(what: str, block, max_voxels, max_pairs):
    """The checks every map entry shares -> the block's seven leading arguments (pointer, bytes, capacities)."""
    max_voxels, max_pairs = map_capacities(max_voxels, max_pairs)
    if not isinstance(block, torch.Tensor):
        raise TypeError(f"{what}: block must be a tensor, got {type(block).__name__}")
    if block.dtype != torch.int64 or block.dim() != 1:
        raise TypeError(f"{what}: block must be a one-dimensional int64 tensor, got {tuple(block.shape)} {block.dtype}")
    need = _lib.load().psam_map_bytes(max_voxels, max_pairs)
    if block.numel() * 8 < need:
        raise ValueError(f"{what}: the block holds {block.numel() * 8} bytes, a map of {max_voxels} voxels and {max_pairs} pairs needs {need}")
    _chk(block, torch.int64, "block")
    return block.data_ptr(), block.numel() * 8, max_voxels, max_pairs


def _map_points(what: str, t, name: str, like=None):
    t = _transfer_cloud(t, f"{what}: {name}")
    if like is not None and tuple(t.shape) != tuple(like.shape):
        raise ValueError(f"{what}: {name} must be {tuple(like.shape)} like xyz, got {tuple(t.shape)}")
    return t


def _map_count(what: str, V, max_voxels) -> int:
    return _superpoint_int(V, 1, max_voxels if isinstance(max_voxels, int) and not isinstance(max_voxels, bool) else MAP_MAX, f"{what}: V")


def map_clear(block: torch.Tensor, max_voxels: int, max_pairs: int, voxel_size) -> None:
    """Empties the map in `block` (int64 words, map_bytes) and sets its voxel size.  No host synchronisation."""
    inv_h = map_inv_h(voxel_size)
    lead = _map_block("map_clear", block, max_voxels, max_pairs)
    check(_lib.load().psam_map_clear(*lead, float(inv_h), _stream()), "psam_map_clear")


def map_header(block: torch.Tensor):
    """The block's header as a list of MAP_HEADER_INTS integers: one host read."""
    if not isinstance(block, torch.Tensor) or block.dtype != torch.int64 or block.dim() != 1 or block.numel() * 2 < MAP_HEADER_INTS:
        raise TypeError("map_header: block must be a one-dimensional int64 tensor of a map's size")
    return block[:MAP_HEADER_INTS // 2].view(torch.int32).tolist()


def map_add(block: torch.Tensor, max_voxels: int, max_pairs: int, xyz: torch.Tensor, rgb: torch.Tensor, labels: torch.Tensor = None, pose=None):
    """xyz, rgb [M, 3] f32, labels [M] int32 or None, pose (transfer_pose's forms, scan frame -> map frame, None = identity) -> (ids [M] int32, header):
    one add (include/pointsam_hip.h: scan map).  header = map_header after the add, the call's one host read; the caller looks at its flags."""
    xyz = _map_points("map_add", xyz, "xyz")
    rgb = _map_points("map_add", rgb, "rgb", xyz)
    M = xyz.shape[0]
    if labels is not None:
        if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int32:
            raise TypeError(f"map_add: labels must be an int32 tensor or None, got {getattr(labels, 'dtype', type(labels).__name__)}")
        if tuple(labels.shape) != (M,):
            raise ValueError(f"map_add: labels must be [{M}] like xyz, got {tuple(labels.shape)}")
    words = transfer_pose(pose)
    lead = _map_block("map_add", block, max_voxels, max_pairs)
    _chk(xyz, name="xyz"); _chk(rgb, name="rgb")
    if labels is not None:
        _chk(labels, torch.int32, "labels")
    if not (xyz.device == rgb.device == block.device and (labels is None or labels.device == xyz.device)):
        raise ValueError(f"map_add: xyz is on {xyz.device}, rgb on {rgb.device}, the block on {block.device}")
    L = _lib.load()
    ws = torch.empty(L.psam_map_add_workspace_bytes(M) // 8 + 2, dtype=torch.int64, device=xyz.device)      # torch allocations are at least 16-byte aligned
    ids = torch.empty(M, dtype=torch.int32, device=xyz.device)
    P, pose_ptr = _pose_arg(words)
    check(L.psam_map_add(*lead, xyz.data_ptr(), rgb.data_ptr(), _p(labels), M, pose_ptr, ids.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream()),
          "psam_map_add")
    return ids, map_header(block)


def map_locate(block: torch.Tensor, max_voxels: int, max_pairs: int, xyz: torch.Tensor, pose=None) -> torch.Tensor:
    """xyz [M, 3] f32 under pose -> ids [M] int32: the map's voxel at each point, -1 where there is none or the point is not accepted.  No host
    synchronisation; changes nothing."""
    xyz = _map_points("map_locate", xyz, "xyz")
    words = transfer_pose(pose)
    lead = _map_block("map_locate", block, max_voxels, max_pairs)
    _chk(xyz, name="xyz")
    ids = torch.empty(xyz.shape[0], dtype=torch.int32, device=xyz.device)
    P, pose_ptr = _pose_arg(words)
    check(_lib.load().psam_map_locate(*lead, xyz.data_ptr(), xyz.shape[0], pose_ptr, ids.data_ptr(), _stream()), "psam_map_locate")
    return ids


def map_labels(block: torch.Tensor, max_voxels: int, max_pairs: int, V: int, min_votes: int = 1):
    """-> (label [V] int32, votes [V] int32): per voxel the label with the most points, ties to the lower label; -1 and 0 below min_votes."""
    V = _map_count("map_labels", V, max_voxels)
    min_votes = _superpoint_int(min_votes, 1, 2 ** 31 - 1, "map_labels: min_votes")
    lead = _map_block("map_labels", block, max_voxels, max_pairs)
    out = torch.empty(2, V, dtype=torch.int32, device=block.device)
    check(_lib.load().psam_map_labels(*lead, V, min_votes, out[0].data_ptr(), out[1].data_ptr(), _stream()), "psam_map_labels")
    return out[0], out[1]


def map_cloud(block: torch.Tensor, max_voxels: int, max_pairs: int, V: int):
    """-> (xyz [V, 3] f32, rgb [V, 3] f32): per voxel the mean position and colour, fl32(fl64(sum) / fl64(count) * 2^-20 - 1)."""
    V = _map_count("map_cloud", V, max_voxels)
    lead = _map_block("map_cloud", block, max_voxels, max_pairs)
    out = torch.empty(2, V, 3, dtype=torch.float32, device=block.device)
    check(_lib.load().psam_map_cloud(*lead, V, out[0].data_ptr(), out[1].data_ptr(), _stream()), "psam_map_cloud")
    return out[0], out[1]


def map_fields(block: torch.Tensor, max_voxels: int, max_pairs: int, V: int):
    """-> (count [V] int32, first_seen [V] int32, last_seen [V] int32, keys [V] int64, sums [V, 6] int64): the map's integers per voxel; sums = the
    fixed-point sums of the position, then of the colour."""
    V = _map_count("map_fields", V, max_voxels)
    lead = _map_block("map_fields", block, max_voxels, max_pairs)
    out = torch.empty(3, V, dtype=torch.int32, device=block.device)
    keys = torch.empty(V, dtype=torch.int64, device=block.device)
    sums = torch.empty(V, 6, dtype=torch.int64, device=block.device)
    check(_lib.load().psam_map_fields(*lead, V, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), keys.data_ptr(), sums.data_ptr(), _stream()),
          "psam_map_fields")
    return out[0], out[1], out[2], keys, sums


# ------------------------------------------------------------------------------------------ scan map carving (csrc/carve.hip)
CARVE_HEADER_INTS = 16           # PSAM_CARVE_HEADER_INTS
CARVE_MAX_MARGIN = (1 << 21) - 1
# the header's words (include/pointsam_hip.h: scan map carving); 10, 11 hold CROSSED as one uint64
CARVE_H_CARVES, CARVE_H_STAMP, CARVE_H_ORIGIN, CARVE_H_RAYS, CARVE_H_ACCEPTED, CARVE_H_REJECTED, CARVE_H_HIT, CARVE_H_MISSED, CARVE_H_CROSSED = \
    1, 2, 3, 4, 5, 6, 7, 8, 10


def carve_origin(origin, pose=None, voxel_size=None):
    """Three numbers (the sensor's position in the scan's frame) -> their fp32 words [3].  With a voxel size: the origin goes through the pose and the
    cell arithmetic of a map point in numpy fp32, exactly as the device does it, and a ValueError says where it has no cell (off [-1, 1]^3)."""
    import numpy as np
    if isinstance(origin, torch.Tensor):
        origin = origin.detach().cpu().numpy()
    try:
        o = np.asarray(origin, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"carve: origin must be three numbers, got {origin!r}") from None
    if o.shape != (3,) or o.dtype.kind != "f":
        raise ValueError(f"carve: origin must be three numbers, got {origin!r}")
    with np.errstate(over="ignore"):
        o = o.astype(np.float32)
    if not np.isfinite(o).all():
        raise ValueError(f"carve: origin must be finite in fp32, got {origin!r}")
    if voxel_size is not None:
        inv_h = map_inv_h(voxel_size)
        words = transfer_pose(pose)
        p = o
        with np.errstate(all="ignore"):
            if words is not None:
                w = np.asarray(words, dtype=np.float32).reshape(3, 4)
                p = np.array([((w[a, 0] * o[0] + w[a, 1] * o[1]) + w[a, 2] * o[2]) + w[a, 3] for a in range(3)], dtype=np.float32)
            c = np.floor((p - np.float32(-1)) * inv_h)
            ok = (c >= 0) & (c < np.float32(1 << 21)) & (p >= np.float32(-1)) & (p <= np.float32(1))
        if not ok.all():
            raise ValueError(f"carve: the origin lands at {p.tolist()} in the map's frame, outside [-1, 1]^3: it has no cell, so no ray can be cast")
    return o


def carve_bytes(max_voxels: int) -> int:
    """The bytes of a carve block (psam_carve_bytes): 64 + 16 max_voxels."""
    return _lib.load().psam_carve_bytes(_superpoint_int(max_voxels, 1, MAP_MAX, "carve: max_voxels"))


def _carve_block(what: str, carve, max_voxels, on_device: bool = True):
    """The checks every carve entry shares -> the block's three leading arguments (pointer, bytes, max_voxels).  on_device False: the shape alone,
    for a caller that has other shapes to ask about before the first device check."""
    max_voxels = _superpoint_int(max_voxels, 1, MAP_MAX, f"{what}: max_voxels")
    if not isinstance(carve, torch.Tensor):
        raise TypeError(f"{what}: carve must be a tensor, got {type(carve).__name__}")
    if carve.dtype != torch.int64 or carve.dim() != 1:
        raise TypeError(f"{what}: carve must be a one-dimensional int64 tensor, got {tuple(carve.shape)} {carve.dtype}")
    need = _lib.load().psam_carve_bytes(max_voxels)
    if carve.numel() * 8 < need:
        raise ValueError(f"{what}: the carve block holds {carve.numel() * 8} bytes, a map of {max_voxels} voxels needs {need}")
    if on_device:
        _chk(carve, torch.int64, "carve")
    return carve.data_ptr(), carve.numel() * 8, max_voxels


def carve_clear(carve: torch.Tensor, max_voxels: int) -> None:
    """Empties the carve block (int64 words, carve_bytes).  No host synchronisation."""
    check(_lib.load().psam_carve_clear(*_carve_block("carve_clear", carve, max_voxels), _stream()), "psam_carve_clear")


def carve_header(carve: torch.Tensor):
    """The carve block's header as a list of CARVE_HEADER_INTS integers, words 10 and 11 joined into CARVE_H_CROSSED: one 64-byte host read."""
    if not isinstance(carve, torch.Tensor) or carve.dtype != torch.int64 or carve.dim() != 1 or carve.numel() * 2 < CARVE_HEADER_INTS:
        raise TypeError("carve_header: carve must be a one-dimensional int64 tensor of a carve block's size")
    h = carve[:CARVE_HEADER_INTS // 2].view(torch.int32).tolist()
    h[CARVE_H_CROSSED] = (h[CARVE_H_CROSSED] & 0xffffffff) | ((h[CARVE_H_CROSSED + 1] & 0xffffffff) << 32)
    return h


def carve_scan(block: torch.Tensor, max_voxels: int, max_pairs: int, carve: torch.Tensor, xyz: torch.Tensor, origin, pose=None, margin: int = 1,
               stamp: int = 1):
    """One carve of the map in `block` into the carve block `carve` (include/pointsam_hip.h: scan map carving): xyz [M, 3] f32, origin three numbers in
    the scan's frame, pose as map_add's, 0 <= margin < 2^21, 1 <= stamp <= 2^31 - 1 -> carve_header after it, the call's one host read."""
    xyz = _map_points("carve_scan", xyz, "xyz")
    o = carve_origin(origin)
    margin = _superpoint_int(margin, 0, CARVE_MAX_MARGIN, "carve_scan: margin")
    stamp = _superpoint_int(stamp, 1, 2 ** 31 - 1, "carve_scan: stamp")
    words = transfer_pose(pose)
    _carve_block("carve_scan", carve, max_voxels, on_device=False)
    lead = _map_block("carve_scan", block, max_voxels, max_pairs)
    tail = _carve_block("carve_scan", carve, lead[2])
    _chk(xyz, name="xyz")
    if not (xyz.device == block.device == carve.device):
        raise ValueError(f"carve_scan: xyz is on {xyz.device}, the block on {block.device}, the carve block on {carve.device}")
    L = _lib.load()
    M = xyz.shape[0]
    ws = torch.empty(L.psam_carve_workspace_bytes(M) // 8 + 2, dtype=torch.int64, device=xyz.device)
    P, pose_ptr = _pose_arg(words)
    O = (ctypes.c_float * 3)(*o.tolist())
    check(L.psam_carve_scan(*lead, tail[0], tail[1], xyz.data_ptr(), M, pose_ptr, ctypes.addressof(O), margin, stamp, ws.data_ptr(), ws.numel() * 8,
                            _stream()), "psam_carve_scan")
    return carve_header(carve)


def carve_fields(carve: torch.Tensor, max_voxels: int, V: int):
    """-> (hits, misses, last_hit, last_missed), each [V] int32: the carve block's integers per map voxel id."""
    V = _map_count("carve_fields", V, max_voxels)
    lead = _carve_block("carve_fields", carve, max_voxels)
    out = torch.empty(4, V, dtype=torch.int32, device=carve.device)
    check(_lib.load().psam_carve_fields(*lead, V, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), _stream()), "psam_carve_fields")
    return out[0], out[1], out[2], out[3]


# ------------------------------------------------------------------------------------------ scan map tracking (csrc/track.hip)
TRACK_MAX_REACH = 4              # PSAM_TRACK_MAX_REACH


def track_reach(radius, voxel_size) -> int:
    """The cells a search of `radius` looks out from a query's own cell on a map of `voxel_size`: max(1, ceil(fl32(radius) * fl32(1 / fl32(voxel_size)))),
    the product and the ceiling in fp64 on those fp32 values.  ValueError above TRACK_MAX_REACH: a step visits (2 reach + 1)^3 cells per query."""
    import math
    r, _, _ = transfer_radius(radius)
    reach = max(1, math.ceil(float(r) * float(map_inv_h(voxel_size))))
    if reach > TRACK_MAX_REACH:
        raise ValueError(f"track: radius {float(r)} is {reach} voxels of size {float(voxel_size)}: the search reaches at most {TRACK_MAX_REACH} cells "
                         f"from a query's own ({(2 * TRACK_MAX_REACH + 1) ** 3} cells per query)")
    return reach


def track_step(block: torch.Tensor, max_voxels: int, max_pairs: int, V: int, xyz: torch.Tensor, pose=None, radius=None, bits: torch.Tensor = None,
               skip: torch.Tensor = None, min_count: int = 1, return_nearest: bool = False, *, voxel_size):
    """One ICP step of a scan against a scan map (include/pointsam_hip.h: scan map tracking): the map's block, capacities and V, xyz [M, 3] f32 (the
    queries), pose as map_add's (scan frame -> map frame) -> sums [20] float64 on the device, align_step's words over the pairs (query, nearest map
    voxel within `radius` of pose(query)): the voxel's mean position, cloud()'s bits, found in the map's own table -- no cloud, no index.  radius:
    None = the voxel size; at most TRACK_MAX_REACH voxels (track_reach).  bits: align_step's.  skip: None, or [ceil(V / 64)] int64 words over voxel
    ids: a voxel whose bit is set is never paired.  min_count: a voxel observed fewer times is never paired.  return_nearest: also nearest [M] int32,
    the voxel id, -1 without a pair.  voxel_size: the size the map was cleared with (the header is not read back).  No host synchronisation."""
    xyz = _map_points("track_step", xyz, "xyz")
    words = transfer_pose(pose)
    _, _, r2 = transfer_radius(voxel_size if radius is None else radius)
    reach = track_reach(voxel_size if radius is None else radius, voxel_size)
    M = xyz.shape[0]
    bits = _packed_row("track_step", "bits", bits, M, "queries")
    V = _map_count("track_step", V, max_voxels)
    skip = _packed_row("track_step", "skip", skip, V, "voxels")
    min_count = _superpoint_int(min_count, 1, 2 ** 31 - 1, "track_step: min_count")
    lead = _map_block("track_step", block, max_voxels, max_pairs)
    _chk(xyz, name="xyz")
    if not (xyz.device == block.device and (bits is None or bits.device == xyz.device) and (skip is None or skip.device == xyz.device)):
        raise ValueError(f"track_step: xyz is on {xyz.device}, the block on {block.device}; bits and skip must be there too")
    dev = xyz.device
    L = _lib.load()
    sums = torch.empty(ALIGN_SUMS, dtype=torch.float64, device=dev)
    nearest = torch.empty(M, dtype=torch.int32, device=dev) if return_nearest else None
    ws = torch.empty(L.psam_track_workspace_bytes(M) // 8, dtype=torch.float64, device=dev)
    P, pose_ptr = _pose_arg(words)
    check(L.psam_track_step(*lead, V, _p(skip), min_count, reach, float(r2), xyz.data_ptr(), M, _p(bits), pose_ptr, _p(nearest), sums.data_ptr(),
                            ws.data_ptr(), ws.numel() * 8, _stream()), "psam_track_step")
    return (sums, nearest) if return_nearest else sums


def track_plane_step(block: torch.Tensor, max_voxels: int, max_pairs: int, V: int, xyz: torch.Tensor, normals: torch.Tensor, pose=None, radius=None,
                     bits: torch.Tensor = None, skip: torch.Tensor = None, min_count: int = 1, return_nearest: bool = False, *, voxel_size):
    """One point-to-plane ICP step of a scan against a scan map (include/pointsam_hip.h: scan map tracking): track_step's arguments and pair, bit for
    bit, and normals [V, 3] f32, one per voxel id, taken as given (map_normals' output fits) -> sums [32] float64 on the device, align_plane_step's
    words over the used pairs: p the posed point, s the voxel's mean, n its normal.  Word [30] counts the pairs whose normal is zero or not finite,
    word [31] the participating queries that have a cell.  return_nearest: also nearest [M] int32.  No host synchronisation."""
    xyz = _map_points("track_plane_step", xyz, "xyz")
    words = transfer_pose(pose)
    _, _, r2 = transfer_radius(voxel_size if radius is None else radius)
    reach = track_reach(voxel_size if radius is None else radius, voxel_size)
    M = xyz.shape[0]
    bits = _packed_row("track_plane_step", "bits", bits, M, "queries")
    V = _map_count("track_plane_step", V, max_voxels)
    if not isinstance(normals, torch.Tensor) or normals.dtype != torch.float32 or tuple(normals.shape) != (V, 3):
        raise ValueError(f"track_plane_step: normals must be a [{V}, 3] float32 tensor, one per voxel id, got "
                         f"{(tuple(normals.shape), normals.dtype) if isinstance(normals, torch.Tensor) else type(normals).__name__}")
    skip = _packed_row("track_plane_step", "skip", skip, V, "voxels")
    min_count = _superpoint_int(min_count, 1, 2 ** 31 - 1, "track_plane_step: min_count")
    lead = _map_block("track_plane_step", block, max_voxels, max_pairs)
    _chk(xyz, name="xyz")
    _chk(normals, name="normals")
    if not (xyz.device == block.device and normals.device == xyz.device and (bits is None or bits.device == xyz.device) and
            (skip is None or skip.device == xyz.device)):
        raise ValueError(f"track_plane_step: xyz is on {xyz.device}, the block on {block.device}; normals, bits and skip must be there too")
    dev = xyz.device
    L = _lib.load()
    sums = torch.empty(PLANE_SUMS, dtype=torch.float64, device=dev)
    nearest = torch.empty(M, dtype=torch.int32, device=dev) if return_nearest else None
    ws = torch.empty(L.psam_scanmap_plane_workspace_bytes(M) // 8, dtype=torch.float64, device=dev)
    P, pose_ptr = _pose_arg(words)
    check(L.psam_scanmap_plane_step(*lead, V, normals.data_ptr(), _p(skip), min_count, reach, float(r2), xyz.data_ptr(), M, _p(bits), pose_ptr, _p(nearest),
                                  sums.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream()), "psam_scanmap_plane_step")
    return (sums, nearest) if return_nearest else sums


# ------------------------------------------------------------------------------------------ scan map relocalisation (csrc/track_score.hip)
TRACK_SCORE_POSES = 4            # PSAM_RELOCALIZE_POSES: the poses one workgroup of psam_relocalize_score takes a tile of queries through


def track_score(block: torch.Tensor, max_voxels: int, max_pairs: int, V: int, xyz: torch.Tensor, poses, radius=None, skip: torch.Tensor = None,
                min_count: int = 1, *, voxel_size):
    """The score of a pose search against a scan map (include/pointsam_hip.h: scan map relocalisation): the map's block, capacities and V, xyz [M, 3]
    f32 (the queries), poses -> counts [P] int32 on the device: under pose p, the queries with at least one map voxel within `radius` of
    pose_p(query) -- exactly int(track_step(..., pose_p, radius, None, skip, min_count)[0]) for every p, from ONE call.  poses: align_score's -- [P, 3,
    4] or [P, 4, 4] host numbers, every row checked as transfer_pose checks a pose; or a [P, 12] float32 tensor ON THE DEVICE, taken AS VALIDATED (a
    row that is not finite scores 0).  radius, skip, min_count and voxel_size: track_step's.  1 <= P <= 2^20.  The workspace (one float4 per voxel
    id) is allocated here.  No host synchronisation."""
    xyz = _map_points("track_score", xyz, "xyz")
    _, _, r2 = transfer_radius(voxel_size if radius is None else radius)
    reach = track_reach(voxel_size if radius is None else radius, voxel_size)
    M = xyz.shape[0]
    V = _map_count("track_score", V, max_voxels)
    skip = _packed_row("track_score", "skip", skip, V, "voxels")
    min_count = _superpoint_int(min_count, 1, 2 ** 31 - 1, "track_score: min_count")
    on_device = isinstance(poses, torch.Tensor) and poses.is_cuda and poses.dim() == 2
    if on_device:
        if poses.shape[1] != 12 or not 1 <= poses.shape[0] <= ALIGN_SCORE_MAX_POSES:
            raise ValueError(f"track_score: device poses must be [P, 12] with 1 <= P <= 2^20, got {tuple(poses.shape)}")
    else:
        host = transfer_poses(poses)
    lead = _map_block("track_score", block, max_voxels, max_pairs)
    _chk(xyz, name="xyz")
    words = _chk(poses, name="poses") if on_device else torch.from_numpy(host).to(xyz.device)
    if not (xyz.device == block.device and words.device == xyz.device and (skip is None or skip.device == xyz.device)):
        raise ValueError(f"track_score: xyz is on {xyz.device}, the block on {block.device}; poses and skip must be there too")
    dev = xyz.device
    L = _lib.load()
    P = words.shape[0]
    counts = torch.empty(P, dtype=torch.int32, device=dev)
    ws = torch.empty(L.psam_relocalize_workspace_bytes(V) // 8, dtype=torch.int64, device=dev)      # torch allocations are at least 16-byte aligned
    check(L.psam_relocalize_score(*lead, V, _p(skip), min_count, reach, float(r2), xyz.data_ptr(), M, words.data_ptr(), P, counts.data_ptr(), ws.data_ptr(),
                                  ws.numel() * 8, _stream()), "psam_relocalize_score")
    return counts


# ------------------------------------------------------------------------------------------ scan map normals (csrc/map_normals.hip)
MAP_NORMALS_MAX_REACH = 2        # PSAM_SCANMAP_NORMALS_MAX_REACH


def map_normals(block: torch.Tensor, max_voxels: int, max_pairs: int, V: int, reach: int = 1, min_voxels: int = 5, skip: torch.Tensor = None,
                min_count: int = 1, scatter: bool = False):
    """One normal per voxel of a scan map (include/pointsam_hip.h: scan map normals) -> (count [V] int32, normal [V, 3] f32, curvature [V] f32), and
    with scatter=True also the exact scatter matrix [V, 6] float64 (xx, xy, xz, yy, yz, zz).  The neighbourhood of a voxel is the allowed voxels
    (count >= min_count, bit in `skip` clear: track_step's) in the (2 reach + 1)^3 cells around its own, reach 1 or 2; the scatter of their MEANS
    (cloud()'s bits) is exact integer arithmetic, the solve and the sign rule are voxel_normals' without a viewpoint.  Below min_voxels, and for a
    voxel that is not allowed itself, the normal is (0, 0, 0): track_plane_step does not use such a pair.  The block is only read; no workspace, no
    host synchronisation."""
    V = _map_count("map_normals", V, max_voxels)
    reach = _superpoint_int(reach, 1, MAP_NORMALS_MAX_REACH, "map_normals: reach")
    min_voxels = _superpoint_int(min_voxels, 1, 2 ** 31 - 1, "map_normals: min_voxels")
    skip = _packed_row("map_normals", "skip", skip, V, "voxels")
    min_count = _superpoint_int(min_count, 1, 2 ** 31 - 1, "map_normals: min_count")
    lead = _map_block("map_normals", block, max_voxels, max_pairs)
    if skip is not None and skip.device != block.device:
        raise ValueError(f"map_normals: the block is on {block.device}; skip must be there too")
    dev = block.device
    L = _lib.load()
    count = torch.empty(V, dtype=torch.int32, device=dev)
    normal = torch.empty(V, 3, dtype=torch.float32, device=dev)
    curvature = torch.empty(V, dtype=torch.float32, device=dev)
    S = torch.empty(V, 6, dtype=torch.float64, device=dev) if scatter else None
    check(L.psam_scanmap_normals(*lead, V, _p(skip), min_count, reach, min_voxels, count.data_ptr(), _p(S), normal.data_ptr(), curvature.data_ptr(), _stream()),
          "psam_scanmap_normals")
    return (count, normal, curvature, S) if scatter else (count, normal, curvature)


# ------------------------------------------------------------------------------------------ scan map views (csrc/map_view.hip)
MAP_VIEW_NO_GATE, MAP_VIEW_NO_LDS = 1, 2      # PSAM_MAP_VIEW_NO_GATE, PSAM_MAP_VIEW_NO_LDS: measurement switches, never a change of the result


def _map_view_camera(camera, what: str):
    from .views import Camera
    if not isinstance(camera, Camera):
        raise TypeError(f"{what}: camera must be a views.Camera, got {type(camera).__name__}")
    return camera


def map_view_eye(camera, voxel_size):
    """camera (views.Camera, its pose from the map's frame to the camera's), the map's voxel size -> (eye [3] fp32, cell (three ints)): the camera's
    centre e = -R^T t, computed in fp64 from the twelve fp32 pose words and rounded to fp32 once, and its cell by a map point's arithmetic in numpy
    fp32, floor((e + 1) * inv_h) with -1 <= e <= 1, exactly as the device does it (carve_origin's rule).  ValueError for an eye the map does not
    accept: rays from outside [-1, 1]^3 are not built.  Host only."""
    import numpy as np
    camera = _map_view_camera(camera, "map_view")
    inv_h = map_inv_h(voxel_size)
    w = np.asarray(camera.pose_words, dtype=np.float32).reshape(3, 4).astype(np.float64)
    with np.errstate(all="ignore"):
        eye = (-(w[:, :3].T @ w[:, 3])).astype(np.float32)
        c = np.floor((eye - np.float32(-1)) * inv_h)
        ok = (c >= 0) & (c < np.float32(1 << 21)) & (eye >= np.float32(-1)) & (eye <= np.float32(1))
    if not ok.all():
        raise ValueError(f"map_view: the camera's centre lies at {eye.tolist()} in the map's frame, outside [-1, 1]^3: it has no cell, so no ray can be cast")
    return eye, tuple(int(v) for v in c)


def map_view(block: torch.Tensor, max_voxels: int, max_pairs: int, V: int, camera, skip: torch.Tensor = None, min_count: int = 1, *, voxel_size,
             flags: int = 0, stats: torch.Tensor = None) -> torch.Tensor:
    """The scan map as `camera` sees it from inside (include/pointsam_hip.h: scan map views): the map's block, capacities and V, a views.Camera whose
    pose runs from the map's frame to the camera's -> keys [height, width] int64 in view_splat's format, (bits(depth) << 32) | VOXEL ID, all ones
    (-1) where the pixel's ray leaves the map without meeting a voxel: view_pick, view_paint_ids and view_paint_rows take them with N = V.  One ray
    per pixel from the centre of the eye's cell, walked through the map's table in exact integers; the first pairable voxel (skip, min_count:
    track_step's) whose mean lies at or behind `near` wins.  voxel_size: the size the map was cleared with.  flags: MAP_VIEW_NO_GATE /
    MAP_VIEW_NO_LDS, for measurement; stats: None or [2] int64 on the device, to which the visited cells and the table lookups are added.  The
    workspace (ops: psam_mapview_ws_bytes, at most 2.2 MB) is allocated here.  Every check comes before any device work; no host synchronisation."""
    eye, _ = map_view_eye(camera, voxel_size)
    inv_h = float(map_inv_h(voxel_size))
    V = _map_count("map_view", V, max_voxels)
    skip = _packed_row("map_view", "skip", skip, V, "voxels")
    min_count = _superpoint_int(min_count, 1, 2 ** 31 - 1, "map_view: min_count")
    flags = _superpoint_int(flags, 0, MAP_VIEW_NO_GATE | MAP_VIEW_NO_LDS, "map_view: flags")
    if stats is not None and not (isinstance(stats, torch.Tensor) and stats.dtype == torch.int64 and tuple(stats.shape) == (2,)):
        raise ValueError("map_view: stats must be None or a [2] int64 tensor")
    P, cam = _view_camera(camera, "map_view")
    lead = _map_block("map_view", block, max_voxels, max_pairs)
    if stats is not None:
        _chk(stats, torch.int64, "stats")
    if (skip is not None and skip.device != block.device) or (stats is not None and stats.device != block.device):
        raise ValueError(f"map_view: the block is on {block.device}; skip and stats must be there too")
    dev = block.device
    L = _lib.load()
    keys = torch.empty(cam[6], cam[5], dtype=torch.int64, device=dev)
    ws = torch.empty(L.psam_mapview_ws_bytes(inv_h) // 8 + 2, dtype=torch.int64, device=dev)      # torch allocations are at least 16-byte aligned
    E = (ctypes.c_float * 3)(*eye.tolist())
    check(L.psam_mapview(*lead, V, inv_h, *cam, ctypes.addressof(E), _p(skip), min_count, flags, keys.data_ptr(), _p(stats), ws.data_ptr(), ws.numel() * 8,
                          _stream()), "psam_mapview")
    return keys
