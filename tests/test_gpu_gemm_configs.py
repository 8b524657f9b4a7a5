"""Every launchable tile / ring configuration of the dense GEMMs, checked on its own.

The packed-operand f16x3 GEMM (csrc/gemm_f16x3p.hip: lock-step ring kernel, csrc/gemm_f16x3pp.hip: ping-pong kernel) ships about thirty
configurations that force_config hooks and documented environment switches reach; the f32 and bf16x6 GEMMs two or three each.  CONFIGS lists
them all with what each can do; a CPU test keeps it equal to the configuration tables the f16x3 dispatch is driven by (and to the `case` labels of
the f32 / bf16x6 switches), so a configuration added or changed later without coverage here fails without a GPU.  On the GPU every entry runs (and `psam_gemm_f16x3p_last_config` confirms it ran, not
a replacement) against an fp64 reference, bit for bit against cfg 21, on selection matrices that must reproduce the packed operands
exactly, with the fused extras and split-K where it takes them, and through the environment switches in fresh child processes."""
import ctypes
import hashlib
import json
import math
import os
import re
import subprocess
import sys
from collections import namedtuple

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "point_sam_amd", "csrc")

# ------------------------------------------------------------------------------------------------ the registry
# kernel: "lockstep" | "pingpong" (psam_gemm_f16x3p_force_config), "f32" (psam_gemm_force_config), "bf16x6" (psam_gemm_bf16x6_force_config)
# bm x bn: workgroup tile; per_cu: workgroups a CU holds; tn: 32-column accumulator tiles per wave (the SwiGLU gate pairs tiles 2q, 2q + 1);
# swiglu: the act == 3 epilogue runs (otherwise the launch is refused); extras: fused options psam_gemm_f16x3p_ex accepts with this
# configuration forced (others are refused); splitk: the split-K switch takes it.
Cfg = namedtuple("Cfg", "kernel bm bn per_cu tn swiglu extras splitk")
_ALL = frozenset({"pack", "stats", "ln_fold", "gmax", "hyper"})
_TWO_WIDE = frozenset({"pack", "stats", "ln_fold", "hyper"})
CONFIGS = {
    ("f16x3p", 0): Cfg("lockstep", 128, 128, 2, 2, True, frozenset(), True),
    ("f16x3p", 4): Cfg("lockstep", 256, 128, 1, 2, True, _ALL, True),
    ("f16x3p", 9): Cfg("lockstep", 128, 128, 1, 2, True, _TWO_WIDE, True),
    ("f16x3p", 12): Cfg("lockstep", 256, 192, 1, 3, False, frozenset(), True),
    ("f16x3p", 14): Cfg("lockstep", 256, 256, 1, 4, True, frozenset({"gmax"}), True),
    ("f16x3p", 21): Cfg("lockstep", 128, 128, 2, 2, True, _ALL, True),
    ("f16x3p", 23): Cfg("lockstep", 256, 192, 1, 3, False, frozenset(), True),
    ("f16x3p", 28): Cfg("lockstep", 128, 128, 2, 2, True, _TWO_WIDE, True),
    ("f16x3p", 29): Cfg("lockstep", 128, 128, 1, 2, True, frozenset(), True),
    ("f16x3p", 30): Cfg("lockstep", 128, 64, 3, 1, False, frozenset(), False),
    ("f16x3p", 31): Cfg("lockstep", 64, 128, 3, 2, True, frozenset(), False),
    ("f16x3p", 40): Cfg("lockstep", 128, 256, 1, 8, True, frozenset(), False),
    ("f16x3p", 41): Cfg("lockstep", 128, 128, 1, 2, True, _TWO_WIDE, True),
    ("f16x3p", 42): Cfg("lockstep", 128, 96, 1, 3, False, frozenset(), True),
    ("f16x3p", 50): Cfg("pingpong", 256, 256, 1, 2, True, _ALL, False),
    ("f16x3p", 51): Cfg("pingpong", 256, 256, 1, 2, True, _ALL, False),
    ("f16x3p", 52): Cfg("pingpong", 256, 256, 1, 2, True, _ALL, False),
    ("f16x3p", 53): Cfg("pingpong", 256, 256, 1, 4, True, frozenset({"pack", "ln_fold", "gmax"}), False),
    ("f16x3p", 55): Cfg("pingpong", 256, 128, 1, 2, True, _ALL, False),
    ("f16x3p", 56): Cfg("pingpong", 256, 128, 1, 2, True, _ALL, False),
    ("f16x3p", 57): Cfg("pingpong", 128, 128, 1, 2, True, _TWO_WIDE, False),
    ("f16x3p", 58): Cfg("pingpong", 128, 128, 2, 2, True, _TWO_WIDE, False),
    ("f16x3p", 59): Cfg("pingpong", 256, 256, 1, 2, True, _ALL, False),
    ("f16x3p", 60): Cfg("pingpong", 256, 256, 1, 2, True, _ALL, False),
    ("f16x3p", 61): Cfg("pingpong", 256, 256, 1, 2, True, _ALL, False),
    ("f16x3p", 62): Cfg("pingpong", 256, 224, 1, 7, False, frozenset({"pack", "ln_fold", "hyper"}), False),
    ("f16x3p", 63): Cfg("pingpong", 256, 192, 1, 6, True, _TWO_WIDE, False),
    ("f16x3p", 64): Cfg("pingpong", 256, 256, 1, 8, True, _TWO_WIDE, False),
    ("f16x3p", 65): Cfg("pingpong", 256, 128, 2, 2, True, _ALL, False),
    ("f16x3p", 66): Cfg("pingpong", 256, 128, 2, 2, True, _ALL, False),
    ("f16x3p", 67): Cfg("pingpong", 128, 256, 2, 2, True, _ALL, False),
    ("f32", 0): Cfg("f32", 128, 128, 1, 2, True, frozenset(), False),
    ("f32", 1): Cfg("f32", 128, 64, 1, 2, True, frozenset(), False),
    ("f32", 2): Cfg("f32", 64, 64, 1, 1, False, frozenset(), False),
    ("bf16x6", 0): Cfg("bf16x6", 128, 128, 1, 2, True, frozenset(), False),
    ("bf16x6", 1): Cfg("bf16x6", 128, 64, 1, 2, True, frozenset(), False),
}
F16 = sorted(c for (k, c) in CONFIGS if k == "f16x3p")
LOCKSTEP = [c for c in F16 if CONFIGS["f16x3p", c].kernel == "lockstep"]
PINGPONG = [c for c in F16 if CONFIGS["f16x3p", c].kernel == "pingpong"]
SPLITK = [c for c in F16 if CONFIGS["f16x3p", c].splitk]
REF_CFG = 21      # the production configuration every other one must reproduce bit for bit
NCU = 256         # MI355X


# ------------------------------------------------------------------------------------------------ source parsing (CPU)
def _default_build(src):
    """The lines a default build compiles: #ifdef PSAM_BUILD_EXPERIMENTS / PSAM_GEMM_ABLATE / PSAM_PP_ONLY blocks dropped (their #else kept),
    #ifndef blocks of those names kept; every other conditional left as it is."""
    names = ("PSAM_BUILD_EXPERIMENTS", "PSAM_GEMM_ABLATE", "PSAM_PP_ONLY")
    out, stack = [], []      # stack entries: None (neutral) or [keep_now, keep_after_else]
    for line in src.splitlines():
        t = line.strip()
        m = re.match(r"#\s*(ifdef|ifndef)\s+(\w+)", t)
        if m and m.group(2) in names:
            stack.append([m.group(1) == "ifndef", m.group(1) == "ifdef"])
            continue
        if re.match(r"#\s*if", t):
            stack.append(None)
        elif re.match(r"#\s*else", t) and stack and stack[-1] is not None:
            stack[-1][0] = stack[-1][1]
            continue
        elif re.match(r"#\s*endif", t):
            if stack.pop() is not None:
                continue
        if all(s is None or s[0] for s in stack):
            out.append(line)
    return "\n".join(out)


def _body(src, signature):
    """The brace-matched body of the first definition whose text starts with `signature`."""
    i = src.index(signature)
    j = src.index("{", src.index(")", i))
    depth = 0
    for k in range(j, len(src)):
        depth += {"{": 1, "}": -1}.get(src[k], 0)
        if depth == 0:
            return src[j:k + 1]
    raise AssertionError(signature)


def _switch_cases(body, after=None):
    """Integer `case` labels of the first `switch (cfg)` in body (after the text `after`)."""
    start = body.index(after) if after else 0
    return {int(c) for c in re.findall(r"\bcase\s+(\d+)\s*:", _body(body[start:], "switch (cfg)"))}


def _split_top(text):
    """text split at the commas outside <> and ()."""
    parts, depth, cur = [], 0, ""
    for ch in text:
        depth += {"<": 1, "(": 1, ">": -1, ")": -1}.get(ch, 0)
        if ch == "," and depth == 0:
            parts.append(cur.strip())
            cur = ""
        else:
            cur += ch
    return parts + [cur.strip()]


def config_table(src, name, caps_names):
    """{cfg: dict(bm, bn, per_cu, tn, caps, lds, reg, splitk)} of the F16PConfig table `name` (launchers as source text, None for nullptr)."""
    body = src[src.index(f"static const F16PConfig {name}[] = {{"):]
    body = body[body.index("\n"):body.index("\n};")]
    rows = {}
    for line in body.splitlines():
        line = line.split("//")[0].strip()
        if not line:
            continue
        assert line.startswith("{") and line.endswith("},"), line
        f = _split_top(line[1:-2])
        assert len(f) == 9, line
        cfg, bm, bn, per_cu, tn = map(int, f[:5])
        caps = 0
        for t in f[5].split("|"):
            caps |= int(t) if t.strip().isdigit() else caps_names[t.strip()]
        launch = [None if x == "nullptr" else x for x in f[6:]]
        assert cfg not in rows, cfg
        rows[cfg] = dict(bm=bm, bn=bn, per_cu=per_cu, tn=tn, caps=caps, lds=launch[0], reg=launch[1], splitk=launch[2])
    return rows


def _caps_names(args_h, *srcs):
    """The capability bits of gemm_f16x3p_args.h and the constexpr unions of them the tables use."""
    names = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(F16P_\w+) = (\d+),", args_h)}
    for src in srcs:
        for m in re.finditer(r"constexpr unsigned ([^;]+);", src):
            for part in m.group(1).split(","):
                k, v = part.split("=")
                names[k.strip()] = 0
                for t in v.split("|"):
                    names[k.strip()] |= names[t.strip()]
    return names


def dispatched_configs():
    rd = lambda f: _default_build(open(os.path.join(CSRC, f)).read())
    p, pp, g32, gsp, args = rd("gemm_f16x3p.hip"), rd("gemm_f16x3pp.hip"), rd("gemm.hip"), rd("gemm_split.hip"), rd("gemm_f16x3p_args.h")
    caps = _caps_names(args, p, pp)
    return {
        "lockstep": config_table(p, "k_f16x3p_configs", caps),
        "pingpong": config_table(pp, "k_pp_configs", caps),
        "caps": caps,
        "f32": _switch_cases(_body(g32, "PSAM_API int32_t psam_gemm_f32(")),
        "bf16x6": _switch_cases(_body(gsp, "PSAM_API int32_t psam_gemm_bf16x6(")),
    }


def test_registry_matches_the_configuration_tables():
    """CPU guard: the registry above is exactly what the default build can launch -- the configuration tables of the f16x3 kernels, entry by entry (tile,
    workgroups per CU, accumulator tiles per wave, SwiGLU, fused extras, split-K form), and the `case` labels of the f32 / bf16x6 switches.  An entry
    added to, removed from or changed in a table -- or in CONFIGS -- fails here until the GPU tests below cover it."""
    d = dispatched_configs()
    bit = d["caps"]
    kind = lambda k: {c for (g, c), v in CONFIGS.items() if v.kernel == k}
    for k in ("lockstep", "pingpong"):
        assert kind(k) == set(d[k]), (k, kind(k) ^ set(d[k]))
        for c, e in d[k].items():
            v = CONFIGS["f16x3p", c]
            swiglu = bool(e["caps"] & bit["F16P_SWIGLU"])
            # fused extras: row statistics and hyper products need the two-tile-wide wave tiles (on the lock-step kernel so do packed output and the folded
            # LayerNorm), the group maximum 64-row wave tiles; row statistics come with the SwiGLU epilogue only
            extras = set(_TWO_WIDE if e["caps"] & bit["F16P_TWO_WIDE"] else ()) | ({"pack", "ln_fold"} if k == "pingpong" else set())
            extras |= {"gmax"} if e["caps"] & bit["F16P_GMAX"] else set()
            if not swiglu:
                extras.discard("stats")
            got = Cfg(k, e["bm"], e["bn"], e["per_cu"], e["tn"], swiglu, frozenset(extras), e["splitk"] is not None)
            assert got == v, (c, got, v)
            assert e["lds"] is not None and not (e["caps"] & bit["F16P_SK_PICK"] and e["splitk"]), c
    assert kind("f32") == d["f32"] and kind("bf16x6") == d["bf16x6"], (d["f32"], d["bf16x6"])
    for (g, c), v in CONFIGS.items():
        assert v.swiglu == (v.tn % 2 == 0), (g, c)      # the SwiGLU gate pairs accumulator tiles (2q, 2q + 1)
        assert v.splitk <= (v.kernel == "lockstep") and not (v.extras and v.kernel in ("f32", "bf16x6")), (g, c)


def test_splitk_suggestion_resolves_the_forced_configuration_like_the_launch():
    """psam_gemm_f16x3p_splitk counts the tiles of the configuration a split-K launch would run: with a forced configuration that has no split-K form the
    launch runs the pick (30, 31: the same factor as unforced) or refuses to split (40: no split suggested).  Host logic: no GPU needed."""
    L = _lib()
    shapes = [(512, 1408, 6144, 0), (512, 1408, 1408, 1), (300, 260, 1024, 2), (1024, 1024, 2784, 0), (256, 4096, 4096, 0)]
    unforced = [L.psam_gemm_f16x3p_splitk(*s) for s in shapes]
    assert unforced[0] > 1
    try:
        for cfg, want in ((30, unforced), (31, unforced), (40, [1] * len(shapes))):
            L.psam_gemm_f16x3p_force_config(cfg)
            assert [L.psam_gemm_f16x3p_splitk(*s) for s in shapes] == want, cfg
    finally:
        L.psam_gemm_f16x3p_force_config(-1)


def test_default_build_filter():
    src = "a\n#ifdef PSAM_PP_ONLY\nb\n#else\nc\n#ifdef PSAM_BUILD_EXPERIMENTS\nd\n#endif\ne\n#endif\n#ifndef PSAM_BUILD_EXPERIMENTS\nf\n#else\ng\n#endif\n#if X\nh\n#endif"
    assert _default_build(src).split("\n") == ["a", "c", "e", "f", "#if X", "h", "#endif"]


# ------------------------------------------------------------------------------------------------ tile order (CPU)
def f16x3p_panel(tiles_m, tiles_n, BM, BN, K):
    """Python mirror of f16x3p_panel (csrc/gemm_f16x3p_args.h, no PSAM_GEMM_PANEL override): the column-panel width of the tile order."""
    l2, a_band, w_col = 2.5 * 1048576.0, float(BM) * K * 4, float(BN) * K * 4
    chunk = tiles_m * tiles_n / 8.0
    best, best_cost, P = tiles_n, 1e300, tiles_n
    while P >= 1:
        rows = min(chunk / P, tiles_m)
        panels = max(chunk / (tiles_m * P), 1.0)
        wp, conc = P * w_col, max(64.0 / P, 1.0)
        w_cost = wp * panels if (wp <= l2 or rows <= conc) else wp * (rows / conc) * panels
        cost = 8.0 * (w_cost + rows * a_band * panels)
        if cost < best_cost * 0.999:
            best_cost, best = cost, P
        P = (P + 1) // 2 if P > 1 else 0
    return best


BIG_K = 256


def hard_tile_order(M, N, cfg, K=BIG_K):
    """More tiles than one round of workgroup slots, a tile count that is not a multiple of the 8 XCDs, a last column panel that is partial."""
    bm, bn, per_cu = cfg.bm, cfg.bn, cfg.per_cu
    tm, tn = -(-M // bm), -(-N // bn)
    return tm * tn > NCU * per_cu and (tm * tn) % 8 != 0 and tn % f16x3p_panel(tm, tn, bm, bn, K) != 0


_BIG_CANDIDATES = [(3900, 5470), (4100, 5470), (3900, 6000), (5000, 3300), (4500, 4500), (3000, 7000), (2600, 5470), (5200, 4700)]


def big_shape(tile):
    """The first candidate (M, N), ragged in both, whose tile order is hard for this tile size."""
    for M, N in _BIG_CANDIDATES:
        if all(hard_tile_order(M, N, CONFIGS["f16x3p", c]) for c in F16 if (CONFIGS["f16x3p", c].bm, CONFIGS["f16x3p", c].bn) == tile):
            return M, N
    return None


TILES = sorted({(CONFIGS["f16x3p", c].bm, CONFIGS["f16x3p", c].bn) for c in F16})


def test_every_tile_size_has_a_hard_tile_order_shape():
    for t in TILES:
        assert big_shape(t) is not None, t
    assert hard_tile_order(3900, 5470, CONFIGS["f16x3p", 21])      # the issue's example on 128x128 tiles


# ------------------------------------------------------------------------------------------------ GPU helpers
torch = None


@pytest.fixture(scope="module")
def ops():
    global torch
    import torch as _torch
    torch = _torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd import ops as _ops
    _ops._lib.load()
    return _ops


def _lib():
    import torch as _torch  # noqa: F401  (first: the library must bind to the HIP runtime torch uses, see _lib.load)
    from point_sam_amd import _lib as L
    return L.load()


class Forced:
    """force_config / force_epilogue for one block; the hooks are process-global, the block always restores the defaults."""

    def __init__(self, cfg=-1, epi=-1, fixup=-1):
        self.cfg, self.epi, self.fixup = cfg, epi, fixup

    def __enter__(self):
        L = _lib()
        L.psam_gemm_f16x3p_force_config(self.cfg)
        L.psam_gemm_f16x3p_force_epilogue(self.epi)
        L.psam_gemm_f16x3p_force_splitk_fixup(self.fixup)
        return self

    def __exit__(self, *a):
        L = _lib()
        L.psam_gemm_f16x3p_force_config(-1)
        L.psam_gemm_f16x3p_force_epilogue(-1)
        L.psam_gemm_f16x3p_force_splitk_fixup(-1)


def _kg(K):
    return max(128, (K + 31) // 32 * 32)      # the packed GEMM's K: a multiple of the 32-k slab, at least 128 (zero padding)


def _pack(ops, x, Kg):
    """Row scales + g8-packed rows of fp32 x [rows, K] zero-padded to Kg columns (the padding changes neither scales nor values)."""
    xz = torch.zeros(x.shape[0], Kg, device="cuda")
    xz[:, :x.shape[1]] = x
    return ops.scale_pack_rows_g8(xz)


def _ptr(t):
    return None if t is None else t.data_ptr()


def f16x3p(ops, A, W, M, N, Kg, out, bias=None, res=None, rowbias=None, rowgroup=0, act=0, fuse=None):
    """One psam_gemm_f16x3p_ex launch on packed operands A = (packed, scale), W = (packed, scale); returns (status, config, split factor)."""
    L = _lib()
    ldr = 0 if res is None else res.stride(0)
    ldrb = 0 if rowbias is None else rowbias.stride(0)
    rc = L.psam_gemm_f16x3p_ex(A[0].data_ptr(), A[0].stride(0), A[1].data_ptr(), W[0].data_ptr(), W[0].stride(0), W[1].data_ptr(), _ptr(out),
                               0 if out is None else out.stride(0), _ptr(bias), _ptr(res), ldr, _ptr(rowbias), ldrb, rowgroup, M, N, Kg, 1.0, act,
                               None if fuse is None else ctypes.byref(fuse), None)
    return rc, L.psam_gemm_f16x3p_last_config(), L.psam_gemm_f16x3p_last_splitk()


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _act64(z, act):
    F = torch.nn.functional
    return F.gelu(z) if act == 1 else z.clamp_min(0) if act == 2 else z


def _swiglu_weights(g, Nh, K):
    """W [2 Nh, K] as the SwiGLU epilogue wants it: alternating 32-row blocks of the gate and value halves; also returns (Wg, Wx, bg, bx)."""
    Wg, Wx = torch.randn(Nh, K, generator=g) / K ** 0.5, torch.randn(Nh, K, generator=g) / K ** 0.5
    bg, bx = torch.randn(Nh, generator=g) * 0.1, torch.randn(Nh, generator=g) * 0.1
    W = torch.stack([Wg.view(Nh // 32, 32, K), Wx.view(Nh // 32, 32, K)], 1).reshape(2 * Nh, K)
    b = torch.stack([bg.view(Nh // 32, 32), bx.view(Nh // 32, 32)], 1).reshape(2 * Nh)
    return W, b, (Wg, Wx, bg, bx)


# ------------------------------------------------------------------------------------------------ 3. every configuration against fp64
EDGE_SHAPES = [(1, 200, 36), (77, 20, 4), (300, 130, 516), (257, 384, 2752), (1000, 64, 128), (640, 768, 160)]
GRP = 16


class Case:
    """One shape's operands and fp64 references (computed once, on the GPU, reused by every configuration)."""

    def __init__(self, ops, M, N, K, seed):
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(M, K, generator=g) * torch.exp(2 * torch.randn(M, 1, generator=g))      # rows spanning ~4 decades
        W = torch.randn(N, K, generator=g) * torch.exp(torch.randn(1, K, generator=g)) / K ** 0.5
        self.M, self.N, self.K, self.Kg = M, N, K, _kg(K)
        self.x, self.W = x.cuda(), W.cuda()
        self.b, self.res = torch.randn(N, generator=g).cuda(), torch.randn(M, N, generator=g).cuda()
        self.rb = torch.randn(-(-M // GRP), N, generator=g).cuda()
        self.A, self.Wp = _pack(ops, self.x, self.Kg), _pack(ops, self.W, self.Kg)
        xd, Wd = self.x.double(), self.W.double()
        z = xd @ Wd.T
        self.scale = xd.abs() @ Wd.abs().T + 1.0
        self.want = {"gelu_res": _act64(z + self.b.double(), 1) + self.res.double(), "res_inplace": z + self.b.double() + self.res.double(),
                     "relu_rowbias": _act64(z + self.rb.double().repeat_interleave(GRP, 0)[:M], 2)}
        self.swiglu = None
        if N % 64 == 0:
            Ws, bs, (Wg, Wx, bg, bx) = _swiglu_weights(g, N // 2, K)
            self.Ws, self.bs = _pack(ops, Ws.cuda(), self.Kg), bs.cuda()
            Wg, Wx, bg, bx = Wg.cuda().double(), Wx.cuda().double(), bg.cuda().double(), bx.cuda().double()
            self.swiglu = torch.nn.functional.silu(xd @ Wg.T + bg) * (xd @ Wx.T + bx)
            self.scale_sw = (xd.abs() @ Wg.abs().T + 1.0) * (xd.abs() @ Wx.abs().T + 1.0)
        self.err32 = {k: self._err(self._f32(ops, k), k) for k in self.want}

    def _f32(self, ops, kind):
        with ops.gemm_mode("f32"):
            if kind == "gelu_res":
                return ops.linear(self.x, self.W, self.b, act=ops.ACT_GELU, residual=self.res)
            if kind == "res_inplace":
                y = self.res.clone()
                return ops.linear(self.x, self.W, self.b, residual=y, out=y)
            return ops.linear(self.x, self.W, None, act=ops.ACT_RELU, rowbias=self.rb, rowgroup=GRP)

    def _err(self, y, kind):
        return ((y.double() - self.want[kind]).abs() / self.scale).max().item()

    def run(self, ops, kind):
        M, N = self.M, self.N
        if kind == "gelu_res":
            y = _nan(M, N)
            st = f16x3p(ops, self.A, self.Wp, M, N, self.Kg, y, bias=self.b, res=self.res, act=1)
        elif kind == "res_inplace":
            y = self.res.clone()
            st = f16x3p(ops, self.A, self.Wp, M, N, self.Kg, y, bias=self.b, res=y)
        elif kind == "relu_rowbias":
            y = _nan(M, N)
            st = f16x3p(ops, self.A, self.Wp, M, N, self.Kg, y, rowbias=self.rb, rowgroup=GRP, act=2)
        else:
            y = _nan(M, N // 2)
            st = f16x3p(ops, self.A, self.Ws, M, N, self.Kg, y, bias=self.bs, act=3)
        return y, st


@pytest.fixture(scope="module")
def edge_cases(ops):
    return [Case(ops, M, N, K, 1000 + i) for i, (M, N, K) in enumerate(EDGE_SHAPES)]


def _bar(K):
    return 3e-7 * math.sqrt(K) + 1e-7


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", F16)
def test_config_matches_fp64(ops, edge_cases, cfg):
    """Each configuration, both epilogue forms: bias + GELU + residual, in-place residual, ReLU + row bias, SwiGLU -- on M = 1 .. several tiles,
    ragged M and N, N below one tile, K = 4, 36, 516, 2752 (K tails inside the slab) -- within 3e-7 sqrt(K) of sum |x||w| and within 4x the f32
    kernel's error, every output element written and finite, and the configuration that ran is the one forced.  Where the registry says SwiGLU
    is impossible the launch is refused, not mis-computed."""
    info = CONFIGS["f16x3p", cfg]
    bad = []
    for epi in (0, 1):
        with Forced(cfg, epi):
            for c in edge_cases:
                where = f"cfg {cfg} epi {epi} {c.M}x{c.N}x{c.K}"
                for kind in ("gelu_res", "res_inplace", "relu_rowbias"):
                    y, (rc, ran, ks) = c.run(ops, kind)
                    torch.cuda.synchronize()
                    assert rc == 0, (where, kind, _lib().psam_last_error_string())
                    assert (ran, ks) == (cfg, 1), (where, kind, ran, ks)
                    if not torch.isfinite(y).all():
                        bad.append((where, kind, "unwritten / non-finite outputs", int((~torch.isfinite(y)).sum())))
                        continue
                    err = c._err(y, kind)
                    if not (err < _bar(c.K) and err < 4 * c.err32[kind] + 1e-7):
                        bad.append((where, kind, err, c.err32[kind]))
                if c.swiglu is None:
                    continue
                y, (rc, ran, ks) = c.run(ops, "swiglu")
                torch.cuda.synchronize()
                if not info.swiglu:
                    assert rc != 0 and ran == -1, (where, "SwiGLU not refused", rc, ran)
                    continue
                assert rc == 0 and (ran, ks) == (cfg, 1), (where, "swiglu", rc, ran, _lib().psam_last_error_string())
                if not torch.isfinite(y).all():
                    bad.append((where, "swiglu", "unwritten / non-finite outputs"))
                    continue
                err = ((y.double() - c.swiglu).abs() / c.scale_sw).max().item()
                if not err < 2 * _bar(c.K):
                    bad.append((where, "swiglu", err))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 4a. the same bits as cfg 21
class BigCase:
    def __init__(self, ops, M, N, K, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.M, self.N, self.K = M, N, K
        x = torch.randn(M, K, device="cuda", generator=g) * torch.exp(torch.randn(M, 1, device="cuda", generator=g))
        W = torch.randn(N, K, device="cuda", generator=g) / K ** 0.5
        self.b, self.res = torch.randn(N, device="cuda", generator=g), torch.randn(M, N, device="cuda", generator=g)
        self.A, self.Wp = _pack(ops, x, K), _pack(ops, W, K)
        self.x, self.W = x, W

    def run(self, ops, kind):
        M, N, K = self.M, self.N, self.K
        if kind == "res_inplace":
            y = self.res.clone()
            return y, f16x3p(ops, self.A, self.Wp, M, N, K, y, bias=self.b, res=y)
        y = _nan(M, N)
        if kind == "plain":
            return y, f16x3p(ops, self.A, self.Wp, M, N, K, y)
        return y, f16x3p(ops, self.A, self.Wp, M, N, K, y, bias=self.b, act=1)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _first_diff(a, b):
    d = (a.view(torch.int32) != b.view(torch.int32)).nonzero()
    return [tuple(int(v) for v in r) for r in d[:4].tolist()], int(d.shape[0])


@pytest.mark.gpu
@pytest.mark.parametrize("tile", TILES, ids=lambda t: f"{t[0]}x{t[1]}")
def test_configs_give_the_bits_of_cfg21(ops, edge_cases, tile):
    """Plain, bias + GELU and in-place residual epilogues: every non-split f16x3 configuration of this tile size, lock-step and ping-pong, both
    epilogue forms, gives exactly the bits of cfg 21 -- on the edge shapes and on one multi-round shape whose tile order is hard for this tile
    size (more tiles than a round of CUs, a tile count that is no multiple of the 8 XCDs, a partial last column panel) and which is checked
    against fp64 as well."""
    cfgs = [c for c in F16 if (CONFIGS["f16x3p", c].bm, CONFIGS["f16x3p", c].bn) == tile]
    M, N = big_shape(tile)
    big = BigCase(ops, M, N, BIG_K, 7 + M + N)
    shapes = [(c.M, c.N, c.Kg, c) for c in edge_cases] + [(M, N, BIG_K, big)]
    bad = []
    for (m, n, k, case) in shapes:
        for kind in ("plain", "gelu", "res_inplace"):
            if isinstance(case, Case):
                case_run = lambda: BigCase.run(_View(case), ops, kind)
            else:
                case_run = lambda: case.run(ops, kind)
            with Forced(REF_CFG, 1):
                ref, (rc, ran, _) = case_run()
            assert rc == 0 and ran == REF_CFG, (rc, ran)
            torch.cuda.synchronize()
            assert torch.isfinite(ref).all()
            if case is big and kind == "gelu":
                z = case.x.double() @ case.W.double().T
                err = ((ref.double() - _act64(z + case.b.double(), 1)).abs() / (case.x.double().abs() @ case.W.double().abs().T + 1.0)).max().item()
                assert err < _bar(k), (m, n, err)
                del z
            for cfg in cfgs + [REF_CFG]:
                for epi in (0, 1):
                    with Forced(cfg, epi):
                        y, (rc, ran, ks) = case_run()
                    torch.cuda.synchronize()
                    assert rc == 0 and (ran, ks) == (cfg, 1), (cfg, epi, m, n, k, kind, rc, ran, _lib().psam_last_error_string())
                    if not _same_bits(y, ref):
                        bad.append((cfg, epi, (m, n, k), kind) + _first_diff(y, ref))
            del ref, y
    assert not bad, bad


class _View:
    """A Case seen through BigCase.run (the padded K of its packed operands)."""

    def __init__(self, c):
        self.M, self.N, self.K, self.A, self.Wp, self.b, self.res = c.M, c.N, c.Kg, c.A, c.Wp, c.b, c.res


# ------------------------------------------------------------------------------------------------ 4b. selection matrices
SEL_K = 2752      # 172 k16 steps, 86 slabs: ring wraps of every depth, the tail of the K loop


def _perm(n):
    return [(i * 37 + 11) % n for i in range(n)]      # 37 is prime to 2752: a permutation of 0 .. n-1


@pytest.fixture(scope="module")
def sel(ops):
    from g8_reference import unpack_g8      # imports torch: here, like every use of torch in this module
    g = torch.Generator().manual_seed(5)
    K, R = SEL_K, 300
    pi = torch.tensor(_perm(K))
    onehot = torch.zeros(K, K)
    onehot[torch.arange(K), pi] = 1.0
    # random operand with 20 binary orders of magnitude along k: the lo plane holds fp16 subnormals
    dense = torch.randn(R, K, generator=g) * 2.0 ** -torch.randint(0, 21, (R, K), generator=g).float()
    oh, dn = _pack(ops, onehot.cuda(), K), _pack(ops, dense.cuda(), K)
    dec = unpack_g8(dn[0], dn[1], K)                     # exact values of the packed dense operand
    assert (oh[1] == 2.0 ** 14).all() and (unpack_g8(oh[0], oh[1], K) == onehot.cuda().double()).all()
    pic = pi.cuda()
    return dict(K=K, R=R, pi=pi, oh=oh, dn=dn, want_a=dec[:, pic].T.contiguous(), want_w=dec[:, pic].contiguous())


def _sel_mismatches(y, want, pi, a_side):
    d = (y.double() != want).nonzero()
    rows = [tuple(int(v) for v in r) for r in d[:6].tolist()]
    # (row, col, k): the k the one-hot row selected
    return int(d.shape[0]), [(r, c, int(pi[r] if a_side else pi[c])) for r, c in rows]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", F16)
def test_selection_matrices_reproduce_the_packed_operand(ops, sel, cfg):
    """A rows one-hot at column pi(i): C[i, :] is the DECODED packed weight column pi(i), exactly (hi*lo + lo*hi + hi*hi of a one-hot row is exact
    in fp32, the scales are powers of two).  W rows one-hot: C[:, n] is the decoded packed A column pi(n) (the A side's lo plane).  pi sweeps every
    k of K = 2752, so a k16 step dropped or repeated at a ring wrap, a hi / lo swap, a swizzle error or an edge-tile clamp leaking into stored rows
    shows as the (row, col, k) it broke."""
    K, R = sel["K"], sel["R"]
    bad = []
    for epi in (0, 1):
        with Forced(cfg, epi):
            ya = _nan(K, R)
            st_a = f16x3p(ops, sel["oh"], sel["dn"], K, R, K, ya)
            yw = _nan(R, K)
            st_w = f16x3p(ops, sel["dn"], sel["oh"], R, K, K, yw)
        torch.cuda.synchronize()
        assert st_a == (0, cfg, 1) and st_w == (0, cfg, 1), (epi, st_a, st_w)
        for name, y, want, a_side in (("A one-hot", ya, sel["want_a"], True), ("W one-hot", yw, sel["want_w"], False)):
            if not torch.equal(y.double(), want):
                bad.append((cfg, epi, name) + _sel_mismatches(y, want, sel["pi"], a_side))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 5a. fused extras
FM, FN, FK = 1024, 768, 512


@pytest.fixture(scope="module")
def fused(ops):
    g = torch.Generator().manual_seed(9)
    x = torch.randn(FM, FK, generator=g) * torch.exp(torch.randn(FM, 1, generator=g))
    W = torch.randn(FN, FK, generator=g) / FK ** 0.5
    Ws, bs, _ = _swiglu_weights(g, FN // 2, FK)
    d = dict(A=_pack(ops, x.cuda(), FK), W=_pack(ops, W.cuda(), FK), Ws=_pack(ops, Ws.cuda(), FK), bs=bs.cuda(),
             b=(torch.randn(FN, generator=g) * 0.1).cuda(), res=torch.randn(FM, FN, generator=g).cuda(),
             mean=torch.randn(FM, generator=g).cuda() * 0.1, rstd=(1 + torch.rand(FM, generator=g)).cuda(), lnc=torch.randn(FN, generator=g).cuda())
    d["k1"] = float(2.0 ** 15 * math.sqrt(FK) * W.double().norm(dim=1).max())
    d["k1s"] = float(2.0 ** 15 * math.sqrt(FK) * Ws.double().norm(dim=1).max())
    return d


def _fused_run(ops, f, what):
    """One fused launch: returns ((status, config, split), {name: output tensor})."""
    from point_sam_amd import _lib as Lm
    fuse = Lm.GemmFuse()
    o = {}
    if what == "swiglu_stats_pack":
        o["C"], o["scale"], o["stats"] = _nan(FM, FN // 2), _nan(FM), _nan(FM, ops.stat_segs(FN), 2)
        fuse.out_scale, fuse.out_k1, fuse.out_k2, fuse.pack_out = o["scale"].data_ptr(), f["k1s"], float(f["bs"].abs().max()), 1
        fuse.stats, fuse.stat_cols = o["stats"].data_ptr(), FN // 2 - 40
        st = f16x3p(ops, f["A"], f["Ws"], FM, FN, FK, o["C"], bias=f["bs"], act=3, fuse=fuse)
        o["stats"] = o["stats"][:, :(FN // 2 - 40 + 31) // 32]
    elif what == "pack_gelu":
        o["C"], o["scale"] = _nan(FM, FN), _nan(FM)
        fuse.out_scale, fuse.out_k1, fuse.out_k2, fuse.pack_out = o["scale"].data_ptr(), f["k1"], float(f["b"].abs().max()) + 1.0, 1
        st = f16x3p(ops, f["A"], f["W"], FM, FN, FK, o["C"], bias=f["b"], act=1, fuse=fuse)
    elif what == "ln_fold_res":
        o["C"] = _nan(FM, FN)
        fuse.ln_mean, fuse.ln_rstd, fuse.ln_c = f["mean"].data_ptr(), f["rstd"].data_ptr(), f["lnc"].data_ptr()
        st = f16x3p(ops, f["A"], f["W"], FM, FN, FK, o["C"], bias=f["b"], res=f["res"], fuse=fuse)
    else:      # gmax32 / gmax64 / gmax64_nostore
        k = 32 if what == "gmax32" else 64
        no_store = what.endswith("nostore")
        o["gmax"] = _nan(FM // k, FN)
        fuse.gmax_out, fuse.gmax_ld, fuse.gmax_k, fuse.no_store = o["gmax"].data_ptr(), FN, k, int(no_store)
        if not no_store:
            o["C"] = _nan(FM, FN)
        st = f16x3p(ops, f["A"], f["W"], FM, FN, FK, o["gmax"] if no_store else o["C"], bias=f["b"], act=2, fuse=fuse)      # (no_store: C never written)
    return st, o


FUSED = {"swiglu_stats_pack": {"stats", "pack"}, "pack_gelu": {"pack"}, "ln_fold_res": {"ln_fold"}, "gmax32": {"gmax"}, "gmax64": {"gmax"},
         "gmax64_nostore": {"gmax"}}


@pytest.mark.gpu
@pytest.mark.parametrize("what", sorted(FUSED))
def test_fused_extras_per_config(ops, fused, what):
    """Every configuration that takes a fused extra (packed output, SwiGLU row statistics, folded LayerNorm, group maximum with and without the
    stored output) gives the default configuration's bits in every output; every other configuration, forced, is refused."""
    with Forced():
        st, ref = _fused_run(ops, fused, what)
    torch.cuda.synchronize()
    assert st[0] == 0 and st[1] >= 0, (st, _lib().psam_last_error_string())
    for k, v in ref.items():
        if k == "C" and "pack" in what:      # g8-packed rows: every word overwritten (no NaN fill left)
            assert (v.view(torch.int32) != 0x7FC00000).all(), (what, k)
        else:
            assert torch.isfinite(v).all(), (what, k)
    bad = []
    for cfg in F16:
        info = CONFIGS["f16x3p", cfg]
        ok = FUSED[what] <= info.extras and (what != "swiglu_stats_pack" or info.swiglu)
        for epi in (0, 1):
            with Forced(cfg, epi):
                st, out = _fused_run(ops, fused, what)
            torch.cuda.synchronize()
            if not ok:
                if st[0] == 0 or st[1] != -1:
                    bad.append((cfg, epi, "not refused", st))
                continue
            if st != (0, cfg, 1):
                bad.append((cfg, epi, "did not run as forced", st, _lib().psam_last_error_string()))
                continue
            for k in ref:
                if not _same_bits(out[k].contiguous(), ref[k].contiguous()):
                    bad.append((cfg, epi, k) + _first_diff(out[k].contiguous(), ref[k].contiguous()))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 5b. split-K
@pytest.mark.gpu
@pytest.mark.parametrize("cfg", SPLITK)
def test_split_k_per_config(ops, cfg):
    """Each configuration of the split-K switch with 2 and 4 splits: within the fp64 bar, bitwise repeatable, and the in-kernel fix-up and the
    partial planes + reduction launch give the same bits."""
    from point_sam_amd import _lib as Lm
    M, N, K = 520, 392, 2752
    g = torch.Generator().manual_seed(cfg)
    x = torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, 1, generator=g))
    W = torch.randn(N, K, generator=g) / K ** 0.5
    b, res = torch.randn(N, generator=g).cuda(), torch.randn(M, N, generator=g).cuda()
    A, Wp = _pack(ops, x.cuda(), K), _pack(ops, W.cuda(), K)
    xd, Wd = x.cuda().double(), W.cuda().double()
    want = _act64(xd @ Wd.T + b.double(), 1) + res.double()
    scale = xd.abs() @ Wd.abs().T + 1.0
    info = CONFIGS["f16x3p", cfg]
    plane = -(-M // info.bm) * info.bm * -(-N // info.bn) * info.bn      # room for the raw accumulator tiles: the fix-up form is taken
    counters = ops.new_counters("cuda")
    for ks in (2, 4):
        outs = {}
        for fixup in (1, 0, 1):
            ws = _nan(ks * plane)
            fuse = Lm.GemmFuse()
            fuse.splitk_ws, fuse.splitk_plane, fuse.splitk = ws.data_ptr(), plane, ks
            fuse.counters = counters.data_ptr()
            y = _nan(M, N)
            with Forced(cfg, fixup=fixup):
                st = f16x3p(ops, A, Wp, M, N, K, y, bias=b, res=res, act=1, fuse=fuse)
            torch.cuda.synchronize()
            assert st == (0, cfg, ks), (ks, fixup, st, _lib().psam_last_error_string())
            assert torch.isfinite(y).all(), (ks, fixup)
            if fixup in outs:
                assert _same_bits(y, outs[fixup]), (ks, "not repeatable") + _first_diff(y, outs[fixup])
            outs[fixup] = y
        assert _same_bits(outs[0], outs[1]), (ks, "fix-up != reduction launch") + _first_diff(outs[0], outs[1])
        err = ((outs[1].double() - want).abs() / scale).max().item()
        assert err < _bar(K), (ks, err)
        assert (counters == 0).all()


# ------------------------------------------------------------------------------------------------ f32 / bf16x6 configurations
@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["f32", "bf16x6"])
def test_f32_and_bf16x6_configs_match_fp64(ops, kernel):
    """The forced tile configurations of the f32 and the split-bf16 GEMMs against fp64 (bias + GELU + residual, SwiGLU where the registry allows
    it, refused where not), on the edge shapes; an unknown configuration is refused."""
    L = _lib()
    fn, force = (L.psam_gemm_f32, L.psam_gemm_force_config) if kernel == "f32" else (L.psam_gemm_bf16x6, L.psam_gemm_bf16x6_force_config)
    cfgs = sorted(c for (k, c) in CONFIGS if k == kernel)
    bad = []
    try:
        for cfg in cfgs + [7]:
            force(cfg)
            for i, (M, N, K) in enumerate(EDGE_SHAPES):
                g = torch.Generator().manual_seed(50 + i)
                x = torch.randn(M, K, generator=g) * torch.exp(2 * torch.randn(M, 1, generator=g))
                W = torch.randn(N, K, generator=g) / K ** 0.5
                b, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
                xd, Wd, bd, rd = x.cuda(), W.cuda(), b.cuda(), res.cuda()
                y = _nan(M, N)
                rc = fn(xd.data_ptr(), K, 0, 0, Wd.data_ptr(), K, 0, 0, y.data_ptr(), N, 0, 0, bd.data_ptr(), rd.data_ptr(), N, 0, 0, 0, 0, 0,
                        M, N, K, 1, 1, 1.0, 1, None)
                torch.cuda.synchronize()
                if cfg == 7:
                    assert rc != 0 and b"unknown config" in L.psam_last_error_string(), (kernel, rc)
                    continue
                assert rc == 0, (kernel, cfg, L.psam_last_error_string())
                want = _act64(x.double() @ W.double().T + b.double(), 1) + res.double()
                err = ((y.cpu().double() - want).abs() / (x.double().abs() @ W.double().abs().T + 1.0)).max().item()
                if not (torch.isfinite(y).all() and err < 2 * _bar(K)):
                    bad.append((kernel, cfg, (M, N, K), err))
                if N % 64 == 0:
                    Ws, bs, (Wg, Wx, bg, bx) = _swiglu_weights(g, N // 2, K)
                    u = _nan(M, N // 2)
                    rc = fn(xd.data_ptr(), K, 0, 0, Ws.cuda().data_ptr(), K, 0, 0, u.data_ptr(), N // 2, 0, 0, bs.cuda().data_ptr(), None, 0, 0, 0, 0, 0,
                            0, M, N, K, 1, 1, 1.0, 3, None)
                    torch.cuda.synchronize()
                    if not CONFIGS[kernel, cfg].swiglu:
                        assert rc != 0, (kernel, cfg, "SwiGLU not refused")
                        continue
                    assert rc == 0, (kernel, cfg, L.psam_last_error_string())
                    xx = x.double()
                    sw = torch.nn.functional.silu(xx @ Wg.double().T + bg.double()) * (xx @ Wx.double().T + bx.double())
                    err = ((u.cpu().double() - sw).abs() / ((xx.abs() @ Wg.double().abs().T + 1) * (xx.abs() @ Wx.double().abs().T + 1))).max().item()
                    if not err < 4 * _bar(K):
                        bad.append((kernel, cfg, (M, N, K), "swiglu", err))
    finally:
        force(-1)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 6. environment switches, one child each
# the shapes these modes pick: the giant encoder at one cloud (M = 512) and ViT-L at M = 4096 (qkv, SwiGLU fc1, fc2, and a narrow GEMM on the
# eight-wave 128x128 tile that PSAM_GEMM_SUB9 steers)
ENV_SHAPES = {"giant_qkv": (512, 4224, 1408, 0), "giant_proj": (512, 1408, 1408, 0), "giant_fc2": (512, 1408, 6144, 0),
              "vitl_qkv": (4096, 3072, 1024, 0), "vitl_fc1": (4096, 5504, 1024, 3), "vitl_fc2": (4096, 1024, 2752, 0), "vitl_narrow": (4096, 768, 1024, 0)}
ENV_MODES = [("PSAM_GEMM_SMALL_M_RING", "1"), ("PSAM_GEMM_PP", "1"), ("PSAM_GEMM_PP", "3"), ("PSAM_GEMM_PP", "4"), ("PSAM_GEMM_PP", "5"),
             ("PSAM_GEMM_SUB9", "9")]
# what each mode must have run (shape -> allowed configurations); shapes not named only have to give the default's bits
ENV_EXPECT = {
    ("PSAM_GEMM_SMALL_M_RING", "1"): {"giant_qkv": {41, 42}, "giant_proj": {41, 42}, "giant_fc2": {41, 42}},
    ("PSAM_GEMM_PP", "1"): {"vitl_fc1": {55}},
    ("PSAM_GEMM_PP", "3"): {"vitl_qkv": {51}, "vitl_fc1": {55}, "vitl_fc2": {51}, "vitl_narrow": {51}},
    ("PSAM_GEMM_PP", "4"): {"vitl_qkv": {51, 62, 63}, "vitl_fc1": {51, 63}},
    ("PSAM_GEMM_PP", "5"): {"vitl_qkv": {65}},
    ("PSAM_GEMM_SUB9", "9"): {"vitl_narrow": {9}},
}
ENV_DEFAULT = {"vitl_narrow": {28}}      # the default process: the two-per-CU eight-wave tile from M = 2048 (what SUB9 overrides)


def _child_main(path):
    sys.path.insert(0, ROOT)
    import torch as T
    global torch
    torch = T
    from point_sam_amd import ops as o
    o._lib.load()
    res = {}
    for name, (M, N, K, act) in sorted(ENV_SHAPES.items()):
        g = T.Generator().manual_seed(M + N + K)
        x = T.randn(M, K, generator=g) * T.exp(T.randn(M, 1, generator=g))
        W = T.randn(N, K, generator=g) / K ** 0.5
        b = T.randn(N, generator=g) * 0.1
        A, Wp = _pack(o, x.cuda(), K), _pack(o, W.cuda(), K)
        y = _nan(M, N // 2 if act == 3 else N)
        st = f16x3p(o, A, Wp, M, N, K, y, bias=b.cuda(), act=act)
        T.cuda.synchronize()
        res[name] = dict(rc=st[0], cfg=st[1], splitk=st[2], finite=bool(T.isfinite(y).all()),
                         sha=hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest())
    with open(path, "w") as f:
        json.dump(res, f)


def _child(tmp_path, env_set):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PSAM_GEMM_")}
    env.update(env_set)
    out = str(tmp_path / ("child_" + "_".join(f"{k}{v}" for k, v in env_set.items()) + ".json"))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--gemm-config-child", out]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (env_set, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.load(open(out))


@pytest.mark.gpu
def test_environment_switches_in_child_processes(ops, tmp_path):
    """PSAM_GEMM_SMALL_M_RING=1, PSAM_GEMM_PP=1/3/4/5 and PSAM_GEMM_SUB9=9 are read once per process: one fresh child per setting, one after
    another.  Each runs the shapes its mode picks; the configuration it was meant to pick ran, and every output has the default process's bits."""
    base = _child(tmp_path, {})
    for name, r in base.items():
        assert r["rc"] == 0 and r["finite"] and r["splitk"] == 1, (name, r)
    for name, allowed in ENV_DEFAULT.items():
        assert base[name]["cfg"] in allowed, (name, base[name])
    bad = []
    for k, v in ENV_MODES:
        got = _child(tmp_path, {k: v})
        for name, r in got.items():
            if r["rc"] != 0 or not r["finite"]:
                bad.append((k, v, name, r))
            elif name in ENV_EXPECT[k, v] and r["cfg"] not in ENV_EXPECT[k, v][name]:
                bad.append((k, v, name, "ran cfg", r["cfg"], "expected", sorted(ENV_EXPECT[k, v][name])))
            elif r["sha"] != base[name]["sha"]:
                bad.append((k, v, name, "bits differ from the default process", r["cfg"], base[name]["cfg"]))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 7. dispatch pins
# What the default process runs, unforced: (psam_gemm_f16x3p_last_config, psam_gemm_f16x3p_last_splitk) of one launch and psam_gemm_f16x3p_splitk
# of its shape, over the bench model's GEMM shapes (ViT-L qkv / proj / SwiGLU fc1 / fc2 with its padded K, the patch encoder's narrow ones, a ragged N)
# from one row to 64 clouds, each fused extra and split-K requested.  PINS holds the values the library gave before its dispatch became table-driven.
PIN_M = (1, 100, 512, 1000, 2047, 2048, 4096, 32768, 65536)
PIN_NK = ((3072, 1024), (1024, 1024), (5504, 1024), (1024, 2752), (2730, 1024), (256, 128), (512, 256))
PIN_EXTRAS = ("pack", "stats_pack", "ln_fold", "gmax", "hyper", "row_ln", "splitk")


def pin_cases():
    """(M, N, K, act, extra) of every pinned launch; extra None = plain."""
    cases = []
    for M in PIN_M:
        for N, K in PIN_NK:
            cases += [(M, N, K, act, None) for act in ((0, 3) if N % 64 == 0 else (0,))]
            if M % 256 == 0 and N % 128 == 0 and M * N <= 4096 * 5504:
                cases += [(M, N, K, 3 if x == "stats_pack" else 0, x) for x in PIN_EXTRAS if x not in ("row_ln", "splitk")]
            if N == 256 and M % 128 == 0:
                cases.append((M, N, K, 1, "row_ln"))
            if M <= 4096 and N % 4 == 0 and K >= 256:
                cases.append((M, N, K, 0, "splitk"))
    return cases


def _pin_launch(M, N, K, act, extra):
    """One unforced launch on zero operands; returns (config, split factor) the library reports."""
    from point_sam_amd import _lib as Lm
    import torch as T
    dev = "cuda"
    A, W = (T.zeros(M, K, device=dev), T.ones(M, device=dev)), (T.zeros(N, K, device=dev), T.ones(N, device=dev))
    ncol = N // 2 if act == 3 else N
    C = T.empty(M, ncol, device=dev)
    fuse, keep = None, []
    if extra:
        fuse = Lm.GemmFuse()
        new = lambda *shape: keep.append(T.zeros(*shape, device=dev)) or keep[-1].data_ptr()
        if extra in ("pack", "stats_pack"):
            fuse.out_scale, fuse.out_k1, fuse.out_k2, fuse.pack_out = new(M), 1.0, 1.0, 1
        if extra == "stats_pack":
            fuse.stats, fuse.stat_cols = new(M, (N // 2 + 31) // 32, 2), N // 2
        elif extra == "ln_fold":
            fuse.ln_mean, fuse.ln_rstd, fuse.ln_c = new(M), new(M), new(N)
        elif extra == "gmax":
            fuse.gmax_out, fuse.gmax_ld, fuse.gmax_k = new(M // 64, N), N, 64
        elif extra == "hyper":
            Z, c, rows = M // 256, 4, 256
            fuse.hyper, fuse.hyper_c, fuse.hyper_rows = new(Z, c, N), c, rows
            fuse.masks, fuse.hyper_pstride = new(N // 64, Z * c * rows), Z * c * rows
        elif extra == "row_ln":
            fuse.row_ln_g, fuse.row_ln_b, fuse.row_ln_eps = new(N), new(N), 1e-6
        elif extra == "splitk":
            fuse.splitk_ws, fuse.splitk_plane, fuse.splitk = new(2, M * N), M * N, 2
            from point_sam_amd import ops as o
            keep.append(o.new_counters(dev))
            fuse.counters = keep[-1].data_ptr()
    _, cfg, ks = f16x3p(None, A, W, M, N, K, C, act=act, fuse=fuse)
    T.cuda.synchronize()
    return cfg, ks


def dispatch_pins():
    """{"M,N,K,act,extra": (config, split factor, psam_gemm_f16x3p_splitk(M, N, K, act))} over pin_cases()."""
    L = _lib()
    return {",".join(map(str, c)): _pin_launch(*c) + (L.psam_gemm_f16x3p_splitk(*c[:4]),) for c in pin_cases()}


PINS = {      # "M,N,K,act,extra": (config, split factor, psam_gemm_f16x3p_splitk)
    "1,3072,1024,0,None": (9, 1, 4), "1,3072,1024,3,None": (9, 1, 1), "1,3072,1024,0,splitk": (9, 2, 4), "1,1024,1024,0,None": (9, 1, 4),
    "1,1024,1024,3,None": (9, 1, 1), "1,1024,1024,0,splitk": (9, 2, 4), "1,5504,1024,0,None": (9, 1, 4), "1,5504,1024,3,None": (9, 1, 1),
    "1,5504,1024,0,splitk": (9, 2, 4), "1,1024,2752,0,None": (9, 1, 4), "1,1024,2752,3,None": (9, 1, 1), "1,1024,2752,0,splitk": (9, 2, 4),
    "1,2730,1024,0,None": (9, 1, 4), "1,256,128,0,None": (9, 1, 1), "1,256,128,3,None": (9, 1, 1), "1,512,256,0,None": (9, 1, 1),
    "1,512,256,3,None": (9, 1, 1), "1,512,256,0,splitk": (9, 2, 1), "100,3072,1024,0,None": (9, 1, 4), "100,3072,1024,3,None": (9, 1, 1),
    "100,3072,1024,0,splitk": (9, 2, 4), "100,1024,1024,0,None": (9, 1, 4), "100,1024,1024,3,None": (9, 1, 1), "100,1024,1024,0,splitk": (9, 2, 4),
    "100,5504,1024,0,None": (9, 1, 4), "100,5504,1024,3,None": (9, 1, 1), "100,5504,1024,0,splitk": (9, 2, 4), "100,1024,2752,0,None": (9, 1, 4),
    "100,1024,2752,3,None": (9, 1, 1), "100,1024,2752,0,splitk": (9, 2, 4), "100,2730,1024,0,None": (9, 1, 4), "100,256,128,0,None": (9, 1, 1),
    "100,256,128,3,None": (9, 1, 1), "100,512,256,0,None": (9, 1, 1), "100,512,256,3,None": (9, 1, 1), "100,512,256,0,splitk": (9, 2, 1),
    "512,3072,1024,0,None": (9, 1, 1), "512,3072,1024,3,None": (9, 1, 1), "512,3072,1024,0,pack": (9, 1, 1), "512,3072,1024,3,stats_pack": (9, 1, 1),
    "512,3072,1024,0,ln_fold": (9, 1, 1), "512,3072,1024,0,gmax": (14, 1, 1), "512,3072,1024,0,hyper": (21, 1, 1),
    "512,3072,1024,0,splitk": (9, 2, 1), "512,1024,1024,0,None": (9, 1, 4), "512,1024,1024,3,None": (9, 1, 1), "512,1024,1024,0,pack": (9, 1, 4),
    "512,1024,1024,3,stats_pack": (9, 1, 1), "512,1024,1024,0,ln_fold": (9, 1, 4), "512,1024,1024,0,gmax": (14, 1, 4),
    "512,1024,1024,0,hyper": (21, 1, 4), "512,1024,1024,0,splitk": (9, 2, 4), "512,5504,1024,0,None": (9, 1, 1), "512,5504,1024,3,None": (9, 1, 1),
    "512,5504,1024,0,pack": (9, 1, 1), "512,5504,1024,3,stats_pack": (9, 1, 1), "512,5504,1024,0,ln_fold": (9, 1, 1),
    "512,5504,1024,0,gmax": (4, 1, 1), "512,5504,1024,0,hyper": (21, 1, 1), "512,5504,1024,0,splitk": (9, 2, 1), "512,1024,2752,0,None": (9, 1, 4),
    "512,1024,2752,3,None": (9, 1, 1), "512,1024,2752,0,pack": (9, 1, 4), "512,1024,2752,3,stats_pack": (9, 1, 1),
    "512,1024,2752,0,ln_fold": (9, 1, 4), "512,1024,2752,0,gmax": (14, 1, 4), "512,1024,2752,0,hyper": (21, 1, 4),
    "512,1024,2752,0,splitk": (9, 2, 4), "512,2730,1024,0,None": (9, 1, 1), "512,256,128,0,None": (9, 1, 1), "512,256,128,3,None": (9, 1, 1),
    "512,256,128,0,pack": (9, 1, 1), "512,256,128,3,stats_pack": (9, 1, 1), "512,256,128,0,ln_fold": (9, 1, 1), "512,256,128,0,gmax": (14, 1, 1),
    "512,256,128,0,hyper": (21, 1, 1), "512,256,128,1,row_ln": (40, 1, 1), "512,512,256,0,None": (9, 1, 1), "512,512,256,3,None": (9, 1, 1),
    "512,512,256,0,pack": (9, 1, 1), "512,512,256,3,stats_pack": (9, 1, 1), "512,512,256,0,ln_fold": (9, 1, 1), "512,512,256,0,gmax": (14, 1, 1),
    "512,512,256,0,hyper": (21, 1, 1), "512,512,256,0,splitk": (9, 2, 1), "1000,3072,1024,0,None": (9, 1, 1), "1000,3072,1024,3,None": (9, 1, 1),
    "1000,3072,1024,0,splitk": (9, 2, 1), "1000,1024,1024,0,None": (9, 1, 4), "1000,1024,1024,3,None": (9, 1, 1),
    "1000,1024,1024,0,splitk": (9, 2, 4), "1000,5504,1024,0,None": (21, 1, 1), "1000,5504,1024,3,None": (21, 1, 1),
    "1000,5504,1024,0,splitk": (21, 2, 1), "1000,1024,2752,0,None": (9, 1, 4), "1000,1024,2752,3,None": (9, 1, 1),
    "1000,1024,2752,0,splitk": (9, 2, 4), "1000,2730,1024,0,None": (9, 1, 1), "1000,256,128,0,None": (9, 1, 1), "1000,256,128,3,None": (9, 1, 1),
    "1000,512,256,0,None": (9, 1, 1), "1000,512,256,3,None": (9, 1, 1), "1000,512,256,0,splitk": (9, 2, 1), "2047,3072,1024,0,None": (21, 1, 1),
    "2047,3072,1024,3,None": (21, 1, 1), "2047,3072,1024,0,splitk": (21, 2, 1), "2047,1024,1024,0,None": (9, 1, 1),
    "2047,1024,1024,3,None": (9, 1, 1), "2047,1024,1024,0,splitk": (9, 2, 1), "2047,5504,1024,0,None": (23, 1, 1),
    "2047,5504,1024,3,None": (9, 1, 1), "2047,5504,1024,0,splitk": (23, 2, 1), "2047,1024,2752,0,None": (9, 1, 1),
    "2047,1024,2752,3,None": (9, 1, 1), "2047,1024,2752,0,splitk": (9, 2, 1), "2047,2730,1024,0,None": (21, 1, 1), "2047,256,128,0,None": (9, 1, 1),
    "2047,256,128,3,None": (9, 1, 1), "2047,512,256,0,None": (9, 1, 1), "2047,512,256,3,None": (9, 1, 1), "2047,512,256,0,splitk": (9, 2, 1),
    "2048,3072,1024,0,None": (21, 1, 1), "2048,3072,1024,3,None": (21, 1, 1), "2048,3072,1024,0,pack": (21, 1, 1),
    "2048,3072,1024,3,stats_pack": (21, 1, 1), "2048,3072,1024,0,ln_fold": (21, 1, 1), "2048,3072,1024,0,gmax": (21, 1, 1),
    "2048,3072,1024,0,hyper": (21, 1, 1), "2048,3072,1024,0,splitk": (21, 2, 1), "2048,1024,1024,0,None": (28, 1, 4),
    "2048,1024,1024,3,None": (28, 1, 1), "2048,1024,1024,0,pack": (28, 1, 4), "2048,1024,1024,3,stats_pack": (28, 1, 1),
    "2048,1024,1024,0,ln_fold": (28, 1, 4), "2048,1024,1024,0,gmax": (14, 1, 4), "2048,1024,1024,0,hyper": (21, 1, 4),
    "2048,1024,1024,0,splitk": (28, 2, 4), "2048,5504,1024,0,None": (23, 1, 1), "2048,5504,1024,3,None": (28, 1, 1),
    "2048,5504,1024,0,pack": (28, 1, 1), "2048,5504,1024,3,stats_pack": (28, 1, 1), "2048,5504,1024,0,ln_fold": (28, 1, 1),
    "2048,5504,1024,0,gmax": (4, 1, 1), "2048,5504,1024,0,hyper": (21, 1, 1), "2048,5504,1024,0,splitk": (23, 2, 1),
    "2048,1024,2752,0,None": (28, 1, 4), "2048,1024,2752,3,None": (28, 1, 1), "2048,1024,2752,0,pack": (28, 1, 4),
    "2048,1024,2752,3,stats_pack": (28, 1, 1), "2048,1024,2752,0,ln_fold": (28, 1, 4), "2048,1024,2752,0,gmax": (14, 1, 4),
    "2048,1024,2752,0,hyper": (21, 1, 4), "2048,1024,2752,0,splitk": (28, 2, 4), "2048,2730,1024,0,None": (21, 1, 1),
    "2048,256,128,0,None": (28, 1, 1), "2048,256,128,3,None": (28, 1, 1), "2048,256,128,0,pack": (28, 1, 1), "2048,256,128,3,stats_pack": (28, 1, 1),
    "2048,256,128,0,ln_fold": (28, 1, 1), "2048,256,128,0,gmax": (14, 1, 1), "2048,256,128,0,hyper": (21, 1, 1), "2048,256,128,1,row_ln": (40, 1, 1),
    "2048,512,256,0,None": (28, 1, 1), "2048,512,256,3,None": (28, 1, 1), "2048,512,256,0,pack": (28, 1, 1), "2048,512,256,3,stats_pack": (28, 1, 1),
    "2048,512,256,0,ln_fold": (28, 1, 1), "2048,512,256,0,gmax": (14, 1, 1), "2048,512,256,0,hyper": (21, 1, 1), "2048,512,256,0,splitk": (28, 2, 1),
    "4096,3072,1024,0,None": (21, 1, 1), "4096,3072,1024,3,None": (21, 1, 1), "4096,3072,1024,0,pack": (21, 1, 1),
    "4096,3072,1024,3,stats_pack": (21, 1, 1), "4096,3072,1024,0,ln_fold": (21, 1, 1), "4096,3072,1024,0,gmax": (21, 1, 1),
    "4096,3072,1024,0,hyper": (21, 1, 1), "4096,3072,1024,0,splitk": (21, 2, 1), "4096,1024,1024,0,None": (21, 1, 1),
    "4096,1024,1024,3,None": (21, 1, 1), "4096,1024,1024,0,pack": (21, 1, 1), "4096,1024,1024,3,stats_pack": (21, 1, 1),
    "4096,1024,1024,0,ln_fold": (21, 1, 1), "4096,1024,1024,0,gmax": (21, 1, 1), "4096,1024,1024,0,hyper": (21, 1, 1),
    "4096,1024,1024,0,splitk": (21, 2, 1), "4096,5504,1024,0,None": (21, 1, 1), "4096,5504,1024,3,None": (21, 1, 1),
    "4096,5504,1024,0,pack": (21, 1, 1), "4096,5504,1024,3,stats_pack": (21, 1, 1), "4096,5504,1024,0,ln_fold": (21, 1, 1),
    "4096,5504,1024,0,gmax": (21, 1, 1), "4096,5504,1024,0,hyper": (21, 1, 1), "4096,5504,1024,0,splitk": (21, 2, 1),
    "4096,1024,2752,0,None": (21, 1, 1), "4096,1024,2752,3,None": (21, 1, 1), "4096,1024,2752,0,pack": (21, 1, 1),
    "4096,1024,2752,3,stats_pack": (21, 1, 1), "4096,1024,2752,0,ln_fold": (21, 1, 1), "4096,1024,2752,0,gmax": (21, 1, 1),
    "4096,1024,2752,0,hyper": (21, 1, 1), "4096,1024,2752,0,splitk": (21, 2, 1), "4096,2730,1024,0,None": (23, 1, 1),
    "4096,256,128,0,None": (28, 1, 1), "4096,256,128,3,None": (28, 1, 1), "4096,256,128,0,pack": (28, 1, 1), "4096,256,128,3,stats_pack": (28, 1, 1),
    "4096,256,128,0,ln_fold": (28, 1, 1), "4096,256,128,0,gmax": (14, 1, 1), "4096,256,128,0,hyper": (21, 1, 1), "4096,256,128,1,row_ln": (40, 1, 1),
    "4096,512,256,0,None": (28, 1, 1), "4096,512,256,3,None": (28, 1, 1), "4096,512,256,0,pack": (28, 1, 1), "4096,512,256,3,stats_pack": (28, 1, 1),
    "4096,512,256,0,ln_fold": (28, 1, 1), "4096,512,256,0,gmax": (14, 1, 1), "4096,512,256,0,hyper": (21, 1, 1), "4096,512,256,0,splitk": (28, 2, 1),
    "32768,3072,1024,0,None": (21, 1, 1), "32768,3072,1024,3,None": (21, 1, 1), "32768,1024,1024,0,None": (21, 1, 1),
    "32768,1024,1024,3,None": (21, 1, 1), "32768,5504,1024,0,None": (21, 1, 1), "32768,5504,1024,3,None": (21, 1, 1),
    "32768,1024,2752,0,None": (21, 1, 1), "32768,1024,2752,3,None": (21, 1, 1), "32768,2730,1024,0,None": (21, 1, 1),
    "32768,256,128,0,None": (28, 1, 1), "32768,256,128,3,None": (28, 1, 1), "32768,256,128,0,pack": (28, 1, 1),
    "32768,256,128,3,stats_pack": (28, 1, 1), "32768,256,128,0,ln_fold": (28, 1, 1), "32768,256,128,0,gmax": (14, 1, 1),
    "32768,256,128,0,hyper": (21, 1, 1), "32768,256,128,1,row_ln": (40, 1, 1), "32768,512,256,0,None": (21, 1, 1),
    "32768,512,256,3,None": (21, 1, 1), "32768,512,256,0,pack": (21, 1, 1), "32768,512,256,3,stats_pack": (21, 1, 1),
    "32768,512,256,0,ln_fold": (21, 1, 1), "32768,512,256,0,gmax": (21, 1, 1), "32768,512,256,0,hyper": (21, 1, 1),
    "65536,3072,1024,0,None": (21, 1, 1), "65536,3072,1024,3,None": (21, 1, 1), "65536,1024,1024,0,None": (21, 1, 1),
    "65536,1024,1024,3,None": (21, 1, 1), "65536,5504,1024,0,None": (21, 1, 1), "65536,5504,1024,3,None": (21, 1, 1),
    "65536,1024,2752,0,None": (21, 1, 1), "65536,1024,2752,3,None": (21, 1, 1), "65536,2730,1024,0,None": (21, 1, 1),
    "65536,256,128,0,None": (21, 1, 1), "65536,256,128,3,None": (21, 1, 1), "65536,256,128,0,pack": (21, 1, 1),
    "65536,256,128,3,stats_pack": (21, 1, 1), "65536,256,128,0,ln_fold": (21, 1, 1), "65536,256,128,0,gmax": (21, 1, 1),
    "65536,256,128,0,hyper": (21, 1, 1), "65536,256,128,1,row_ln": (40, 1, 1), "65536,512,256,0,None": (21, 1, 1),
    "65536,512,256,3,None": (21, 1, 1),
}


@pytest.mark.gpu
def test_dispatch_pins(ops):
    """Every pinned launch runs the configuration and split factor it ran before, and the split-K suggestion for its shape is unchanged."""
    got = dispatch_pins()
    assert set(got) == set(PINS), set(got) ^ set(PINS)
    bad = {k: (v, PINS[k]) for k, v in got.items() if v != PINS[k]}
    assert not bad, bad


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--gemm-config-child":
    _child_main(sys.argv[2])
