"""Every launchable row-kernel and patch-layer instance, checked on its own.

csrc/rowops.hip ships the memory-bound kernels every forward pass runs -- LayerNorm (`layernorm_kernel<NREG>` for rows that are not 16-byte aligned or not
256 .. 4096 columns wide, `layernorm_v4_kernel<NV4>` otherwise, the latter also with a g8-packed output and a per-row bound), the SwiGLU gate with its inner
LayerNorm (`swiglu_ln_kernel<NREG>`), the 3-NN interpolation (`interp3_kernel`, `interp3_c256_kernel<4>`), group max and `add_bcast` -- and csrc/tokenizer.hip
the neighbourhood gather and the first mini-PointNet layer fused with it (`patch_l1_kernel<CIN, CENTRAL, PACK>`).  INSTANCES lists every template instance
with the code its family's `*_last_instance` query reports and how it is reached; a CPU test keeps it equal to the launch sites of the sources (the
LN_LAUNCH / LNV_LAUNCH / SG_LAUNCH / L1_LAUNCH macros expanded) and the dispatch thresholds equal to the ones the cases are built around, so an instance added
or a threshold moved later fails without a GPU.  On the GPU every entry is forced by shape, stride or alignment, run, and confirmed to have run as itself:
  * against an fp64 evaluation on the CPU of the same fp32 inputs, at the project's bounds for these kernels (2e-5; 1e-5 for the interpolation);
  * into buffers with guard rows (and guard columns where the row stride exceeds the row) that must keep their sentinel;
  * packed outputs decoded against fp64 AND bit for bit against pack_rows_g8(y, row_scale_f16(y)) of the same call's unpacked output y;
  * at both sides of every dispatch threshold, at odd row counts (clamped tails), above one pass of the grid-stride loop and with ragged last float4s.
The last test asserts that the run confirmed every code of the registry at least once (it needs the other GPU tests of this file in the same session)."""
import os
import re
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

from oracle import pointsam_oracle as O
import g8_reference
from g8_reference import unpack_g8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "point_sam_amd", "csrc")
gpu = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------ 1. the registry
# family: ln | swiglu | patch_l1 | interp3 (one `psam_<family>_last_instance` query each).  codes: what the query reports after this instance ran (the float4
# LayerNorm reports + 100 when it wrote the packed form: a runtime flag of the same instance).  reach: how a test gets it.
Inst = namedtuple("Inst", "family file codes reach")
INSTANCES = {
    "layernorm_kernel<2>": Inst("ln", "rowops.hip", (2,), "cols <= 128"),
    "layernorm_kernel<4>": Inst("ln", "rowops.hip", (4,), "128 < cols <= 256, a stride % 4 != 0 or a pointer % 16 != 0"),
    "layernorm_kernel<8>": Inst("ln", "rowops.hip", (8,), "256 < cols <= 512, unaligned"),
    "layernorm_kernel<16>": Inst("ln", "rowops.hip", (16,), "512 < cols <= 1024, unaligned"),
    "layernorm_kernel<44>": Inst("ln", "rowops.hip", (44,), "1024 < cols <= 2816, unaligned"),
    "layernorm_kernel<0>": Inst("ln", "rowops.hip", (0,), "cols > 4096, or 2816 < cols unaligned (streaming)"),
    "layernorm_v4_kernel<1>": Inst("ln", "rowops.hip", (1001, 1101), "aligned, span <= 256 (span = cols, packed: cols rounded up to 32)"),
    "layernorm_v4_kernel<2>": Inst("ln", "rowops.hip", (1002, 1102), "aligned, 256 < span <= 512"),
    "layernorm_v4_kernel<4>": Inst("ln", "rowops.hip", (1004, 1104), "aligned, 512 < span <= 1024"),
    "layernorm_v4_kernel<8>": Inst("ln", "rowops.hip", (1008, 1108), "aligned, 1024 < span <= 2048"),
    "layernorm_v4_kernel<16>": Inst("ln", "rowops.hip", (1016, 1116), "aligned, 2048 < span <= 4096"),
    "swiglu_ln_kernel<8>": Inst("swiglu", "rowops.hip", (8,), "H <= 512"),
    "swiglu_ln_kernel<32>": Inst("swiglu", "rowops.hip", (32,), "512 < H <= 2048"),
    "swiglu_ln_kernel<44>": Inst("swiglu", "rowops.hip", (44,), "2048 < H <= 2816"),
    "swiglu_ln_kernel<0>": Inst("swiglu", "rowops.hip", (0,), "H > 2816 (streaming through `out`)"),
    "patch_l1_kernel<4,false,false>": Inst("patch_l1", "tokenizer.hip", (40,), "C == 1"),
    "patch_l1_kernel<4,false,true>": Inst("patch_l1", "tokenizer.hip", (41,), "C == 1, scale_out"),
    "patch_l1_kernel<5,true,false>": Inst("patch_l1", "tokenizer.hip", (50,), "C == 1, center_idx"),
    "patch_l1_kernel<5,true,true>": Inst("patch_l1", "tokenizer.hip", (51,), "C == 1, center_idx, scale_out"),
    "patch_l1_kernel<6,false,false>": Inst("patch_l1", "tokenizer.hip", (60,), "C == 3"),
    "patch_l1_kernel<6,false,true>": Inst("patch_l1", "tokenizer.hip", (61,), "C == 3, scale_out"),
    "patch_l1_kernel<9,true,false>": Inst("patch_l1", "tokenizer.hip", (90,), "C == 3, center_idx"),
    "patch_l1_kernel<9,true,true>": Inst("patch_l1", "tokenizer.hip", (91,), "C == 3, center_idx, scale_out"),
    "interp3_kernel": Inst("interp3", "rowops.hip", (0,), "C != 256"),
    "interp3_c256_kernel<4>": Inst("interp3", "rowops.hip", (256,), "C == 256"),
}
KERNELS = ("layernorm_kernel", "layernorm_v4_kernel", "swiglu_ln_kernel", "patch_l1_kernel", "interp3_kernel", "interp3_c256_kernel")
QUERIES = ("psam_layernorm_last_instance", "psam_swiglu_ln_last_instance", "psam_patch_l1_last_instance", "psam_interp3_last_instance")
# the dispatchers' threshold chains, (largest size served, template argument), None = everything above: what the shapes below sit on both sides of
LN_CHAIN = [(128, 2), (256, 4), (512, 8), (1024, 16), (2816, 44), (None, 0)]
LNV_CHAIN = [(256, 1), (512, 2), (1024, 4), (2048, 8), (None, 16)]
SG_CHAIN = [(512, 8), (2048, 32), (2816, 44), (None, 0)]


def _pick(chain, n):
    return next(arg for lim, arg in chain if lim is None or n <= lim)


def _kpad(cols):
    return (cols + 31) // 32 * 32


def ln_code(cols, vec, pack=False):
    """psam_layernorm_ex2's dispatch: the float4 kernel by its span (the packed form also writes the zero padding of the 32-k slab), else the scalar one."""
    if vec:
        assert 256 <= cols <= 4096
        return 1000 + _pick(LNV_CHAIN, _kpad(cols) if pack else cols) + (100 if pack else 0)
    return _pick(LN_CHAIN, cols)


def swiglu_code(H):
    return _pick(SG_CHAIN, H)


def patch_code(C, central, pack):
    return (3 + C * (2 if central else 1)) * 10 + int(pack)


# ------------------------------------------------------------------------------------------------ source parsing (CPU)
def _split_args(s):
    """Top-level comma split of a macro argument list."""
    out, depth, cur = [], 0, ""
    for ch in s:
        depth += {"(": 1, "<": 0, ")": -1}.get(ch, 0)
        if ch == "," and depth == 0:
            out.append(cur.strip()); cur = ""
        else:
            cur += ch
    return out + [cur.strip()] if cur.strip() or out else []


def expand_macros(src):
    """The source with its own function-like macros expanded in preprocessor order (#define ... #undef; line continuations joined; comments dropped):
    every `LN_LAUNCH(8);` becomes the hipLaunchKernelGGL it stands for, also through a macro that uses another (L1_PICK -> L1_LAUNCH)."""
    src = re.sub(r"//[^\n]*", "", src).replace("\\\n", " ")
    macros, out = {}, []

    def expand(line, depth=0):
        assert depth < 8, line
        for name, (params, body) in macros.items():
            while True:
                m = re.search(r"\b%s\(" % name, line)
                if not m:
                    break
                level, k = 1, m.end()
                while level:
                    assert k < len(line), f"unbalanced use of {name}: {line!r}"
                    level += {"(": 1, ")": -1}.get(line[k], 0)
                    k += 1
                args = _split_args(line[m.end():k - 1])
                assert len(args) == len(params), (name, args, params)
                text = body
                for p, a in zip(params, args):
                    text = re.sub(r"\b%s\b" % p, a, text)
                line = line[:m.start()] + text + line[k:]
        return expand(line, depth + 1) if any(re.search(r"\b%s\(" % n, line) for n in macros) else line

    for line in src.splitlines():
        m = re.match(r"\s*#\s*define\s+(\w+)\(([^)]*)\)\s+(.*)", line)
        if m:
            macros[m.group(1)] = (_split_args(m.group(2)), m.group(3))
            continue
        m = re.match(r"\s*#\s*undef\s+(\w+)", line)
        if m:
            macros.pop(m.group(1), None)
            continue
        out.append(expand(line))
    return "\n".join(out)


def launched_instances(src, kernels=KERNELS):
    """{"patch_l1_kernel<9,true,false>", ...}: the instantiations of `kernels` named at the hipLaunchKernelGGL sites of the macro-expanded source, spelled
    without blanks.  A template argument that is a name (`constexpr int R = 4;` before the launch) is replaced by its value."""
    text = expand_macros(src)
    found = set()
    for m in re.finditer(r"hipLaunchKernelGGL\(\s*\(?\s*([A-Za-z_]\w*_kernel)\s*(<[^<>()]*>)?", text):
        if m.group(1) not in kernels:
            continue
        args = [a.strip() for a in (m.group(2) or "<>")[1:-1].split(",") if a.strip()]
        for i, a in enumerate(args):
            if re.fullmatch(r"[A-Za-z_]\w*", a) and a not in ("true", "false"):
                vals = re.findall(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % a, text[:m.start()])
                assert vals, f"template argument {a} of {m.group(1)} has no constexpr value before its launch"
                args[i] = vals[-1]
        found.add(m.group(1) + ("<" + ",".join(args) + ">" if args else ""))
    return found


def dispatch_chain(src, macro, var):
    """[(limit, template argument), ..., (None, argument)] of the first `if (var <= limit) MACRO(arg); else if ... else MACRO(arg);` chain of the source."""
    text = re.sub(r"//[^\n]*", "", src)
    first = re.search(r"if \(%s <= ([\d *]+)\) %s\((\d+)\);" % (var, macro), text)
    assert first, (macro, var)
    chain, pos = [(eval(first.group(1)), int(first.group(2)))], first.end()
    while True:
        m = re.match(r"\s*else if \(%s <= ([\d *]+)\) %s\((\d+)\);" % (var, macro), text[pos:])
        if not m:
            break
        chain.append((eval(m.group(1)), int(m.group(2))))
        pos += m.end()
    last = re.match(r"\s*else %s\((\d+)\);" % macro, text[pos:])
    assert last, (macro, "chain without a final else")
    return chain + [(None, int(last.group(1)))]


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def source_instances(rowops_src, tokenizer_src):
    return {**{k: "rowops.hip" for k in launched_instances(rowops_src)}, **{k: "tokenizer.hip" for k in launched_instances(tokenizer_src)}}


def test_registry_matches_the_launch_sites():
    """INSTANCES == the instantiations of the six kernels that csrc/rowops.hip and csrc/tokenizer.hip launch (macros expanded; the repeat launch of the
    ablation build names the same set); the dispatch thresholds are the ones the cases are built around; the codes follow the documented rule; the header
    declares the four queries and the Python binding knows them."""
    row, tok = _read("rowops.hip"), _read("tokenizer.hip")
    got, want = source_instances(row, tok), {k: i.file for k, i in INSTANCES.items()}
    assert got == want, (sorted(set(got) ^ set(want)), "launched by the sources vs listed in INSTANCES")
    assert dispatch_chain(row, "LN_LAUNCH", "cols") == LN_CHAIN
    assert dispatch_chain(row, "LNV_LAUNCH", "span") == LNV_CHAIN
    assert dispatch_chain(row, "SG_LAUNCH", "H") == SG_CHAIN
    assert "const int span = pack ? kpad32(cols) : cols;" in row and "int kpad32(int k) { return (k + 31) & ~31; }" in _read("g8_pack.h")
    assert "if (C == 256) {" in re.sub(r"\s+", " ", row[row.index("PSAM_API int32_t psam_interp3_ex("):])
    for k, i in INSTANCES.items():
        args = k[k.index("<") + 1:-1].split(",") if "<" in k else []
        if k.startswith("layernorm_kernel") or k.startswith("swiglu_ln_kernel"):
            assert i.codes == (int(args[0]),), k
        elif k.startswith("layernorm_v4_kernel"):
            assert i.codes == (1000 + int(args[0]), 1100 + int(args[0])), k
        elif k.startswith("patch_l1_kernel"):
            assert i.codes == (int(args[0]) * 10 + (args[2] == "true"),) and (args[1] == "true") == (int(args[0]) in (5, 9)), k
        else:
            assert i.codes == ((256,) if "c256" in k else (0,)), k
    from point_sam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pointsam_hip.h")).read()
    for name in QUERIES:
        assert re.search(r"int32_t\s+%s\s*\(\s*void\s*\)\s*;" % name, hdr), name
        assert name in _lib.SIGNATURES, name
        src = tok if "patch_l1" in name else row
        assert re.search(r"PSAM_API int32_t %s\(void\)" % name, src), name


def test_the_parser_sees_an_edited_launch_site():
    """The registry test must fail when a launch site is added or edited, through a macro or directly, and when an entry leaves the registry."""
    row, tok = _read("rowops.hip"), _read("tokenizer.hip")
    base = set(INSTANCES)
    assert set(source_instances(row, tok)) == base
    site = "    if (cols <= 128) LN_LAUNCH(2);"
    assert row.count(site) == 1
    assert set(source_instances(row.replace(site, "    if (cols <= 64) LN_LAUNCH(1);\n    else if (cols <= 128) LN_LAUNCH(2);"), tok)) - base == {"layernorm_kernel<1>"}
    assert set(source_instances(row.replace("else LNV_LAUNCH(16);", "else LNV_LAUNCH(32);"), tok)) ^ base == {"layernorm_v4_kernel<16>", "layernorm_v4_kernel<32>"}
    assert set(source_instances(row.replace("else if (H <= 44 * 64) SG_LAUNCH(44);", ""), tok)) ^ base == {"swiglu_ln_kernel<44>"}
    assert set(source_instances(row.replace("constexpr int R = 4;\n        hipLaunchKernelGGL(interp3_c256_kernel<R>", "constexpr int R = 2;\n        hipLaunchKernelGGL(interp3_c256_kernel<R>"),
                                tok)) ^ base == {"interp3_c256_kernel<4>", "interp3_c256_kernel<2>"}
    assert set(source_instances(row, tok.replace("L1_LAUNCH(9, true, PK)", "L1_LAUNCH(12, true, PK)"))) ^ base == \
        {"patch_l1_kernel<9,true,false>", "patch_l1_kernel<9,true,true>", "patch_l1_kernel<12,true,false>", "patch_l1_kernel<12,true,true>"}
    assert set(source_instances(row, tok.replace("if (scale_out) L1_PICK(true); else L1_PICK(false);", "L1_PICK(false);"))) ^ base == \
        {k for k in base if k.startswith("patch_l1_kernel") and k.endswith("true>")}
    assert dispatch_chain(row.replace("else if (cols <= 2816) LN_LAUNCH(44);", "else if (cols <= 3072) LN_LAUNCH(48);"), "LN_LAUNCH", "cols") != LN_CHAIN


def test_queries_report_minus_one_before_a_launch_and_after_a_refusal():
    """No GPU needed: a thread that never launched reads -1 from the four queries, and so does one whose call was refused on the host (null pointers)."""
    import threading
    from point_sam_amd import _lib
    lib = _lib.load()
    seen = []
    t = threading.Thread(target=lambda: seen.extend(getattr(lib, q)() for q in QUERIES))
    t.start(); t.join()
    assert seen == [-1, -1, -1, -1]
    assert lib.psam_layernorm_ex2(None, 0, None, 0, None, None, None, 0, 1, 256, 1e-5, 0, None, 0, None, 0.0, 0.0, 0.0, None) != 0
    assert lib.psam_swiglu_ln(None, 0, 0, None, None, None, 0, 1, 1, 1e-5, None) != 0
    assert lib.psam_patch_l1_ex(None, None, None, None, None, None, None, None, None, 1e-5, 1, 1, 1, 1, 1, 1, 0.0, None, None, None) != 0
    assert lib.psam_interp3_ex(None, None, None, None, 1, 1, 1, 1, 256, None, None, None, 0.0, 0, None) != 0
    assert [getattr(lib, q)() for q in QUERIES] == [-1, -1, -1, -1]


# ------------------------------------------------------------------------------------------------ the cases
# patch_l1 / group_gather: (B, rep, N, G, K).  15 rows: odd, the two-rows-per-wave clamp; 378 rows with rep > 1; 65869 rows: odd and above the
# 8192 blocks x 4 waves x 2 rows = 65536 rows of one pass, so the grid-stride loop and the clamp happen together.
PATCH_SHAPES = [(1, 1, 97, 3, 5), (2, 3, 500, 7, 9), (1, 1, 4096, 331, 199)]
PATCH_CASES = [(s, C, central, radius) for s in range(len(PATCH_SHAPES)) for C in (1, 3) for central in (False, True) for radius in (None, 0.1)]
GATHER_CASES = [(s, C) for s in range(len(PATCH_SHAPES)) for C in (1, 3, 128)]
GATHER_REPS, GATHER_RADII = (1, 3), (None, 0.1, 0.25)

# LayerNorm, scalar kernel: (cols, how).  "strided": a [:, :cols] view of a buffer with row stride cols + 1 (x and out; the residual cols + 3);
# "contiguous": ld == cols (narrower than 256 or wider than 4096: never the float4 kernel); "offset": strides % 4 == 0, x starts one float into its buffer.
# Both sides of every threshold of LN_CHAIN; 2817 (strided), 4097 and 5000 stream.
LN_SCALAR_CASES = [(c, "strided") for c in (128, 129, 256, 257, 512, 513, 1024, 1025, 2816, 2817)] + [(64, "contiguous"), (4097, "contiguous"),
                                                                                                       (5000, "contiguous"), (512, "offset")]
LN_ROWS = (1, 37)
# float4 kernel: (cols, ld).  Both sides of every threshold of LNV_CHAIN; ragged last float4 (ld = cols rounded up to 4), 4093 on <16>'s last slot.
LN_V4_CASES = [(c, c) for c in (256, 260, 512, 516, 1024, 1028, 2048, 2052, 4096)] + [(257, 260), (1021, 1024), (4093, 4096)]
LN_PACKED_CASES = [(256, 256), (512, 512), (1024, 1024), (1408, 1408)]      # <1>, <2>, <4>, <8>; <16>: the bound cases (and test_layernorm_packed_output)
LN_BOUND_CASES = [(256, 256), (1408, 1408), (2730, 2752)]
LN_BOUND_COEFFS = [(0.0, 3.5, 0.25), (0.02, 1.5, 0.0)]      # (c2, c1, c0) >= 0, the first all-linear

SWIGLU_H = (170, 512, 513, 2048, 2049, 2816, 2817, 4090)
SWIGLU_ROWS = (1, 9)

INTERP_G = 20
INTERP_GENERIC_C = (64, 128, 320, 512)      # 320: the second trip of the 256-column loop with idle lanes
INTERP_SHAPES = [(1, 1, 1), (3, 101, 3), (2, 6, 1), (4, 300, 2)]      # (Z, N, rep): 1, 303, 12, 1200 rows -> tails of 1, 3, 0, 0 rows of the 4-row wave
INTERP_FIVE_ROWS = (1, 5, 1)      # a full wave, then a second one that holds one row and three clamped duplicates (computed, exchanged, not stored)


def test_cases_reach_every_instance():
    """The case tables, through the dispatch rules above, name every code of the registry (the GPU tests assert that each case ran as predicted)."""
    codes = {("ln", ln_code(c, False)) for c, _ in LN_SCALAR_CASES}
    codes |= {("ln", ln_code(c, True)) for c, _ in LN_V4_CASES}
    codes |= {("ln", ln_code(c, True, True)) for c, _ in LN_PACKED_CASES + LN_BOUND_CASES}
    codes |= {("swiglu", swiglu_code(H)) for H in SWIGLU_H}
    codes |= {("patch_l1", patch_code(C, central, pack)) for _, C, central, _ in PATCH_CASES for pack in (False, True)}
    codes |= {("interp3", 0), ("interp3", 256)}
    assert codes == {(i.family, c) for i in INSTANCES.values() for c in i.codes}
    for chain, sizes in ((LN_CHAIN, [c for c, how in LN_SCALAR_CASES if how == "strided"]), (LNV_CHAIN, [c for c, ld in LN_V4_CASES if c == ld]), (SG_CHAIN, SWIGLU_H)):
        for lim, _ in chain[:-1]:
            assert lim in sizes and (lim + 1 in sizes or (chain is LNV_CHAIN and lim + 4 in sizes)), (lim, "both sides of the threshold")
    rows = [B * rep * G * K for B, rep, _, G, K in PATCH_SHAPES]
    assert rows == [15, 378, 65869] and rows[0] % 2 == 1 and rows[2] % 2 == 1 and rows[2] > 8192 * 4 * 2
    assert [Z * N % 4 for Z, N, _ in INTERP_SHAPES] == [1, 3, 0, 0]


# ------------------------------------------------------------------------------------------------ GPU plumbing
@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd import ops as _ops
    _ops._lib.load()
    return _ops


SENTINEL = -7.25      # what buffers hold where no kernel may write
SEEN = set()          # (family, code) confirmed by a `last_instance` query after a launch
WORST = {}            # family -> largest |kernel - fp64| seen, printed by the last test


def _confirm(ops, family, code, what=""):
    query = {"ln": "psam_layernorm_last_instance", "swiglu": "psam_swiglu_ln_last_instance", "patch_l1": "psam_patch_l1_last_instance",
             "interp3": "psam_interp3_last_instance"}[family]
    ran = getattr(ops._lib.load(), query)()
    assert ran == code, f"{what}: expected {family} instance {code}, the library ran {ran}"
    SEEN.add((family, code))


def _err(got, want, atol, family, what, rowmax_term=0.0):
    """Largest |got - want| (fp64), printed, recorded and asserted <= atol (+ rowmax_term x the row's largest |want|)."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    err = (got - want).abs()
    tol = atol + rowmax_term * want.abs().amax(dim=-1, keepdim=True)
    worst = err.max().item()
    WORST[family] = max(WORST.get(family, 0.0), worst)
    print(f"| {what} | {worst:.2e} | {atol:.0e}{' + 2^-21 rowmax' if rowmax_term else ''} | max abs ref {want.abs().max().item():.3g} |")
    assert torch.isfinite(got).all() and not (err > tol).any(), f"{what}: {int((err > tol).sum())}/{err.numel()} above tolerance, max abs err {worst:.3e}"
    return worst


class Guarded:
    """A [rows, cols] window with row stride ld at float offset `off` of a SENTINEL-filled buffer that also holds `extra` guard rows; untouched() asserts
    everything outside the window (padding columns, guard rows, the floats before it) still holds the sentinel."""

    def __init__(self, rows, cols, ld=None, extra=2, off=0, fill=None):
        ld = cols if ld is None else ld
        self.flat = torch.full((off + (rows + extra) * ld,), SENTINEL, device="cuda")
        self.all = self.flat[off:].view(rows + extra, ld)
        self.win = self.all[:rows, :cols]
        self.rows, self.cols = rows, cols
        if fill is not None:
            self.win.copy_(fill)

    def untouched(self, what=""):
        g = self.flat.clone()
        g[self.flat.numel() - self.all.numel():].view_as(self.all)[:self.rows, :self.cols] = SENTINEL
        assert (g == SENTINEL).all(), f"{what}: {int((g != SENTINEL).sum())} floats outside the output window were written"


def _same_words(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _packed_is_the_packing_of(ops, words, scales, y, what):
    """Assertion 2 of the packed outputs: scales == row_scale_f16(y) and words == pack_rows_g8(y, scales), bit for bit.  Prints what differs before asserting."""
    want_s = ops.row_scale_f16(y)
    want_w = ops.pack_rows_g8(y, want_s)
    nw = int((words.contiguous().view(torch.int32) != want_w.view(torch.int32)).sum())
    ns = int((scales != want_s).sum())
    print(f"| {what} | words differing {nw}/{want_w.numel()} | scales differing {ns}/{want_s.numel()} |")
    assert ns == 0, f"{what}: {ns} row scales differ from row_scale_f16 of the unpacked output"
    assert nw == 0, f"{what}: {nw} packed words differ from pack_rows_g8 of the unpacked output"
    _is_the_host_packing_of(words, scales, y, what)


def _is_the_host_packing_of(words, scales, y, what):
    """The same two equalities against tests/g8_reference.py: torch on the CPU, no device code of the project in the expectation."""
    host_s = g8_reference.row_scale_f16(y)
    host_w = g8_reference.pack_g8(y, host_s)
    nw = int((words.contiguous().view(torch.int32).cpu() != host_w).sum())
    ns = int((scales.cpu() != host_s).sum())
    print(f"| {what}, host packer | words differing {nw}/{host_w.numel()} | scales differing {ns}/{host_s.numel()} |")
    assert ns == 0, f"{what}: {ns} row scales differ from g8_reference.row_scale_f16 of the unpacked output"
    assert nw == 0, f"{what}: {nw} packed words differ from g8_reference.pack_g8 of the unpacked output"


def _one_ulp(a, b):
    """Every element of fp32 a equals b or one of b's two fp32 neighbours."""
    inf = torch.full_like(b, float("inf"))
    return bool(((a == b) | (a == torch.nextafter(b, inf)) | (a == torch.nextafter(b, -inf))).all())


# ------------------------------------------------------------------------------------------------ 3. patch_l1 and group_gather
def _patch_inputs(shape, C, seed):
    """Random clouds, random neighbour / centre indices in [0, N) with kidx[:, :, 0] = center_idx (the zero-offset row), centres = the centre points."""
    B, rep, N, G, K = shape
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(B, N, 3, generator=g) * 2 - 1
    feats = torch.randn(B * rep, N, C, generator=g)
    cidx = torch.randint(0, N, (B, G), generator=g)
    kidx = torch.randint(0, N, (B, G, K), generator=g)
    kidx[:, :, 0] = cidx
    centers = O.batch_index_select(xyz, cidx)
    return g, xyz, feats, centers, kidx, cidx


def _rep(t, rep):
    return t.repeat_interleave(rep, 0) if rep > 1 else t


@gpu
@pytest.mark.parametrize("s,C,central,radius", PATCH_CASES, ids=lambda v: str(v))
def test_patch_l1_instances(ops, s, C, central, radius):
    """patch_l1_kernel<3 + C (+ C), central, PACK> for PACK = false and true on one case, each confirmed by psam_patch_l1_last_instance.
    Unpacked: within 2e-5 (the project's bound for this kernel) of GELU(LayerNorm(Linear(group_points(...)))) in fp64.  Packed: (1) decoded within
    2e-5 + 2^-21 x the row maximum of fp64; (2) scales and words == pack_rows_g8(y, row_scale_f16(y)) of the unpacked output y of the same case, bit for bit
    (the two instantiations do the same arithmetic up to the split).  Guard rows of `out` and `scale_out` keep their sentinel."""
    shape = PATCH_SHAPES[s]
    B, rep, N, G, K = shape
    g, xyz, feats, centers, kidx, cidx = _patch_inputs(shape, C, seed=100 * s + 10 * C + central)
    cin = 3 + C * (2 if central else 1)
    W = torch.randn(128, cin, generator=g) * 0.5
    b, lw, lb = torch.randn(128, generator=g) * 0.1, 1 + 0.1 * torch.randn(128, generator=g), 0.1 * torch.randn(128, generator=g)
    grouped = O.group_points(_rep(xyz, rep).double(), feats.double(), _rep(centers, rep).double(), _rep(kidx, rep), radius, _rep(cidx, rep) if central else None)
    pre = F.linear(grouped, W.double(), b.double()).reshape(-1, 128)
    ref = F.gelu(F.layer_norm(pre, (128,), lw.double(), lb.double(), 1e-5))
    rows = B * rep * G * K
    assert ref.shape == (rows, 128)
    what = f"patch_l1 C={C} central={central} radius={radius} rows={rows}"
    print(f"\n{what}: smallest pre-LN row std {pre.std(dim=1, unbiased=False).min().item():.3g}")
    dev = [t.cuda().contiguous() for t in (xyz, feats, centers, kidx, W, b, lw, lb)]
    cdev = cidx.cuda() if central else None
    out = Guarded(rows, 128)
    ops.patch_l1(*dev, 1e-5, out=out.win, radius=radius, center_idx=cdev)
    _confirm(ops, "patch_l1", patch_code(C, central, False), what)
    out.untouched(what)
    _err(out.win, ref, 2e-5, "patch_l1", what)
    pk, sc = Guarded(rows, 128), Guarded(rows, 1)
    ops.patch_l1(*dev, 1e-5, out=pk.win, radius=radius, center_idx=cdev, scale_out=sc.win)
    _confirm(ops, "patch_l1", patch_code(C, central, True), what + " packed")
    pk.untouched(what + " packed"); sc.untouched(what + " scales")
    scales = sc.win[:, 0].contiguous()
    _err(unpack_g8(pk.win, scales, 128), ref, 2e-5, "patch_l1 packed", what + " packed, decoded", rowmax_term=2.0 ** -21)
    _packed_is_the_packing_of(ops, pk.win, scales, out.win, what + " packed")


@gpu
@pytest.mark.parametrize("s,C", GATHER_CASES, ids=lambda v: str(v))
def test_group_gather_radius_width_rep(ops, s, C):
    """group_gather_kernel over rep in {1, 3} x radius in {none, 0.1, 0.25} x row width in {3 + C, the next multiple of 4, 3 + C + 5}: the feature
    columns equal the oracle's, the padding columns are exactly 0, guard rows are untouched.  Relative coordinates: without radius equal to the oracle's;
    with radius bit-equal to the kernel's stated `(p - c) * (1.0f / radius)` evaluated in fp32 and at most 1 ulp from the oracle's division (for 0.25,
    a power of two, equal to it)."""
    B, _, N, G, K = PATCH_SHAPES[s]
    lib = ops._lib.load()
    for rep in GATHER_REPS:
        g, xyz, feats, centers, kidx, _ = _patch_inputs((B, rep, N, G, K), C, seed=1000 + 100 * s + C + rep)
        xr, cr, kr = _rep(xyz, rep), _rep(centers, rep), _rep(kidx, rep)
        want = O.group_points(xr, feats, cr, kr).reshape(-1, 3 + C)
        rows = B * rep * G * K
        want_f = want[:, 3:].cuda()
        dev = [t.cuda().contiguous() for t in (xyz, feats, centers, kidx)]
        for radius in GATHER_RADII:
            oracle = want[:, :3] if radius is None else O.group_points(xr, feats[..., :1], cr, kr, radius).reshape(-1, 4)[:, :3]
            spec = want[:, :3] if radius is None else want[:, :3] * (torch.tensor(1.0) / torch.tensor(radius, dtype=torch.float32))
            for width in sorted({3 + C, (3 + C + 3) // 4 * 4, 3 + C + 5}):
                what = f"group_gather rows={rows} C={C} rep={rep} radius={radius} width={width}"
                out = Guarded(rows, width)
                rc = lib.psam_group_gather_ld(*(t.data_ptr() for t in dev), B, rep, N, G, K, C, float(radius or 0.0), out.win.data_ptr(), width,
                                              torch.cuda.current_stream().cuda_stream)
                assert rc == 0, what
                out.untouched(what)
                assert torch.equal(out.win[:, 3:3 + C], want_f), what + ": feature columns"
                assert (out.win[:, 3 + C:] == 0).all(), what + ": padding columns"
                rel = out.win[:, :3].cpu()
                assert torch.equal(rel, spec), what + ": relative coordinates vs (p - c) * (1.0f / radius) in fp32"
                assert _one_ulp(rel, oracle), what + ": more than 1 ulp from the oracle's division"
                if radius in (None, 0.25):
                    assert torch.equal(rel, oracle), what
            if radius is not None and width == 3 + C + 5:
                print(f"| {what} | elements that differ from the division: {(spec != oracle).float().mean().item():.3f} |")
        # the wrapper: same kernel, the buffer is its own
        got = ops.group_gather(*dev, radius=0.25, width=3 + C + 5)
        assert got.shape == (B * rep, G, K, 3 + C + 5) and torch.equal(got.view(rows, -1)[:, :3].cpu(), oracle) and (got[..., 3 + C:] == 0).all()


# ------------------------------------------------------------------------------------------------ 3. LayerNorm
def _ln_inputs(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    x, r = torch.randn(rows, cols, generator=g) * 3 + 1, torch.randn(rows, cols, generator=g)
    w, b = 1 + 0.1 * torch.randn(cols, generator=g), 0.1 * torch.randn(cols, generator=g)
    return x, r, w, b


def _ln_both_forms(ops, rows, cols, ld, ldr, vec, off=0, inplace=False, tag=""):
    """Plain LayerNorm, then LayerNorm(x + residual) + GELU + scale_out, on [rows, cols] windows with row stride ld (residual: ldr; x starts `off` floats
    into its buffer): the predicted instance ran, guards untouched, within 2e-5 of fp64, scale_out == row_scale_f16(output) exactly."""
    x, r, w, b = _ln_inputs(rows, cols, seed=cols * 10 + rows)
    wd, bd = w.cuda(), b.cuda()
    code = ln_code(cols, vec)
    what = f"LN{tag} rows={rows} cols={cols} ld={ld}{' in place' if inplace else ''}"
    xin = Guarded(rows, cols, ld, off=off, fill=x.cuda())
    out = xin if inplace else Guarded(rows, cols, ld)
    ops.layernorm(xin.win, wd, bd, 1e-6, out=out.win)
    _confirm(ops, "ln", code, what)
    out.untouched(what); xin.untouched(what + " (input buffer)")
    _err(out.win, F.layer_norm(x.double(), (cols,), w.double(), b.double(), 1e-6), 2e-5, "layernorm", what)
    xin = Guarded(rows, cols, ld, off=off, fill=x.cuda())
    out = xin if inplace else Guarded(rows, cols, ld)
    res, rs = Guarded(rows, cols, ldr, fill=r.cuda()), Guarded(rows, 1)
    ops.layernorm(xin.win, wd, bd, 1e-5, act=ops.ACT_GELU, residual=res.win, out=out.win, scale_out=rs.win)
    _confirm(ops, "ln", code, what + " +res+gelu")
    out.untouched(what + " +res+gelu"); rs.untouched(what + " scales"); res.untouched(what + " (residual buffer)")
    assert torch.equal(res.win.cpu(), r)
    _err(out.win, F.gelu(F.layer_norm((x + r).double(), (cols,), w.double(), b.double(), 1e-5)), 2e-5, "layernorm", what + " +res+gelu")
    assert torch.equal(rs.win[:, 0].contiguous(), ops.row_scale_f16(out.win)), what + ": scale_out != row_scale_f16(output)"


@gpu
@pytest.mark.parametrize("cols,how", LN_SCALAR_CASES, ids=lambda v: str(v))
def test_layernorm_scalar_instances(ops, cols, how):
    """layernorm_kernel<2 / 4 / 8 / 16 / 44 / 0>: what rows that are not 16-byte aligned (odd stride, or a base pointer one float off) and rows narrower than
    256 or wider than 4096 columns get, at both sides of every threshold, one row and 37 rows (a last block of one wave)."""
    for rows in LN_ROWS:
        if how == "strided":
            _ln_both_forms(ops, rows, cols, cols + 1, cols + 3, vec=False, tag=" scalar")
        elif how == "contiguous":
            _ln_both_forms(ops, rows, cols, cols, cols + 8, vec=False, tag=" scalar")
        else:
            _ln_both_forms(ops, rows, cols, cols, cols + 4, vec=False, off=1, tag=" scalar (x one float off)")


@gpu
@pytest.mark.parametrize("cols,ld", LN_V4_CASES, ids=lambda v: str(v))
def test_layernorm_float4_instances(ops, cols, ld):
    """layernorm_v4_kernel<1 / 2 / 4 / 8 / 16> on aligned rows, at both sides of every threshold and with a ragged last float4 (read whole, written element by
    element: the padding columns keep their sentinel), out of place and in place."""
    for rows in LN_ROWS:
        for inplace in (False, True):
            _ln_both_forms(ops, rows, cols, ld, ld + 4, vec=True, inplace=inplace, tag=" float4")


def _ln_packed_runs(ops, cols, ld, rows, act, bound=None):
    """(y: the unpacked output, words [rows, Kp], scales [rows], bound values or None) of one float4 LayerNorm case; the packed run is in place on a padded
    buffer whose padding holds 7.0 (the kernel must overwrite it with zeros)."""
    x, _, w, b = _ln_inputs(rows, cols, seed=cols + 7)
    x = x * torch.exp(torch.randn(rows, 1, generator=torch.Generator().manual_seed(cols)))
    wd, bd = w.cuda(), b.cuda()
    Kp = _kpad(cols)
    y = Guarded(rows, cols, ld)
    xin = Guarded(rows, Kp, ld)
    xin.win.fill_(7.0); xin.win[:, :cols] = x.cuda()
    ops.layernorm(xin.win[:, :cols], wd, bd, 1e-6, act=act, out=y.win)
    _confirm(ops, "ln", ln_code(cols, True), f"LN cols={cols} unpacked")
    y.untouched()
    rs, bb = Guarded(rows, 1), Guarded(rows, 1)
    ops.layernorm(xin.win[:, :cols], wd, bd, 1e-6, act=act, out=xin.win[:, :cols], scale_out=rs.win, pack=True,
                  bound_out=None if bound is None else (bb.win, *bound))
    _confirm(ops, "ln", ln_code(cols, True, True), f"LN cols={cols} packed")
    xin.untouched(f"LN cols={cols} packed"); rs.untouched(); bb.untouched()
    ref = F.layer_norm(x.double(), (cols,), w.double(), b.double(), 1e-6)
    return y.win, xin.win, rs.win[:, 0].contiguous(), None if bound is None else bb.win[:, 0].cpu().double(), F.gelu(ref) if act else ref


@gpu
@pytest.mark.parametrize("cols,ld", LN_PACKED_CASES, ids=lambda v: str(v))
def test_layernorm_packed_instances(ops, cols, ld):
    """The identity test_layernorm_packed_output states, for every packed instance it leaves out (<1>, <8>; <2>, <4> again with the instance confirmed):
    LayerNorm with pack=True == LayerNorm, then row_scale_f16 + pack_rows_g8, bit for bit; and the decoded rows are within 2e-5 + 2^-21 rowmax of fp64."""
    for rows in LN_ROWS:
        for act in (ops.ACT_NONE, ops.ACT_GELU):
            y, words, scales, _, ref = _ln_packed_runs(ops, cols, ld, rows, act)
            what = f"LN packed rows={rows} cols={cols} act={act}"
            _packed_is_the_packing_of(ops, words, scales, y, what)
            _err(unpack_g8(words, scales, cols), ref, 2e-5, "layernorm packed", what + ", decoded", rowmax_term=2.0 ** -21)


@gpu
def test_layernorm_packed_last_lane_pairs_with_a_zero_lane(ops):
    """cols = 260 = 4 (mod 8) on a row stride of packed_cols(260) = 288: the last float4 of the row shares its group with a lane that holds zeros, and the 28
    padding columns are written as zeros over the 7.0 they held.  Five rows: a workgroup of four waves, then a ragged one."""
    cols, ld, rows = 260, ops.packed_cols(260), 5
    assert ld == 288
    for act in (ops.ACT_NONE, ops.ACT_GELU):
        y, words, scales, _, ref = _ln_packed_runs(ops, cols, ld, rows, act)
        what = f"LN packed rows={rows} cols={cols} ld={ld} act={act}"
        assert words.shape == (rows, ld)
        _packed_is_the_packing_of(ops, words, scales, y, what)
        _err(unpack_g8(words, scales, cols), ref, 2e-5, "layernorm packed", what + ", decoded", rowmax_term=2.0 ** -21)


@gpu
@pytest.mark.parametrize("K", [36, 64])
def test_scale_pack_writers_at_the_pairing_edges(ops, K):
    """psam_scale_pack_rows_g8, _add and _add_dual on five rows (four waves, then a ragged workgroup).  K = 36 = 4 (mod 8): the last real lane's partner is a
    zero lane and columns 36 .. 63 are padding, written as zeros.  K = 64 with ld == K: the row is full, nothing is written past it (guard rows and the floats
    outside the windows keep their sentinel).  Words and scales equal, bit for bit, pack_rows_g8 of the fp32 rows and the host packer of g8_reference."""
    L, check = ops._lib.load(), ops._lib.check
    rows, Kp = 5, ops.packed_cols(K)
    g = torch.Generator().manual_seed(K)
    x = (torch.randn(rows, K, generator=g) * torch.exp(2 * torch.randn(rows, 1, generator=g))).cuda()
    pos = torch.randn(rows, K, generator=g).cuda()
    total = pos + x              # one fp32 addition per element, as the kernels form it
    stream = torch.cuda.current_stream().cuda_stream
    win = lambda: (Guarded(rows, Kp), Guarded(rows, 1))
    (p1, s1), (p2, s2), (p3, s3), (p4, s4) = win(), win(), win(), win()
    check(L.psam_scale_pack_rows_g8(x.data_ptr(), K, rows, K, p1.win.data_ptr(), Kp, s1.win.data_ptr(), stream), "scale_pack")
    check(L.psam_scale_pack_rows_g8_add(x.data_ptr(), K, pos.data_ptr(), K, rows, 1, rows, K, p2.win.data_ptr(), Kp, s2.win.data_ptr(), stream), "add")
    check(L.psam_scale_pack_rows_g8_add_dual(x.data_ptr(), K, pos.data_ptr(), K, rows, 1, rows, K, p3.win.data_ptr(), s3.win.data_ptr(), p4.win.data_ptr(),
                                             s4.win.data_ptr(), Kp, stream), "dual")
    torch.cuda.synchronize()
    for name, p, sc, y in (("scale_pack", p1, s1, x), ("add", p2, s2, total), ("dual, sum", p3, s3, total), ("dual, x", p4, s4, x)):
        what = f"{name} rows={rows} K={K}"
        p.untouched(what); sc.untouched(what + ": scales")
        _packed_is_the_packing_of(ops, p.win, sc.win[:, 0].contiguous(), y, what)


@gpu
@pytest.mark.parametrize("cols,ld", LN_BOUND_CASES, ids=lambda v: str(v))
def test_layernorm_row_bound(ops, cols, ld):
    """bound_out=(buf, c2, c1, c0): with t0 the fp64 L2 norm of the fp32 output row and P(t) = c2 t^2 + c1 t + c0, P(t0) <= buf[r] (the point of the feature: a
    bound) <= P(1.0001 t0) (1 + 1e-5) (the kernel's own safety factor plus fp32 rounding of a sum of <= 4096 squares); words and scales are the ones of the
    same call without the bound."""
    rows = 37
    for act in (ops.ACT_NONE, ops.ACT_GELU):
        y, words0, scales0, _, ref = _ln_packed_runs(ops, cols, ld, rows, act)
        _err(unpack_g8(words0, scales0, cols), ref, 2e-5, "layernorm packed", f"LN packed cols={cols} ld={ld} act={act}, decoded", rowmax_term=2.0 ** -21)
        assert (unpack_g8(words0, scales0, _kpad(cols))[:, cols:] == 0).all(), "K padding not zero"
        t0 = y.cpu().double().norm(dim=1)
        for c2, c1, c0 in LN_BOUND_COEFFS:
            _, words, scales, got, _ = _ln_packed_runs(ops, cols, ld, rows, act, bound=(c2, c1, c0))
            assert _same_words(words, words0) and torch.equal(scales, scales0), "asking for the bound changed the packed rows"
            P = lambda t: (c2 * t + c1) * t + c0
            lo, hi = P(t0), P(t0 * 1.0001) * (1 + 1e-5)
            print(f"| LN bound cols={cols} act={act} c=({c2}, {c1}, {c0}) | buf / P(t0) - 1 in [{(got / lo - 1).min().item():.3e}, {(got / lo - 1).max().item():.3e}] |")
            assert (got >= lo).all(), f"row bound below P(||y||): min buf / P(t0) - 1 = {(got / lo - 1).min().item():.3e}"
            assert (got <= hi).all(), f"row bound above P(1.0001 ||y||) (1 + 1e-5): max buf / hi - 1 = {(got / hi - 1).max().item():.3e}"


# ------------------------------------------------------------------------------------------------ 3. swiglu_ln
@gpu
@pytest.mark.parametrize("H", SWIGLU_H)
def test_swiglu_ln_instances(ops, H):
    """swiglu_ln_kernel<8 / 32 / 44 / 0> at both sides of every threshold, one row and nine, xoff = Hp = H rounded up to 32, out with row stride H, Hp and Hp + 64:
    columns [0, H) within 2e-5 of LayerNorm(SiLU(g) x) in fp64, columns [H, ldo) zero, the guard rows untouched.  The columns of gx between H and Hp hold 1e6
    (never read into the statistics)."""
    Hp = (H + 31) // 32 * 32
    w, b = None, None
    for rows in SWIGLU_ROWS:
        g = torch.Generator().manual_seed(H + rows)
        gx = torch.randn(rows, 2 * Hp, generator=g)
        gx[:, H:Hp] = 1e6; gx[:, Hp + H:] = 1e6
        w, b = 1 + 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
        want = F.layer_norm((F.silu(gx[:, :H].double()) * gx[:, Hp:Hp + H].double()), (H,), w.double(), b.double(), 1e-6)
        gxd, wd, bd = gx.cuda(), w.cuda(), b.cuda()
        for ldo in sorted({H, Hp, Hp + 64}):
            what = f"swiglu_ln H={H} rows={rows} ldo={ldo}"
            out = Guarded(rows, ldo)
            ops.swiglu_ln(gxd, Hp, H, wd, bd, 1e-6, out.win)
            _confirm(ops, "swiglu", swiglu_code(H), what)
            out.untouched(what)
            _err(out.win[:, :H], want, 2e-5, "swiglu_ln", what)
            assert (out.win[:, H:] == 0).all(), what + ": columns [H, ldo) must read 0"


# ------------------------------------------------------------------------------------------------ 3. interp3
def _interp_inputs(Z, N, rep, C, seed):
    g = torch.Generator().manual_seed(seed)
    B = Z // rep
    src = torch.randn(Z, INTERP_G, C, generator=g)
    idx = torch.randint(0, INTERP_G, (B, N, 3), generator=g)
    idx[0, 0] = 5                                      # equal triples: all three the same row ...
    idx[B - 1, N - 1, 1] = idx[B - 1, N - 1, 0]        # ... and two of three (the same point when B N == 1)
    w3 = torch.rand(B, N, 3, generator=g)              # not normalised
    want = O.interpolate(src.double(), _rep(idx, rep), _rep(w3, rep).double())
    return g, src, idx, w3, want


@gpu
@pytest.mark.parametrize("C", INTERP_GENERIC_C)
def test_interp3_generic_kernel(ops, C):
    """interp3_kernel (every C but 256): fp64 reference at 1e-5 (the project's bound), guard rows untouched; LayerNorm / packed output are refused on the host
    for these widths (non-zero status, last_instance -1, nothing written)."""
    lib = ops._lib.load()
    for Z, N, rep in INTERP_SHAPES[:3]:
        _, src, idx, w3, want = _interp_inputs(Z, N, rep, C, seed=C + N)
        what = f"interp3 C={C} Z={Z} N={N} rep={rep}"
        out = Guarded(Z * N, C)
        d = [t.cuda() for t in (src, idx, w3)]
        ops.interp3(*d, out.win, rep)
        _confirm(ops, "interp3", 0, what)
        out.untouched(what)
        _err(out.win, want.view(-1, C), 1e-5, "interp3", what)
        gam, sc = torch.ones(C, device="cuda"), Guarded(Z * N, 1)
        out = Guarded(Z * N, C)
        stream = torch.cuda.current_stream().cuda_stream
        rc = lib.psam_interp3_ex(*(t.data_ptr() for t in d), out.win.data_ptr(), rep, Z, N, INTERP_G, C, None, gam.data_ptr(), gam.data_ptr(), 1e-5, 1, stream)
        assert rc != 0 and lib.psam_interp3_last_instance() == -1, (what, "ln= with C != 256", rc)
        torch.cuda.synchronize()
        assert (out.flat == SENTINEL).all(), what + ": a refused call wrote"
        ops.interp3(*d, out.win, rep)
        assert lib.psam_interp3_last_instance() == 0
        out.win.fill_(SENTINEL)
        rc = lib.psam_interp3_ex(*(t.data_ptr() for t in d), out.win.data_ptr(), rep, Z, N, INTERP_G, C, sc.win.data_ptr(), None, None, 0.0, 0, stream)
        assert rc != 0 and lib.psam_interp3_last_instance() == -1, (what, "scale_out= with C != 256", rc)
        torch.cuda.synchronize()
        assert (out.flat == SENTINEL).all() and (sc.flat == SENTINEL).all(), what + ": a refused call wrote"


@gpu
@pytest.mark.parametrize("Z,N,rep", INTERP_SHAPES + [INTERP_FIVE_ROWS])
def test_interp3_c256_kernel(ops, Z, N, rep):
    """interp3_c256_kernel<4>, four rows per wave, at row counts with a tail of 1, 3 and 0 rows: plain; LayerNorm + GELU; LayerNorm + ReLU; LayerNorm + GELU
    packed -- each within 1e-5 of fp64 (packed: decoded, + 2^-21 rowmax), guard rows and scale_out beyond Z N untouched, and the packed rows bit for bit the
    packing of the unpacked LayerNorm + GELU output of the same inputs."""
    C = 256
    g, src, idx, w3, want = _interp_inputs(Z, N, rep, C, seed=Z * 1000 + N)
    gam, bet = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    ln = F.layer_norm(want, (C,), gam.double(), bet.double(), 1e-5)
    d = [t.cuda() for t in (src, idx, w3)]
    lnp = (gam.cuda(), bet.cuda(), 1e-5)
    y = None
    for name, kw, ref in (("plain", {}, want), ("LN+GELU", dict(ln=lnp, act=ops.ACT_GELU), F.gelu(ln)), ("LN+ReLU", dict(ln=lnp, act=ops.ACT_RELU), F.relu(ln))):
        what = f"interp3 C=256 Z={Z} N={N} rep={rep} {name}"
        out = Guarded(Z * N, C)
        ops.interp3(*d, out.win, rep, **kw)
        _confirm(ops, "interp3", 256, what)
        out.untouched(what)
        _err(out.win, ref.view(-1, C), 1e-5, "interp3", what)
        if name == "LN+GELU":
            y = out.win
    what = f"interp3 C=256 Z={Z} N={N} rep={rep} LN+GELU packed"
    out, sc = Guarded(Z * N, C), Guarded(Z * N, 1)
    ops.interp3(*d, out.win, rep, scale_out=sc.win, ln=lnp, act=ops.ACT_GELU)
    _confirm(ops, "interp3", 256, what)
    out.untouched(what); sc.untouched(what + ": scale_out beyond Z N")
    scales = sc.win[:, 0].contiguous()
    _err(unpack_g8(out.win, scales, C), F.gelu(ln).view(-1, C), 1e-5, "interp3 packed", what + ", decoded", rowmax_term=2.0 ** -21)
    _packed_is_the_packing_of(ops, out.win, scales, y, what)


# ------------------------------------------------------------------------------------------------ 3. the small ones
@gpu
@pytest.mark.parametrize("C", [256, 36])
def test_add_bcast_broadcasts_rows_into_a_token_buffer(ops, C):
    """add_bcast with b=None, sa=0, so=T C: the form that writes the output tokens in front of every prompt's token rows; the other rows keep their sentinel."""
    Z, R, T = 6, 5, 8
    a = torch.randn(R, C, generator=torch.Generator().manual_seed(C))
    tokens = torch.full((Z + 1, T, C), SENTINEL, device="cuda")
    ops.add_bcast(a.cuda(), Z, None, tokens, Z, R, C, sa=0, so=T * C)
    assert torch.equal(tokens[:Z, :R].cpu(), a.expand(Z, R, C))
    assert (tokens[:Z, R:] == SENTINEL).all() and (tokens[Z] == SENTINEL).all()


@gpu
@pytest.mark.parametrize("K", [1, 16, 33])
def test_group_max_into_a_strided_view(ops, K):
    groups, C = 37, 97
    x = torch.randn(groups * K, C, generator=torch.Generator().manual_seed(K))
    out = Guarded(groups, C, C + 24, off=8)
    ops.group_max(x.cuda(), K, out=out.win)
    out.untouched(f"group_max K={K}")
    assert torch.equal(out.win.cpu(), x.view(groups, K, C).max(1).values)


@gpu
def test_every_registry_instance_was_confirmed(ops):
    """Runs last: the GPU tests above confirmed, by `last_instance`, every code of every registry entry at least once."""
    want = {(i.family, c) for i in INSTANCES.values() for c in i.codes}
    print("\nconfirmed instances:", ", ".join(f"{f}:{c}" for f, c in sorted(SEEN)))
    print("largest |kernel - fp64| per family:", ", ".join(f"{k} {v:.2e}" for k, v in sorted(WORST.items())))
    assert SEEN == want, f"never confirmed: {sorted(want - SEEN)}; not in the registry: {sorted(SEEN - want)}"
