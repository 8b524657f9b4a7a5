"""Every launchable attention kernel instance, checked on its own.

csrc/attention.hip ships three families -- fp32 MFMA (`flash_attn_f32_kernel`, one instance per head dim), fp32-input f16x3 (`flash_attn_f16x3_kernel<64>`,
`<128, 96>`, `<128>`, with an optional key split) and packed-operand f16x3 (`flash_attn_packed_kernel<8>`, `<4>`, `<4, 2>`; `<4, 3, 2>` in experiments
builds) -- and csrc/rowops.hip the small-sequence kernels behind psam_attention_small.  INSTANCES lists them all with how each is reached; a CPU test keeps it
equal to the launch sites of the sources, so an instance added or changed later without coverage here fails without a GPU.  On the GPU every entry is forced,
run, and confirmed by the library's `*_last_instance` / `_last_keysplit` queries to have run as itself:
  * against an fp64 SDPA of the values the kernel receives, in a per-(cloud, head) measure, bounded by the error of a plain fp32 evaluation of the same inputs;
  * bit for bit against its sibling instances where the design promises the same arithmetic, and repeatably;
  * on one-hot selection inputs, where the output must be one V row of the right key, head and cloud to 2^-20 relative;
  * through the environment switches in fresh child processes."""
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
NCU = 256         # MI355X: the shape conditions below are stated for it; the `last_*` assertions fail loudly on anything else
gpu = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------ 1. the registry
# family: f32 | f16x3 | packed | small.  code: what the family's `last_instance` query reports after this instance ran.  hds: head dims served.
# reach: how a test gets it (hook or environment value + shape condition).  experiments: compiled only with PSAM_BUILD_EXPERIMENTS.
Inst = namedtuple("Inst", "family file code hds reach experiments")
INSTANCES = {
    "flash_attn_f32_kernel<2,1>": Inst("f32", "attention.hip", 16, (16,), "psam_attention_f32, hd == 16", False),
    "flash_attn_f32_kernel<3,1>": Inst("f32", "attention.hip", 24, (24,), "psam_attention_f32, hd == 24", False),
    "flash_attn_f32_kernel<4,1>": Inst("f32", "attention.hip", 32, (32,), "psam_attention_f32, hd == 32", False),
    "flash_attn_f32_kernel<6,2>": Inst("f32", "attention.hip", 48, (48,), "psam_attention_f32, hd == 48", False),
    "flash_attn_f32_kernel<8,2>": Inst("f32", "attention.hip", 64, (64,), "psam_attention_f32, hd == 64", False),
    "flash_attn_f32_kernel<11,3>": Inst("f32", "attention.hip", 88, (88,), "psam_attention_f32, hd == 88", False),
    "flash_attn_f32_kernel<12,3>": Inst("f32", "attention.hip", 96, (96,), "psam_attention_f32, hd == 96", False),
    "flash_attn_f32_kernel<16,4>": Inst("f32", "attention.hip", 128, (128,), "psam_attention_f32, hd == 128", False),
    "flash_attn_f16x3_kernel<64>": Inst("f16x3", "attention.hip", 64, (64,), "psam_attention_f16x3_ex2, hd == 64 (never key-split)", False),
    "flash_attn_f16x3_kernel<128,96>": Inst("f16x3", "attention.hip", 96, (72, 80, 88, 96),
                                            "psam_attention_f16x3_ex2, 64 < hd <= 96, PSAM_ATTN_FULL_WIDTH unset; key split by max_keysplit", False),
    "flash_attn_f16x3_kernel<128>": Inst("f16x3", "attention.hip", 128, (104, 112, 120, 128),
                                         "psam_attention_f16x3_ex2, 96 < hd <= 128 (or 64 < hd <= 96 with PSAM_ATTN_FULL_WIDTH=1); key split by max_keysplit", False),
    "flash_attn_packed_kernel<8>": Inst("packed", "attention.hip", 831, (64,),
                                        "psam_attention_packed_force_nw(8) / PSAM_ATTN_PACKED_NW=8; or variant 0 with ceil(L/256) H B >= CUs; or L <= 128", False),
    "flash_attn_packed_kernel<4>": Inst("packed", "attention.hip", 431, (64,),
                                        "psam_attention_packed_force_nw(4) / PSAM_ATTN_PACKED_NW=4; or variant 0 with ceil(L/256) H B < CUs and L > 128", False),
    "flash_attn_packed_kernel<4,2>": Inst("packed", "attention.hip", 421, (64,),
                                          "psam_attention_packed_force_variant(1) / PSAM_ATTN_VARIANT=1, no forced shape, L > 128, ceil(L/128) H B <= 4 CUs", False),
    "flash_attn_packed_kernel<4,3,2>": Inst("packed", "attention.hip", 432, (64,), "psam_attention_packed_force_variant(2), no forced shape, L > 128", True),
    "attention_small_kernel": Inst("small", "rowops.hip", 0, (16, 24, 32, 64), "psam_attention_small otherwise (psam_attention_small_force_split(0) for many keys)", False),
    "attention_small_split_kernel": Inst("small", "rowops.hip", 1, (16, 32, 64), "psam_attention_small, Lk >= 128, Z H Lq <= 2048, hd in 4 8 16 32 64", False),
    "attention_fewkeys_kernel<4>": Inst("small", "rowops.hip", 4, (16,), "psam_attention_small, Lk <= 16, Lq >= 64, hd == 16", False),
    "attention_fewkeys_kernel<8>": Inst("small", "rowops.hip", 8, (32,), "psam_attention_small, Lk <= 16, Lq >= 64, hd == 32", False),
}
PACKED = [(k, i.code) for k, i in INSTANCES.items() if i.family == "packed" and not i.experiments]
F16X3_OF_HD = {hd: i.code for i in INSTANCES.values() if i.family == "f16x3" for hd in i.hds}
F16X3_HDS = sorted(F16X3_OF_HD)
F32_HDS = sorted(hd for i in INSTANCES.values() if i.family == "f32" for hd in i.hds)


# ------------------------------------------------------------------------------------------------ source parsing (CPU)
def _split_build(src, names=("PSAM_BUILD_EXPERIMENTS",)):
    """(default, guarded): the lines a default build compiles and the lines inside `#ifdef <names>` blocks (their #else parts count as default);
    PSAM_ATTN_ABLATE blocks (a separate measuring build) are dropped from both."""
    default, guarded, stack = [], [], []      # stack entries: None (neutral) or [state now, state after #else]; states: "on" | "exp" | "off"
    for line in src.splitlines():
        t = line.strip()
        m = re.match(r"#\s*(ifdef|ifndef)\s+(\w+)", t)
        if m and (m.group(2) in names or m.group(2) == "PSAM_ATTN_ABLATE"):
            inside = "off" if m.group(2) == "PSAM_ATTN_ABLATE" else "exp"
            stack.append([inside, "on"] if m.group(1) == "ifdef" else ["on", inside])
            continue
        if re.match(r"#\s*if", t):
            stack.append(None)
        elif re.match(r"#\s*else", t) and stack and stack[-1] is not None:
            stack[-1][0] = stack[-1][1]
            continue
        elif re.match(r"#\s*endif", t):
            if stack.pop() is not None:
                continue
        states = [s[0] for s in stack if s is not None]
        if "off" in states:
            continue
        (guarded if "exp" in states else default).append(line)
    return "\n".join(default), "\n".join(guarded)


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


_KERNEL = r"([A-Za-z_]\w*_kernel)\s*(<[^<>()]*>)?"


def launched_instances(text):
    """Kernel instantiations named at launch sites (hipLaunchKernelGGL, and the FA_LAUNCH(HD8, DT) macro of the f32 family) and in the LDS opt-in (psam_reserve_lds),
    spelled without blanks: {"flash_attn_packed_kernel<4,2>", ...}.  The macro's own definition (template arguments that are names) is not an instance."""
    text = re.sub(r"//[^\n]*", "", text)
    found = set()
    for m in re.finditer(r"hipLaunchKernelGGL\(\s*\(?\s*" + _KERNEL, text):
        found.add(m.group(1) + (m.group(2) or "").replace(" ", ""))
    for m in re.finditer(r"psam_reserve_lds\(\s*&\s*" + _KERNEL, text):
        found.add(m.group(1) + (m.group(2) or "").replace(" ", ""))
    macro = re.search(r"#define\s+FA_LAUNCH\(HD8, DT\)\s+hipLaunchKernelGGL\(\(" + _KERNEL, text)
    for m in re.finditer(r"\bFA_LAUNCH\(\s*(\d+)\s*,\s*(\d+)\s*\)", text):
        assert macro, "FA_LAUNCH used but not defined as a launch"
        found.add(f"{macro.group(1)}<{m.group(1)},{m.group(2)}>")
    return {f for f in found if not re.search(r"<.*[A-Za-z_]", f)}


def source_instances(attention_src, rowops_src):
    """({instance: file} of a default build, {instance: file} that only an experiments build adds)."""
    d_att, g_att = _split_build(attention_src)
    small = _body(rowops_src, "PSAM_API int32_t psam_attention_small(")
    d_row, g_row = _split_build(small)
    default = {**{k: "attention.hip" for k in launched_instances(d_att)}, **{k: "rowops.hip" for k in launched_instances(d_row)}}
    extra = {**{k: "attention.hip" for k in launched_instances(g_att)}, **{k: "rowops.hip" for k in launched_instances(g_row)}}
    return default, {k: f for k, f in extra.items() if k not in default}


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def test_registry_matches_the_launch_sites():
    """INSTANCES == the kernel instantiations csrc/attention.hip and psam_attention_small (csrc/rowops.hip) launch or opt into LDS for, default build and
    experiments-only; every packed instance is both launched and given its LDS attribute; the codes the sources report match the table."""
    att, row = _read("attention.hip"), _read("rowops.hip")
    default, extra = source_instances(att, row)
    want_default = {k: i.file for k, i in INSTANCES.items() if not i.experiments}
    want_extra = {k: i.file for k, i in INSTANCES.items() if i.experiments}
    assert default == want_default, (sorted(set(default) ^ set(want_default)), "launched by the sources vs listed in INSTANCES")
    assert extra == want_extra, (sorted(set(extra) ^ set(want_extra)), "experiments-only")
    body = re.sub(r"//[^\n]*", "", _body(att, "PSAM_API int32_t psam_attention_packed("))
    for k, i in INSTANCES.items():
        if i.family == "packed":
            spaced = re.escape(k).replace(",", r",\s*")
            assert re.search(r"psam_reserve_lds\(&" + spaced + r",", body), k
            assert re.search(r"hipLaunchKernelGGL\(\(?" + spaced + r"\)?,", body), k
            assert re.search(r"pa_launched\([^)]*\b%d\b" % i.code, body), (k, i.code)
            args = [int(a) for a in k[k.index("<") + 1:-1].split(",")]
            nw, ring, qb = args + [3, 1][len(args) - 1:]      # template <int NW, int RING = 3, int QB = 1>
            assert i.code == nw * 100 + ring * 10 + qb, (k, i.code)
    # the f32 family: one instance per admitted head dim, HD8 = hd / 8
    for k, i in INSTANCES.items():
        if i.family == "f32":
            assert int(k[k.index("<") + 1:k.index(",")]) * 8 == i.code == i.hds[0], k
            assert re.search(r"case %d: FA_LAUNCH\(%s\)" % (i.code, k[k.index("<") + 1:-1].replace(",", r",\s*")), att), k
    assert set(F16X3_HDS) == {64, 72, 80, 88, 96, 104, 112, 120, 128} and F32_HDS == [16, 24, 32, 48, 64, 88, 96, 128]


def test_the_parser_sees_an_edited_launch_site():
    """The registry test must fail when one launch site is edited to a new instance: the parser reports the new instance and misses the old one."""
    att, row = _read("attention.hip"), _read("rowops.hip")
    site = "hipLaunchKernelGGL(flash_attn_packed_kernel<4>, dim3("
    assert att.count(site) == 1
    default, _ = source_instances(att.replace(site, "hipLaunchKernelGGL((flash_attn_packed_kernel<2, 3>), dim3("), row)
    assert "flash_attn_packed_kernel<2,3>" in default and set(default) - set(INSTANCES) == {"flash_attn_packed_kernel<2,3>"}
    default, _ = source_instances(att.replace("case 88: FA_LAUNCH(11, 3)", "case 88: FA_LAUNCH(11, 2)"), row)
    assert set(default) ^ {k for k, i in INSTANCES.items() if not i.experiments} == {"flash_attn_f32_kernel<11,3>", "flash_attn_f32_kernel<11,2>"}
    default, extra = source_instances(att.replace("#ifdef PSAM_BUILD_EXPERIMENTS", "#ifdef PSAM_SOMETHING_ELSE"), row)
    assert "flash_attn_packed_kernel<4,3,2>" in default and not extra


def test_exports_are_declared_and_bound():
    from point_sam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pointsam_hip.h")).read()
    for name in ("psam_attention_packed_last_instance", "psam_attention_packed_force_nw", "psam_attention_f16x3_last_instance",
                 "psam_attention_f16x3_last_keysplit", "psam_attention_f32_last_instance", "psam_attention_small_last_instance"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.SIGNATURES, name
    lib = _lib.load()
    # nothing has launched on this thread: refused / never-run values
    import threading
    seen = []
    t = threading.Thread(target=lambda: seen.extend([lib.psam_attention_packed_last_instance(), lib.psam_attention_f16x3_last_instance(),
                                                     lib.psam_attention_f16x3_last_keysplit(), lib.psam_attention_f32_last_instance(),
                                                     lib.psam_attention_small_last_instance()]))
    t.start(); t.join()
    assert seen == [-1, -1, 0, -1, -1]
    # a refused call (null pointers: rejected on the host before any device call) reports -1 / 0
    assert lib.psam_attention_f16x3_ex2(None, 0, 0, None, 0, 0, None, 0, 0, None, 0, 0, 1, 1, 1, 1, 64, 1.0, None, 0.0, 0.0, None, 1, None, 0, None, None) != 0
    assert (lib.psam_attention_f16x3_last_instance(), lib.psam_attention_f16x3_last_keysplit()) == (-1, 0)
    assert lib.psam_attention_packed(None, 0, None, None, 0, None, 1, 1, 1, 64, 1.0, 1.0, None) != 0 and lib.psam_attention_packed_last_instance() == -1
    assert lib.psam_attention_f32(None, 0, 0, None, 0, 0, None, 0, 0, None, 0, 0, 1, 1, 1, 1, 64, 1.0, None) != 0 and lib.psam_attention_f32_last_instance() == -1
    assert lib.psam_attention_small(None, 0, 0, None, 0, 0, None, 0, 0, None, 0, 0, 1, 1, 1, 1, 16, 1.0, None) != 0 and lib.psam_attention_small_last_instance() == -1


# ------------------------------------------------------------------------------------------------ the cases
# Packed family: (H, B, L, slack, pad).  slack: the common power-of-two scale comes from a bound `slack` times the largest value (a different scale per
# call: 8, 64, 1000); pad: the packed input is a column window of a wider buffer (ld = 3 D + 40, 8 containers in) and so is the output (ldo = D + 24).
# L: ragged last tile with the second 32-key sub-tile partly (129, 130, 257) and wholly (191 has it, 129 / 130 / 257 do not) past the end; 1, 2, 3, 4, 5, 16
# and 32 tiles (more than ring slots); H B = 6 (not a multiple of 8: plain block mapping) and 8, 32, 128 (XCD-aware mapping), each with several query blocks.
PackedCase = namedtuple("PackedCase", "H B L slack pad")
PACKED_CASES = [PackedCase(3, 2, 129, 8.0, False), PackedCase(3, 2, 130, 1000.0, True), PackedCase(3, 2, 191, 8.0, True), PackedCase(3, 2, 192, 64.0, False),
                PackedCase(3, 2, 193, 8.0, True), PackedCase(4, 2, 256, 8.0, False), PackedCase(3, 2, 257, 64.0, True), PackedCase(3, 2, 300, 8.0, True),
                PackedCase(3, 2, 300, 1000.0, True), PackedCase(4, 2, 300, 8.0, False), PackedCase(3, 2, 1000, 8.0, True), PackedCase(4, 2, 1000, 64.0, False),
                PackedCase(3, 2, 2048, 8.0, False), PackedCase(16, 8, 300, 8.0, True), PackedCase(16, 2, 2048, 8.0, True)]
PACKED_ONE_BLOCK = [PackedCase(3, 2, 64, 8.0, True), PackedCase(4, 2, 100, 64.0, False), PackedCase(3, 2, 128, 8.0, True)]      # L <= 128: <8> only
ONEHOT_PACKED_L = (64, 100, 128, 129, 130, 191, 192, 193, 256, 257, 300, 1000, 2048)

# F16x3 family, unsplit: every head dim at ragged Lq != Lk.  Key split (head dims above 64): (ks, Lq, Lk) with ks = min(max_keysplit, 4, CUs / units,
# ntiles / 2), units = ceil(Lq / 128) H B = 12 (H 3, B 2), ntiles = ceil(Lk / 64): the smallest admitted tile count 2 ks (4, 6, 8), tile counts that divide by
# the factor (8 / 2, 9 / 3, 16 / 4) and that do not (5 / 2, 8 / 3, 10 / 4), Lq != Lk throughout (plain output admits it).
F16X3_PLAIN = (130, 257)
SplitCase = namedtuple("SplitCase", "ks Lq Lk")
F16X3_SPLIT = [SplitCase(2, 130, 200), SplitCase(2, 130, 300), SplitCase(2, 200, 512), SplitCase(3, 130, 330), SplitCase(3, 200, 500), SplitCase(3, 130, 570),
               SplitCase(4, 130, 500), SplitCase(4, 200, 630), SplitCase(4, 130, 1000)]
F16X3_SPLIT_HDS = (72, 88, 104, 128)
SPLIT_H, SPLIT_B = 3, 2

# Small family: (kernel code, hd, H, Z, Lq, Lk)
SMALL_CASES = [(0, 32, 4, 2, 7, 7), (0, 24, 3, 2, 3, 70), (0, 16, 8, 2, 6, 1000), (1, 16, 8, 2, 7, 512), (1, 64, 3, 2, 5, 515), (1, 32, 3, 2, 10, 130),
               (4, 16, 3, 2, 300, 12), (8, 32, 4, 2, 300, 16)]


def expected_keysplit(B, H, Lq, Lk, hd, max_keysplit, ncu=NCU):
    """fa_keysplit_factor of csrc/attention.hip."""
    if hd <= 64:
        return 1
    units, ntiles = -(-Lq // 128) * H * B, -(-Lk // 64)
    ks = min(ncu // units, 4, max_keysplit, ntiles // 2)
    return ks if ks > 1 and units <= 4096 else 1


def test_split_cases_are_what_they_claim():
    for c in F16X3_SPLIT:
        nt = -(-c.Lk // 64)
        assert c.Lq != c.Lk and nt >= 2 * c.ks
        for hd in F16X3_SPLIT_HDS:
            assert expected_keysplit(SPLIT_B, SPLIT_H, c.Lq, c.Lk, hd, c.ks) == c.ks
            assert expected_keysplit(SPLIT_B, SPLIT_H, c.Lq, c.Lk, hd, 4) >= c.ks
    for ks in (2, 3, 4):
        nts = {-(-c.Lk // 64) for c in F16X3_SPLIT if c.ks == ks}
        assert 2 * ks in nts and any(n % ks == 0 and n > 2 * ks for n in nts) and any(n % ks for n in nts), (ks, nts)
    assert "constexpr int64_t FA_SK_MAX_UNITS = PSAM_CNT_ATTN_N;" in _read("attention.hip")      # expected_keysplit: `units <= 4096`
    assert int(re.search(r"PSAM_CNT_ATTN_N = (\d+)", _read("common.h")).group(1)) == 4096
    for c in PACKED_CASES:
        assert c.L > 128 and -(-c.L // 128) * c.H * c.B <= 4 * NCU      # <4, 2> admits it
    assert {c.L for c in PACKED_CASES} == {129, 130, 191, 192, 193, 256, 257, 300, 1000, 2048} and all(c.L <= 128 for c in PACKED_ONE_BLOCK)
    assert {(c.H * c.B) % 8 == 0 for c in PACKED_CASES if c.L > 256} == {True, False}
    # the two shapes production sends to <8> by itself on 256 CUs
    assert [c for c in PACKED_CASES if -(-c.L // 256) * c.H * c.B >= NCU] == [PackedCase(16, 8, 300, 8.0, True), PackedCase(16, 2, 2048, 8.0, True)]


# ------------------------------------------------------------------------------------------------ references and measures (torch, CPU)
def _sdpa_by_head(q, k, v, H, scale, dtype):
    """softmax(q k^T scale) v per (cloud, head), one head at a time (a 2048 x 2048 fp64 score matrix at a time): matmul, softmax, matmul in `dtype`."""
    B, Lq, D = q.shape
    hd = D // H
    out = torch.empty(B, Lq, D, dtype=dtype)
    for b in range(B):
        for h in range(H):
            c = slice(h * hd, (h + 1) * hd)
            s = (q[b, :, c].to(dtype) @ k[b, :, c].to(dtype).T) * scale
            out[b, :, c] = torch.softmax(s, -1) @ v[b, :, c].to(dtype)
    return out


def block_errors(got, want, H):
    """[B, H]: per (cloud, head) the largest |got - want| over that block divided by that block's largest |want|."""
    B, L, D = want.shape
    g, w = got.double().view(B, L, H, D // H), want.double().view(B, L, H, D // H)
    return (g - w).abs().amax(dim=(1, 3)) / w.abs().amax(dim=(1, 3))


def global_error(got, want):
    return ((got.double() - want.double()).abs().max() / want.double().abs().max()).item()


class Reference:
    """fp64 SDPA of the given values and the error of the plain fp32 evaluation of the same values, both in the per-block measure.
    bound = 4 x (fp32 evaluation's error) + 2e-7: the project's "same accuracy class as the f32 kernel" rule."""

    def __init__(self, q, k, v, H, scale):
        self.H = H
        self.want = _sdpa_by_head(q, k, v, H, scale, torch.float64)
        e32 = block_errors(_sdpa_by_head(q, k, v, H, scale, torch.float32), self.want, H)
        self.ref_err = e32.max().item()
        self.bound = 4 * self.ref_err + 2e-7

    def check(self, got, what):
        e = block_errors(got, self.want, self.H)
        err, (b, h) = e.max().item(), divmod(int(e.argmax()), self.H)
        print(f"| {what} | {err:.2e} | {self.ref_err:.2e} | {self.bound:.2e} | {global_error(got, self.want):.2e} | ({b}, {h}) |")
        assert math.isfinite(err) and err <= self.bound, f"{what}: per-(cloud, head) error {err:.3e} in block (cloud {b}, head {h}) > {self.bound:.3e} " \
                                                         f"(fp32 evaluation: {self.ref_err:.3e})"
        return err


def _header(title):
    print(f"\n{title}\n| case | kernel err | fp32 evaluation err | bound | kernel err / tensor max | worst (cloud, head) |\n|---|---|---|---|---|---|")


def onehot_inputs(B, H, Lq, Lk, hd, seed, gain=48.0):
    """One-hot selection inputs: (q, k, v [B, L, H hd] fp32, pi [B, H, Lq], scale).  Keys: unit-norm random rows times 8; q_i = k_pi(i) with pi drawn per (cloud,
    head) -- a permutation where Lq == Lk, else a random map; V: 11 significant bits, +-(1024 + randint(1024)) / 1024 * 2^randint(-3, 4), distinct per (cloud,
    head, key), so its hi / lo split is exact in every kernel.  Asserts the precondition in fp64: the selected logit exceeds every other one of its row by
    >= 64 in the log2 domain (the leakage of all other keys is below 2^-50 of the result)."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randn(B, Lk, H, hd, generator=g)
    k = k / k.norm(dim=-1, keepdim=True) * 8.0
    pi = torch.stack([torch.stack([torch.randperm(Lk, generator=g) if Lq == Lk else torch.randint(Lk, (Lq,), generator=g) for _ in range(H)]) for _ in range(B)])
    q = torch.gather(k, 1, pi.permute(0, 2, 1)[..., None].expand(B, Lq, H, hd))
    v = (1024 + torch.randint(1024, (B, Lk, H, hd), generator=g)).float() / 1024 * torch.exp2(torch.randint(-3, 4, (B, Lk, H, hd), generator=g).float())
    v = v * (1 - 2 * torch.randint(2, (B, Lk, H, hd), generator=g)).float()
    scale = gain / math.sqrt(hd)
    assert len({tuple(r) for r in v.reshape(B * Lk * H, hd)[:, :4].tolist()}) == B * Lk * H, "V rows not distinct"
    q, k, v = q.reshape(B, Lq, H * hd), k.reshape(B, Lk, H * hd), v.reshape(B, Lk, H * hd)
    onehot_precondition(q, k, pi, H, scale)
    return q, k, v, pi, scale


def onehot_precondition(q, k, pi, H, scale):
    """fp64, the reference alone: q_i is k_pi(i), and its logit exceeds every other logit of its row by >= 64 in the log2 domain."""
    B, Lq, D = q.shape
    hd = D // H
    for b in range(B):
        for h in range(H):
            qh, kh = q[b, :, h * hd:(h + 1) * hd].double(), k[b, :, h * hd:(h + 1) * hd].double()
            assert torch.equal(qh, kh[pi[b, h]])
            s = (qh @ kh.T) * (scale * 1.4426950408889634)
            sel = s.gather(1, pi[b, h][:, None])[:, 0]
            gap = (sel - s.scatter(1, pi[b, h][:, None], -1e300).max(1).values).min().item()
            assert gap >= 64.0, f"one-hot precondition: gap {gap:.1f} < 64 (cloud {b} head {h}: Lq {Lq} Lk {k.shape[1]} hd {hd})"


def onehot_check(got, v, pi, H, what):
    """every element: |out[i, d] - V[pi(i), d]| <= 2^-20 |V[pi(i), d]| -- P is split into 22 bits, hi v and lo v are exact and their sum rounds once, the
    normalisation by l is a division and two multiplications: about 2^-21 together; the bound is twice that.  No absolute term."""
    B, Lq, D = got.shape
    hd = D // H
    sel = torch.gather(v.view(B, -1, H, hd), 1, pi.permute(0, 2, 1)[..., None].expand(B, Lq, H, hd)).double()
    rel = ((got.double().view(B, Lq, H, hd) - sel).abs() / sel.abs())
    worst = rel.max().item()
    print(f"| {what} | {worst:.2e} | {2.0 ** -20:.2e} |")
    if not worst <= 2.0 ** -20:
        b, i, h, d = [int(x) for x in torch.unravel_index(torch.nan_to_num(rel, nan=1e30).argmax(), rel.shape)]
        # a mix-up selects a wrong but plausible row: say which, if it is one
        vv = v.view(B, -1, H, hd)
        hit = (vv == got.view(B, Lq, H, hd)[b, i, h].to(vv.dtype)).all(-1).nonzero()
        raise AssertionError(f"{what}: query {i} of (cloud {b}, head {h}) channel {d}: got {got.view(B, Lq, H, hd)[b, i, h, d].item()!r}, V[pi(i)] "
                             f"{sel[b, i, h, d].item()!r} (pi(i) = {int(pi[b, h, i])}; rel {worst:.3e} > 2^-20); row equals V[(cloud, key, head)] {hit.tolist()[:4]}")


def test_onehot_preconditions_hold_for_every_case():
    """The one-hot inputs of every GPU case meet the gap precondition (asserted inside onehot_inputs), on the CPU with the reference alone."""
    for hd in sorted(set(F32_HDS) | set(F16X3_HDS)):
        onehot_inputs(2, 3, *F16X3_PLAIN, hd, seed=hd)
    for c in F16X3_SPLIT[1::3]:
        onehot_inputs(SPLIT_B, SPLIT_H, c.Lq, c.Lk, 88, seed=c.Lk)
    for L in (130, 1000):
        onehot_inputs(2, 3, L, L, 64, seed=L)
    for code, hd, H, Z, Lq, Lk in SMALL_CASES:
        onehot_inputs(Z, H, Lq, Lk, hd, seed=Lk + hd)


# ------------------------------------------------------------------------------------------------ GPU plumbing
try:
    import torch
    from g8_reference import unpack_g8
except ImportError:      # pragma: no cover
    torch = None


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd import ops as _ops
    _ops._lib.load()
    return _ops


SENTINEL = -7.25      # what buffers hold where no kernel may write


class forced_packed:
    """Force (variant, nw) of psam_attention_packed for the enclosed launches; restored on exit (the hooks are process-global)."""

    def __init__(self, lib, variant, nw):
        self.lib, self.variant, self.nw = lib, variant, nw

    def __enter__(self):
        self.lib.psam_attention_packed_force_variant(self.variant)
        self.lib.psam_attention_packed_force_nw(self.nw)

    def __exit__(self, *exc):
        self.lib.psam_attention_packed_force_variant(-1)
        self.lib.psam_attention_packed_force_nw(-1)


# instance code -> (variant, nw) that forces it whatever the shape (421: where <4, 2> admits the shape)
PACKED_FORCE = {831: (0, 8), 431: (0, 4), 421: (1, 0), 432: (2, 0)}


class PackedProblem:
    """g8-packed q | k | v rows of one case on the device (optionally a window of a wider buffer whose other columns hold NaN), the values they decode to,
    and an output buffer (optionally a window as well) -- run(code) forces one instance, launches, confirms it ran and returns (out window, o_scale)."""

    def __init__(self, ops, H, B, L, slack, pad, q, k, v, scale):
        self.ops, self.lib, self.H, self.B, self.L, self.scale = ops, ops._lib.load(), H, B, L, scale
        D = self.D = H * 64
        x = torch.cat([q.reshape(B * L, D), k.reshape(B * L, D), v.reshape(B * L, D)], 1)
        e = math.floor(math.log2(float(x.abs().max()) * slack))
        self.sc = torch.full((B * L,), 2.0 ** (14 - e), device="cuda")
        assert float(x.abs().max()) * float(self.sc[0]) < 2.0 ** 15
        self.off, self.ld, self.ldo = (8, 3 * D + 40, D + 24) if pad else (0, 3 * D, D)
        self.big = torch.full((B * L, self.ld), float("nan"), device="cuda")
        self.xp = self.big[:, self.off:self.off + 3 * D]
        ops.pack_rows_g8(x.cuda(), self.sc, out=self.xp)
        dec = unpack_g8(self.xp.contiguous().cpu(), self.sc.cpu(), 3 * D)
        self.q, self.k, self.v = (dec[:, i * D:(i + 1) * D].reshape(B, L, D) for i in range(3))      # fp64, exactly what the kernel reads
        self.v_bound = float(self.v.abs().max()) * 1.01

    def run(self, code, force=True):
        obig = torch.full((self.B * self.L + 8, self.ldo), SENTINEL, device="cuda")
        out = obig[:self.B * self.L, self.off:self.off + self.D]
        so = torch.full((self.B * self.L + 8,), SENTINEL, device="cuda")
        with forced_packed(self.lib, *(PACKED_FORCE[code] if force else (0, 0))):
            self.ops.attention_packed(self.xp, self.sc, out, so, self.B, self.H, self.L, 64, self.scale, self.v_bound)
            ran = self.lib.psam_attention_packed_last_instance()
        torch.cuda.synchronize()
        assert ran == code, f"asked for packed instance {code}, the library ran {ran} (H {self.H} B {self.B} L {self.L}; CU-count dependent dispatch?)"
        guard = obig.clone()
        guard[:self.B * self.L, self.off:self.off + self.D] = SENTINEL
        assert (guard == SENTINEL).all(), "the kernel wrote outside its output window (padding columns / rows past the end)"
        assert (so[self.B * self.L:] == SENTINEL).all()
        so = so[:self.B * self.L]
        assert (so == so[0]).all() and float(torch.log2(so[0])) == round(float(torch.log2(so[0]))) and self.v_bound * float(so[0]) < 2.0 ** 15
        return out.contiguous(), so

    def decode(self, out, so):
        return unpack_g8(out.cpu(), so.cpu(), self.D).view(self.B, self.L, self.D)


def _packed_random(ops, c):
    g = torch.Generator().manual_seed(c.H * 1000 + c.L + c.B)
    H, B, L, D = c.H, c.B, c.L, c.H * 64
    q = torch.randn(B, L, D, generator=g) * 1.7
    k = torch.randn(B, L, D, generator=g) * 0.6
    v = torch.randn(B, L, D, generator=g) * torch.exp(torch.randn(B, L, 1, generator=g))
    v[1::2] *= 64.0                                                       # V magnitudes 2^6 apart between clouds
    k[B - 1, L - 3, (H - 1) * 64:] = q[B - 1, min(7, L - 1), (H - 1) * 64:] * 2.0      # a key that dominates late (forces the online-softmax rescale)
    return PackedProblem(ops, H, B, L, c.slack, c.pad, q, k, v, 64 ** -0.5)


def _same_words(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 3 + 4. packed family
def _packed_codes(ops, L):
    codes = [code for _, code in PACKED] if L > 128 else [831]
    if ops._lib.has_experiments() and L > 128:
        codes.append(432)
    return codes


@gpu
@pytest.mark.parametrize("case", PACKED_CASES + PACKED_ONE_BLOCK, ids=lambda c: f"H{c.H}-B{c.B}-L{c.L}-x{c.slack:g}{'-pad' if c.pad else ''}")
def test_packed_instances_match_fp64_and_each_other(ops, case):
    """<8>, <4> and <4, 2> (and <4, 3, 2> in an experiments build), each forced and confirmed, on one case: repeatable over three runs, identical words of
    `out` and `o_scale` across the instances (per query row they do the same arithmetic in the same order; waves and ring change only the staging), nothing
    written outside the output window, and the decoded output against the fp64 SDPA of the decoded packed rows in the per-(cloud, head) measure within
    4 x the fp32 evaluation's error + 2e-7.  The shapes 256 CUs send to <8> by themselves also run unforced (variant 0)."""
    pr = _packed_random(ops, case)
    ref = Reference(pr.q, pr.k, pr.v, pr.H, pr.scale)
    _header(f"packed H={case.H} B={case.B} L={case.L} bound x{case.slack:g} pad={case.pad}")
    first = None
    for code in _packed_codes(ops, case.L):
        runs = [pr.run(code) for _ in range(3)]
        for o, s in runs[1:]:
            assert _same_words(o, runs[0][0]) and _same_words(s, runs[0][1]), f"instance {code}: not repeatable"
        ref.check(pr.decode(*runs[0]), f"packed {code} H={case.H} B={case.B} L={case.L} x{case.slack:g}{' pad' if case.pad else ''}")
        if first is None:
            first = (code, runs[0])
        else:
            assert _same_words(runs[0][1], first[1][1]), f"o_scale of instance {code} differs from {first[0]}"
            assert _same_words(runs[0][0], first[1][0]), f"out of instance {code} differs from {first[0]} in " \
                                                         f"{int((runs[0][0].view(torch.int32) != first[1][0].view(torch.int32)).sum())} words"
    if -(-case.L // 256) * case.H * case.B >= NCU or case.L <= 128:      # production's own route to <8>
        o, s = pr.run(831, force=False)
        assert _same_words(o, first[1][0]) and _same_words(s, first[1][1])


@gpu
def test_packed_forced_variant_runs_as_forced_or_is_refused(ops):
    """psam_attention_packed_force_variant(v) for a v the build cannot run -- 2 without PSAM_BUILD_EXPERIMENTS, anything above -- and a forced workgroup shape
    other than 4 / 8 waves are REFUSED (the GEMM rule: a forced configuration runs as forced or not at all): error status, last_instance -1, nothing written."""
    lib = ops._lib.load()
    pr = _packed_random(ops, PackedCase(3, 2, 300, 8.0, False))
    out = torch.full((pr.B * pr.L, pr.D), SENTINEL, device="cuda")
    so = torch.full((pr.B * pr.L,), SENTINEL, device="cuda")
    call = lambda: lib.psam_attention_packed(pr.xp.data_ptr(), pr.ld, pr.sc.data_ptr(), out.data_ptr(), pr.D, so.data_ptr(), pr.B, pr.H, pr.L, 64, pr.scale,
                                             pr.v_bound, torch.cuda.current_stream().cuda_stream)
    refused = [(3, 0), (7, 0), (0, 5), (1, 2)] + ([] if ops._lib.has_experiments() else [(2, 0)])
    for variant, nw in refused:
        with forced_packed(lib, variant, nw):
            rc = call()
            assert rc != 0 and lib.psam_attention_packed_last_instance() == -1, (variant, nw, rc)
            assert b"variant" in lib.psam_last_error_string() or b"workgroup shape" in lib.psam_last_error_string()
        torch.cuda.synchronize()
        assert (out == SENTINEL).all() and (so == SENTINEL).all(), (variant, nw)
    if ops._lib.has_experiments():
        pr.run(432)
    # what the variant does not decide: one query block always runs <8>; a forced shape wins over the variant
    with forced_packed(lib, 1, 8):
        assert call() == 0 and lib.psam_attention_packed_last_instance() == 831
    with forced_packed(lib, 1, 4):
        assert call() == 0 and lib.psam_attention_packed_last_instance() == 431
    small = _packed_random(ops, PackedCase(3, 2, 128, 8.0, False))
    for variant in (0, 1):
        with forced_packed(lib, variant, 0):
            small.ops.attention_packed(small.xp, small.sc, out[:small.B * small.L], so[:small.B * small.L], small.B, small.H, small.L, 64, small.scale, small.v_bound)
            assert lib.psam_attention_packed_last_instance() == 831
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. f16x3 and f32 families
def f16x3_launch(ops, q, k, v, out, B, H, Lq, Lk, hd, scale, max_keysplit):
    """psam_attention_f16x3_ex2 called directly on 2-D row views: (status, last_instance, last_keysplit)."""
    lib = ops._lib.load()
    nb = int(lib.psam_attention_f16x3_keysplit_ws_bytes(B, H, Lq, Lk, hd, max_keysplit)) if max_keysplit > 1 else 0
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
    cnt = ops.arrival_counters(out.device)
    rc = lib.psam_attention_f16x3_ex2(q.data_ptr(), q.stride(0), Lq * q.stride(0), k.data_ptr(), k.stride(0), Lk * k.stride(0), v.data_ptr(), v.stride(0),
                                      Lk * v.stride(0), out.data_ptr(), out.stride(0), Lq * out.stride(0), B, H, Lq, Lk, hd, scale, None, 0.0, 0.0, None,
                                      max_keysplit, ws.data_ptr() if nb else None, nb, cnt.data_ptr() if nb else None, torch.cuda.current_stream().cuda_stream)
    st = (rc, lib.psam_attention_f16x3_last_instance(), lib.psam_attention_f16x3_last_keysplit())
    torch.cuda.synchronize()
    return st


def _random_qkv(B, H, Lq, Lk, hd, seed):
    g = torch.Generator().manual_seed(seed)
    D = H * hd
    q = torch.randn(B, Lq, D, generator=g) * torch.exp(0.5 * torch.randn(B, Lq, 1, generator=g)) * 1.7
    k = torch.randn(B, Lk, D, generator=g) * 0.6
    v = torch.randn(B, Lk, D, generator=g) * torch.exp(torch.randn(B, Lk, 1, generator=g))
    v[1::2] *= 64.0
    k[B - 1, Lk - 3, (H - 1) * hd:] = q[B - 1, 7, (H - 1) * hd:] * 2.0
    return q, k, v


def _guarded_out(rows, D):
    buf = torch.full((rows + 8, D), SENTINEL, device="cuda")
    return buf, buf[:rows]


_REFS = {}


def _plain_reference(hd):
    """One fp64 reference per head dim at the ragged shape, shared by the f32 and f16x3 tests."""
    if hd not in _REFS:
        q, k, v = _random_qkv(2, 3, *F16X3_PLAIN, hd, seed=hd)
        _REFS[hd] = (q, k, v, Reference(q, k, v, 3, hd ** -0.5))
    return _REFS[hd]


@gpu
@pytest.mark.parametrize("hd", F16X3_HDS)
def test_f16x3_instances_match_fp64(ops, hd):
    """Every head dim of the fp32-input f16x3 attention on the instance the registry names (64 / 96 / 128 channels, confirmed), unsplit, Lq != Lk, against
    fp64 in the per-(cloud, head) measure; repeatable over three runs."""
    B, H, (Lq, Lk) = 2, 3, F16X3_PLAIN
    q, k, v, ref = _plain_reference(hd)
    qd, kd, vd = (t.cuda().view(-1, H * hd) for t in (q, k, v))
    _header(f"f16x3 hd={hd} Lq={Lq} Lk={Lk}")
    outs = []
    for rep in range(3):
        buf, out = _guarded_out(B * Lq, H * hd)
        st = f16x3_launch(ops, qd, kd, vd, out, B, H, Lq, Lk, hd, hd ** -0.5, 1)
        assert st == (0, F16X3_OF_HD[hd], 1), st
        assert (buf[B * Lq:] == SENTINEL).all()
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), "not repeatable"
    ref.check(outs[0].cpu().view(B, Lq, H * hd), f"f16x3 <{F16X3_OF_HD[hd]}> hd={hd} {Lq}x{Lk} ks=1")


@gpu
@pytest.mark.parametrize("hd", F32_HDS)
def test_f32_instances_match_fp64(ops, hd):
    """The eight head dims of the fp32 MFMA attention at the same ragged Lq, Lk, each confirmed by psam_attention_f32_last_instance."""
    B, H, (Lq, Lk) = 2, 3, F16X3_PLAIN
    lib = ops._lib.load()
    q, k, v, ref = _plain_reference(hd)
    qd, kd, vd = (t.cuda().view(-1, H * hd) for t in (q, k, v))
    _header(f"f32 hd={hd} Lq={Lq} Lk={Lk}")
    buf, out = _guarded_out(B * Lq, H * hd)
    with ops.gemm_mode("f32"):
        ops.attention(qd, kd, vd, out, B, H, Lq, Lk, hd, hd ** -0.5)
    assert lib.psam_attention_f32_last_instance() == hd
    torch.cuda.synchronize()
    assert (buf[B * Lq:] == SENTINEL).all()
    ref.check(out.cpu().view(B, Lq, H * hd), f"f32 hd={hd} {Lq}x{Lk}")


@gpu
@pytest.mark.parametrize("case", F16X3_SPLIT, ids=lambda c: f"ks{c.ks}-{c.Lq}x{c.Lk}")
def test_f16x3_key_split_factors(ops, case):
    """Key-split factors 2, 3 and 4 asked for through max_keysplit of psam_attention_f16x3_ex2 and confirmed by last_keysplit, on both channel layouts
    (head dims 72, 88: <128, 96>; 104, 128: <128>), Lq != Lk, tile counts 2 ks, divisible and not: against fp64 in the per-(cloud, head) measure, repeatable;
    max_keysplit = 1 on the same shape runs unsplit."""
    B, H, (ks, Lq, Lk) = SPLIT_B, SPLIT_H, case
    _header(f"f16x3 key split ks={ks} Lq={Lq} Lk={Lk} ({-(-Lk // 64)} tiles)")
    for hd in F16X3_SPLIT_HDS:
        q, k, v = _random_qkv(B, H, Lq, Lk, hd, seed=hd + Lk)
        v[:, Lk // 2:] *= 32.0      # the splits carry different V-tile scales
        ref = Reference(q, k, v, H, hd ** -0.5)
        qd, kd, vd = (t.cuda().view(-1, H * hd) for t in (q, k, v))
        outs = []
        for rep in range(3):
            buf, out = _guarded_out(B * Lq, H * hd)
            st = f16x3_launch(ops, qd, kd, vd, out, B, H, Lq, Lk, hd, hd ** -0.5, ks)
            assert st == (0, F16X3_OF_HD[hd], ks), (st, "expected split", ks)
            assert (buf[B * Lq:] == SENTINEL).all()
            outs.append(out)
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), f"hd {hd}: not repeatable"
        ref.check(outs[0].cpu().view(B, Lq, H * hd), f"f16x3 <{F16X3_OF_HD[hd]}> hd={hd} {Lq}x{Lk} ks={ks}")
        buf, out = _guarded_out(B * Lq, H * hd)
        assert f16x3_launch(ops, qd, kd, vd, out, B, H, Lq, Lk, hd, hd ** -0.5, 1) == (0, F16X3_OF_HD[hd], 1)
        ref.check(out.cpu().view(B, Lq, H * hd), f"f16x3 <{F16X3_OF_HD[hd]}> hd={hd} {Lq}x{Lk} ks=1")


@gpu
def test_f16x3_key_split_switches(ops):
    """psam_attention_f16x3_force_keysplit(0) switches the split off whatever max_keysplit asks; head dim 64 never splits; the split's packed output
    (Lq == Lk) is the packing of its plain output."""
    lib = ops._lib.load()
    B, H, L, hd = SPLIT_B, SPLIT_H, 500, 88
    q, k, v = _random_qkv(B, H, L, L, hd, seed=5)
    qd, kd, vd = (t.cuda().view(-1, H * hd) for t in (q, k, v))
    out = torch.empty(B * L, H * hd, device="cuda")
    try:
        lib.psam_attention_f16x3_force_keysplit(0)
        assert f16x3_launch(ops, qd, kd, vd, out, B, H, L, L, hd, hd ** -0.5, 4) == (0, 96, 1)
    finally:
        lib.psam_attention_f16x3_force_keysplit(-1)
    assert f16x3_launch(ops, qd, kd, vd, out, B, H, L, L, hd, hd ** -0.5, 4) == (0, 96, 4)
    q64, k64, v64 = (t.cuda().view(-1, H * 64) for t in _random_qkv(B, H, L, L, 64, seed=6))
    out64 = torch.empty(B * L, H * 64, device="cuda")
    assert f16x3_launch(ops, q64, k64, v64, out64, B, H, L, L, 64, 0.125, 4) == (0, 64, 1)
    for ks in (2, 3, 4):
        with ops.gemm_mode("f16x3"), ops.attention_keysplit(ks):
            plain = torch.empty(B * L, H * hd, device="cuda")
            ops.attention(qd, kd, vd, plain, B, H, L, L, hd, hd ** -0.5)
            assert lib.psam_attention_f16x3_last_keysplit() == ks
            got = torch.empty(B * L, ops.packed_cols(H * hd), device="cuda"); so = torch.empty(B * L, device="cuda")
            ops.attention(qd, kd, vd, got[:, :H * hd], B, H, L, L, hd, hd ** -0.5, pack=(torch.ones(B * L, device="cuda"), float(v.abs().max()) * 1.1, 0.0, so))
            assert lib.psam_attention_f16x3_last_keysplit() == ks
            assert _same_words(got[:, :H * hd].contiguous(), ops.pack_rows_g8(plain, so)[:, :H * hd].contiguous())


# ------------------------------------------------------------------------------------------------ 5. one-hot selection
def _onehot_header(title):
    print(f"\n{title}\n| case | largest |out - V[pi(i)]| / |V[pi(i)]| | bound |\n|---|---|---|")


@gpu
@pytest.mark.parametrize("L", ONEHOT_PACKED_L)
def test_onehot_selection_packed(ops, L):
    """The chain "key j's score multiplies V row j of the same head of the same cloud" through the DMA source swizzle, the transposing LDS read, the tile ring
    and the S^T register-to-key map, for every packed instance: with q_i = k_pi(i) and a logit gap >= 64 the decoded output row i IS V row pi(i)."""
    B, H = 2, 3
    q, k, v, pi, scale = onehot_inputs(B, H, L, L, 64, seed=L)
    pr = PackedProblem(ops, H, B, L, 8.0, L % 2 == 1, q, k, v, scale)
    assert torch.equal(pr.v.float(), v), "V must survive the packing exactly"
    onehot_precondition(pr.q, pr.k, pi, H, scale)      # on the values the kernel reads (q and k rounded to 22 bits by the packing)
    _onehot_header(f"one-hot packed L={L}")
    for code in _packed_codes(ops, L):
        onehot_check(pr.decode(*pr.run(code)), v, pi, H, f"packed {code} L={L}")


@gpu
@pytest.mark.parametrize("hd", sorted(set(F16X3_HDS) | set(F32_HDS)))
def test_onehot_selection_f16x3_and_f32(ops, hd):
    B, H, (Lq, Lk) = 2, 3, F16X3_PLAIN
    lib = ops._lib.load()
    q, k, v, pi, scale = onehot_inputs(B, H, Lq, Lk, hd, seed=hd)
    qd, kd, vd = (t.cuda().view(-1, H * hd) for t in (q, k, v))
    _onehot_header(f"one-hot hd={hd} Lq={Lq} Lk={Lk}")
    if hd in F16X3_OF_HD:
        buf, out = _guarded_out(B * Lq, H * hd)
        assert f16x3_launch(ops, qd, kd, vd, out, B, H, Lq, Lk, hd, scale, 1) == (0, F16X3_OF_HD[hd], 1)
        assert (buf[B * Lq:] == SENTINEL).all()
        onehot_check(out.cpu().view(B, Lq, H * hd), v, pi, H, f"f16x3 <{F16X3_OF_HD[hd]}> hd={hd}")
    if hd in F32_HDS:
        buf, out = _guarded_out(B * Lq, H * hd)
        with ops.gemm_mode("f32"):
            ops.attention(qd, kd, vd, out, B, H, Lq, Lk, hd, scale)
        assert lib.psam_attention_f32_last_instance() == hd
        torch.cuda.synchronize()
        assert (buf[B * Lq:] == SENTINEL).all()
        onehot_check(out.cpu().view(B, Lq, H * hd), v, pi, H, f"f32 hd={hd}")


@gpu
@pytest.mark.parametrize("case", F16X3_SPLIT, ids=lambda c: f"ks{c.ks}-{c.Lq}x{c.Lk}")
def test_onehot_selection_f16x3_key_split(ops, case):
    """One-hot selection under the key split: the queries of every (cloud, head) select keys in every split, so each row's result comes out of the combine
    of one split that holds everything and others that hold nothing."""
    B, H, (ks, Lq, Lk) = SPLIT_B, SPLIT_H, case
    _onehot_header(f"one-hot key split ks={ks} Lq={Lq} Lk={Lk}")
    for hd in (88, 128):
        q, k, v, pi, scale = onehot_inputs(B, H, Lq, Lk, hd, seed=hd + Lk)
        nt = -(-Lk // 64)
        part = torch.bucketize(pi, torch.tensor([s * nt // ks * 64 for s in range(1, ks)]), right=True)      # split s walks tiles [s nt / ks, (s + 1) nt / ks)
        assert all(len(set(part[b, h].tolist())) == ks for b in range(B) for h in range(H)), "pi must send queries to keys in every split"
        qd, kd, vd = (t.cuda().view(-1, H * hd) for t in (q, k, v))
        buf, out = _guarded_out(B * Lq, H * hd)
        assert f16x3_launch(ops, qd, kd, vd, out, B, H, Lq, Lk, hd, scale, ks) == (0, F16X3_OF_HD[hd], ks)
        assert (buf[B * Lq:] == SENTINEL).all()
        onehot_check(out.cpu().view(B, Lq, H * hd), v, pi, H, f"f16x3 <{F16X3_OF_HD[hd]}> hd={hd} ks={ks}")


@gpu
@pytest.mark.parametrize("code,hd,H,Z,Lq,Lk", SMALL_CASES)
def test_onehot_selection_small(ops, code, hd, H, Z, Lq, Lk):
    """The four kernels behind psam_attention_small, each confirmed by psam_attention_small_last_instance."""
    lib = ops._lib.load()
    q, k, v, pi, scale = onehot_inputs(Z, H, Lq, Lk, hd, seed=Lk + hd)
    qd, kd, vd = (t.cuda().view(-1, H * hd) for t in (q, k, v))
    _onehot_header(f"one-hot small kernel {code} hd={hd} Lq={Lq} Lk={Lk}")
    buf, out = _guarded_out(Z * Lq, H * hd)
    try:
        lib.psam_attention_small_force_split(1 if code == 1 else 0)
        ops.attention_small(qd, kd, vd, out, Z, H, Lq, Lk, hd, scale)
        assert lib.psam_attention_small_last_instance() == code
    finally:
        lib.psam_attention_small_force_split(1)
    torch.cuda.synchronize()
    assert (buf[Z * Lq:] == SENTINEL).all()
    onehot_check(out.cpu().view(Z, Lq, H * hd), v, pi, H, f"small {code} hd={hd} {Lq}x{Lk}")


# ------------------------------------------------------------------------------------------------ 6. environment switches, 4. <128, 96> == <128>
ENV_PACKED = PackedCase(3, 2, 300, 8.0, True)
ENV_F16X3 = (SPLIT_B, SPLIT_H, 200, 500)      # B, H, Lq, Lk: splits four ways by default (12 units on 256 CUs, 8 tiles)
ENV_HDS = (72, 80, 88, 96)
ENV_MODES = [("PSAM_ATTN_VARIANT", "0"), ("PSAM_ATTN_VARIANT", "1"), ("PSAM_ATTN_PACKED_NW", "4"), ("PSAM_ATTN_PACKED_NW", "8"), ("PSAM_ATTN_KEYSPLIT", "0"),
             ("PSAM_ATTN_FULL_WIDTH", "1")]


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def _env_case(o, packed_force=None, keysplit_force=None):
    """The fixed case of the environment test: one packed launch and, per head dim in (64, 96], one unsplit and one default-split f16x3 launch.
    packed_force: instance code to force by hook (None: whatever the process picks); keysplit_force: psam_attention_f16x3_force_keysplit mode."""
    lib = o._lib.load()
    res = {}
    pr = _packed_random(o, ENV_PACKED)
    if packed_force is None:
        out = torch.full((pr.B * pr.L, pr.ldo), SENTINEL, device="cuda")
        so = torch.empty(pr.B * pr.L, device="cuda")
        w = out[:, pr.off:pr.off + pr.D]
        o.attention_packed(pr.xp, pr.sc, w, so, pr.B, pr.H, pr.L, 64, pr.scale, pr.v_bound)
        res["packed"] = dict(inst=lib.psam_attention_packed_last_instance(), sha=_sha(w), sha_scale=_sha(so))
    else:
        w, so = pr.run(packed_force)
        res["packed"] = dict(inst=packed_force, sha=_sha(w), sha_scale=_sha(so))
    B, H, Lq, Lk = ENV_F16X3
    try:
        if keysplit_force is not None:
            lib.psam_attention_f16x3_force_keysplit(keysplit_force)
        for hd in ENV_HDS:
            qd, kd, vd = (t.cuda().view(-1, H * hd) for t in _random_qkv(B, H, Lq, Lk, hd, seed=hd))
            for cap in (1, 4):
                out = torch.empty(B * Lq, H * hd, device="cuda")
                rc, inst, ks = f16x3_launch(o, qd, kd, vd, out, B, H, Lq, Lk, hd, hd ** -0.5, cap)
                res[f"hd{hd}_cap{cap}"] = dict(rc=rc, inst=inst, ks=ks, sha=_sha(out), finite=bool(torch.isfinite(out).all()))
    finally:
        if keysplit_force is not None:
            lib.psam_attention_f16x3_force_keysplit(-1)
    return res


def _child_main(path):
    sys.path.insert(0, ROOT)
    from point_sam_amd import ops as o
    o._lib.load()
    with open(path, "w") as f:
        json.dump(_env_case(o), f)


def _child(tmp_path, env_set):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PSAM_ATTN_")}
    env.update(env_set)
    out = str(tmp_path / ("child_" + "_".join(f"{k}{v}" for k, v in env_set.items()) + ".json"))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--attention-instance-child", out]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)      # a failing child raises here: nothing further starts
    assert r.returncode == 0, (env_set, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.load(open(out))


@gpu
def test_environment_switches_in_child_processes(ops, tmp_path):
    """PSAM_ATTN_VARIANT=0/1, PSAM_ATTN_PACKED_NW=4/8, PSAM_ATTN_KEYSPLIT=0 and PSAM_ATTN_FULL_WIDTH=1 are read once per process: one fresh child per
    setting, one after another, each under its own time limit.  The instance / split the switch names ran, and the output has the bits of the same
    instance forced by hook in this process -- for PSAM_ATTN_FULL_WIDTH=1 the bits of the <128, 96> instance ("same bits": the products with the zero
    padding add exact zeros), at head dims 72 to 96, unsplit and split."""
    here = {code: _env_case(ops, packed_force=code)["packed"] for code in (831, 431, 421)}
    f16 = _env_case(ops, packed_force=421)
    off = _env_case(ops, packed_force=421, keysplit_force=0)
    for hd in ENV_HDS:
        assert (f16[f"hd{hd}_cap1"]["inst"], f16[f"hd{hd}_cap1"]["ks"], f16[f"hd{hd}_cap4"]["ks"]) == (96, 1, 4), (hd, f16)
        assert off[f"hd{hd}_cap4"]["ks"] == 1 and off[f"hd{hd}_cap4"]["sha"] == f16[f"hd{hd}_cap1"]["sha"]
    expect_packed = {("PSAM_ATTN_VARIANT", "0"): 431, ("PSAM_ATTN_VARIANT", "1"): 421, ("PSAM_ATTN_PACKED_NW", "4"): 431, ("PSAM_ATTN_PACKED_NW", "8"): 831}
    for k, v in [(None, None)] + ENV_MODES:
        got = _child(tmp_path, {k: v} if k else {})
        inst = expect_packed.get((k, v), 421)      # the default process: variant 1
        assert got["packed"]["inst"] == inst, (k, v, got["packed"])
        assert got["packed"]["sha"] == here[inst]["sha"] and got["packed"]["sha_scale"] == here[inst]["sha_scale"], (k, v, "packed bits differ from the hook's")
        for hd in ENV_HDS:
            for cap in (1, 4):
                r, name = got[f"hd{hd}_cap{cap}"], f"hd{hd}_cap{cap}"
                assert r["rc"] == 0 and r["finite"], (k, v, name, r)
                assert r["inst"] == (128 if k == "PSAM_ATTN_FULL_WIDTH" else 96), (k, v, name, r)
                assert r["ks"] == (1 if k == "PSAM_ATTN_KEYSPLIT" else cap), (k, v, name, r)
                assert r["sha"] == (off if k == "PSAM_ATTN_KEYSPLIT" else f16)[name]["sha"], (k, v, name, "bits differ from this process's")


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--attention-instance-child":
    _child_main(sys.argv[2])
