"""Every launchable FPS, kNN and 3-NN kernel instance of csrc/tokenizer.hip, checked on its own.

The search kernels are bit-exact against oracle/tokenizer_oracle.c by contract: farthest point sampling (`fps_kernel<PPT4>` for one workgroup per cloud with
PPT4 = 1 .. 8 groups of 4096 points in registers / LDS and 0 = streamed; `fps_coop_kernel<1|2|4>` and `fps_coop_pruned_kernel<1|2|4>` for W workgroups per
cloud that hand tagged 64-bit keys to each other), the K nearest neighbours (`knn_kernel`, `knn_band_kernel`), the three nearest centres of every point
(`three_nn_kernel`) and the border-farthest search.  INSTANCES lists the 17 FPS / kNN instances with the code `psam_fps_last_instance` /
`psam_knn_last_instance` reports; a CPU test keeps it equal to the launch sites of the source (FPS_LAUNCH / FPS_COOP / FPS_COOP_PRUNED expanded), another
pins the constants that `fps_dispatch`, the Python model of psam_fps / fps_coop_ppt4, copies from the source, so an instance added or a threshold moved fails
without a GPU.  On the GPU every case
  * equals the C oracle bit for bit and ran as the instance (and grid width) the model predicts for the device's CU count;
  * passes an fp64 check that does not share the oracle's arithmetic: for FPS a greedy-validity replay (the chosen point's fp64 min-distance is within
    2^-20 of the largest one: an fp32 d2 carries four roundings, <= 2^-22 relative on each side of a comparison, 2^-21, doubled), for kNN a partition check
    (distinct indices, max d64(returned) <= min d64(not returned) (1 + 2^-20), ascending within the same slack), for 3-NN the weights at 1e-6;
  * sits on an edge: both ends of every single-workgroup instance, W <= 16 and W > 16 of every cooperative one (row-wide and wave-wide key maximum), the
    one-XCD placement and without, nine clouds, the wrap of the 12-bit iteration tag (G = 4200), the last index the 20-bit key field admits (N = 2^20), each
    inner path of the kNN kernels (band fits / overflows KNN_CAND, tie cut at the K-th value or not), K = 1 .. KNN_MAXK, N < 4, clouds off 16-byte
    boundaries, 3-NN with more than 64 KiB of dynamic LDS up to the guard's limit.
The last test asserts that the run confirmed every code of the registry at least once (it needs the other GPU tests of this file in the same session)."""
import functools
import math
import os
import re
import threading
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import pointsam_oracle as O
from test_gpu_kernels import _clustered_cloud
from test_gpu_row_instances import launched_instances

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOKENIZER = os.path.join(ROOT, "point_sam_amd", "csrc", "tokenizer.hip")
gpu = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------ 1. the registry
# family: fps | knn (one `psam_<family>_last_instance` query each).  code: what the query reports after this instance ran (fps: kind * 100 + PPT4).
Inst = namedtuple("Inst", "family code reach")
INSTANCES = {
    **{f"fps_kernel<{p}>": Inst("fps", p, f"{4096 * (p - 1)} < N <= {4096 * p}, not cooperative") for p in range(1, 9)},
    "fps_kernel<0>": Inst("fps", 0, "N > 32768, not cooperative (streaming)"),
    **{f"fps_coop_kernel<{p}>": Inst("fps", 100 + p, f"cooperative, {p} groups of 4096 points per workgroup, pruning off") for p in (1, 2, 4)},
    **{f"fps_coop_pruned_kernel<{p}>": Inst("fps", 200 + p, f"cooperative, {p} groups of 4096 points per workgroup, pruning on") for p in (1, 2, 4)},
    "knn_kernel": Inst("knn", 0, "psam_knn_force_band(0)"),
    "knn_band_kernel": Inst("knn", 1, "psam_knn_force_band(1) (the default)"),
}
KERNELS = ("fps_kernel", "fps_coop_kernel", "fps_coop_pruned_kernel", "knn_kernel", "knn_band_kernel")
QUERIES = ("psam_fps_last_instance", "psam_fps_last_grid_x", "psam_knn_last_instance")
TUNING_ENV = ("PSAM_FPS_COOP_PPT4", "PSAM_FPS_COOP_MIN_GROUPS", "PSAM_FPS_PRUNE", "PSAM_KNN_BAND")      # read once by the library: would make the model wrong

# the constants fps_dispatch and the kNN cases copy from the source; pinned_constants() parses the same ones out of it
GROUP = 4096          # points per group: four per thread of a 1024-thread workgroup
MODEL = {"fps_threads": 1024, "min_groups": 8, "ppt4_max": 4, "ppt4_loop": "1..4 doubling", "w_max": 64, "w_stop": 16, "groups8_max_b": 2, "n_max_shift": 20,
         "b_max": 1024, "xs_rule": "W * cdiv(B, 8) <= cus / 8 and mode != 2", "single_max_groups": 8, "knn_cand": 2048, "knn_maxk": 1024, "knn_top_shift": 21}


def _cdiv(a, b):
    return -(-a // b)


def fps_groups(N):
    return _cdiv(N, GROUP)


def fps_coop_ppt4(B, N, cus):
    """fps_coop_ppt4 of the source: (PPT4, W), PPT4 = 0 when the cloud does not go cooperative."""
    groups = fps_groups(N)
    if groups < MODEL["min_groups"] or N > (1 << MODEL["n_max_shift"]) or B > MODEL["b_max"]:
        return 0, 0
    if groups == 8:
        return (0, 0) if B > MODEL["groups8_max_b"] else (1, 8)
    best, W = 0, 0
    for ppt4 in (1, 2, 4):
        if ppt4 > MODEL["ppt4_max"]:
            break
        w = groups // ppt4
        if groups % ppt4 != 0 or w > MODEL["w_max"] or B * w > cus:
            continue
        best, W = ppt4, w
        if w <= MODEL["w_stop"]:
            break
    return best, W


def fps_dispatch(B, N, cus, coop_mode, prune):
    """(code, grid_x) of psam_fps: what psam_fps_last_instance / psam_fps_last_grid_x report after the call.  coop_mode: psam_fps_set_cooperative's
    argument (0 = never cooperative, 1 = default, 2 = cooperative without the one-XCD placement); prune: psam_fps_set_pruning's (0 / 1)."""
    ppt4, W = fps_coop_ppt4(B, N, cus) if coop_mode else (0, 0)
    if ppt4:
        xs = 8 if (W * _cdiv(B, 8) <= cus // 8 and coop_mode != 2) else 1
        return (200 if prune else 100) + ppt4, W * xs
    groups = fps_groups(N)
    return (groups if groups <= MODEL["single_max_groups"] else 0), 0


# ------------------------------------------------------------------------------------------------ source parsing (CPU)
def _src():
    return open(TOKENIZER).read()


def pinned_constants(src):
    """The constants of MODEL as the source text states them (None / a different value where a statement was edited)."""
    text = re.sub(r"\s+", " ", re.sub(r"//[^\n]*", "", src))

    def num(pattern):
        m = re.search(pattern, text)
        return int(m.group(1)) if m else None

    def has(literal, value):
        return value if literal in text else None

    return {
        "fps_threads": num(r"constexpr int FPS_THREADS = (\d+);"),
        "min_groups": num(r'k_min_groups\("PSAM_FPS_COOP_MIN_GROUPS", (\d+)\); const int [^;]* min_groups = k_min_groups\.get_positive\(\);'),
        "ppt4_max": num(r'k_ppt4_max\("PSAM_FPS_COOP_PPT4", (\d+)\), [^;]*; const int ppt4_max = k_ppt4_max\.get_positive\(\),'),
        "ppt4_loop": has("for (int ppt4 = 1; ppt4 <= 4 && ppt4 <= ppt4_max; ppt4 *= 2) {", "1..4 doubling"),
        "w_max": num(r"if \(groups % ppt4 != 0 \|\| w > (\d+) \|\| \(int64_t\)B \* w > psam_cu_count\(\)\) continue;"),
        "w_stop": num(r"best = ppt4; \*W = \(int\)w; if \(w <= (\d+)\) break;"),
        "groups8_max_b": num(r"if \(groups == 8\) \{ if \(B > (\d+) \|\| ppt4_max < 1\) return 0; \*W = 8; return 1; \}"),
        "n_max_shift": num(r"if \(groups < min_groups \|\| N > \(1 << (\d+)\) \|\| B > 1024\) return 0;"),
        "b_max": num(r"if \(groups < min_groups \|\| N > \(1 << 20\) \|\| B > (\d+)\) return 0;"),
        "xs_rule": has("const int xs = ((int64_t)W * psam_cdiv(B, 8) <= psam_cu_count() / 8 && coop_mode != 2) ? 8 : 1;", "W * cdiv(B, 8) <= cus / 8 and mode != 2"),
        "single_max_groups": num(r"case (\d+): FPS_LAUNCH\(\d+\); break; default: FPS_LAUNCH\(0\); break;"),
        "knn_cand": num(r"constexpr int KNN_CAND = (\d+);"),
        "knn_maxk": num(r"constexpr int KNN_MAXK = (\d+);"),
        "knn_top_shift": num(r"atomicAdd\(&hist\[u\[e\] >> (\d+)\], 1u\);"),
    }


def test_registry_matches_the_launch_sites():
    """INSTANCES == the instantiations of the five kernels that csrc/tokenizer.hip launches (macros expanded); the codes follow the documented rule; the
    single-workgroup switch maps `groups` to the instance of the same number; the header declares the three queries and the Python binding knows them."""
    src = _src()
    assert launched_instances(src, KERNELS) == set(INSTANCES), (sorted(launched_instances(src, KERNELS) ^ set(INSTANCES)), "launched by the source vs listed in INSTANCES")
    assert len(INSTANCES) == 17
    for k, i in INSTANCES.items():
        if k.startswith("fps"):
            kind = {"fps_kernel": 0, "fps_coop_kernel": 1, "fps_coop_pruned_kernel": 2}[k[:k.index("<")]]
            assert i == Inst("fps", kind * 100 + int(k[k.index("<") + 1:-1]), i.reach), k
        else:
            assert i.family == "knn" and i.code == (k == "knn_band_kernel"), k
    assert re.findall(r"case (\d+): FPS_LAUNCH\((\d+)\); break;", src) == [(str(p), str(p)) for p in range(1, 9)]
    for macro in ("FPS_COOP", "FPS_COOP_PRUNED"):
        assert "if (coop == 1) %s(1); else if (coop == 2) %s(2); else %s(4);" % (macro, macro, macro) in src
    assert "if (!band) hipLaunchKernelGGL(knn_kernel," in src and "else hipLaunchKernelGGL(knn_band_kernel," in src
    from point_sam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pointsam_hip.h")).read()
    for name in QUERIES:
        assert re.search(r"int32_t\s+%s\s*\(\s*void\s*\)\s*;" % name, hdr), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"PSAM_API int32_t %s\(void\)" % name, src), name


def test_the_parser_sees_an_edited_launch_site():
    """The registry test must fail when a launch site is added, edited or dropped."""
    src, base = _src(), set(INSTANCES)
    default = "        default: FPS_LAUNCH(0); break;"
    assert src.count(default) == 1
    assert launched_instances(src.replace(default, "        case 9: FPS_LAUNCH(9); break;\n" + default), KERNELS) - base == {"fps_kernel<9>"}
    assert src.count("else FPS_COOP(4);") == 1 and src.count("else FPS_COOP_PRUNED(4);") == 1
    assert launched_instances(src.replace("else FPS_COOP(4);", "else FPS_COOP(8);"), KERNELS) ^ base == {"fps_coop_kernel<4>", "fps_coop_kernel<8>"}
    assert launched_instances(src.replace("else FPS_COOP_PRUNED(4);", ";"), KERNELS) ^ base == {"fps_coop_pruned_kernel<4>"}
    assert src.count("        case 3: FPS_LAUNCH(3); break;\n") == 1
    assert launched_instances(src.replace("        case 3: FPS_LAUNCH(3); break;\n", ""), KERNELS) ^ base == {"fps_kernel<3>"}
    band = "    else hipLaunchKernelGGL(knn_band_kernel, dim3(G, B)"
    assert src.count(band) == 1
    assert launched_instances(src.replace(band, "    else hipLaunchKernelGGL(knn_kernel, dim3(G, B)"), KERNELS) ^ base == {"knn_band_kernel"}


def test_the_model_copies_the_constants_of_the_source():
    """fps_dispatch and the kNN cases are built around MODEL; every entry is parsed out of the source text, so a moved threshold fails here."""
    src = _src()
    assert pinned_constants(src) == MODEL
    assert GROUP == 4 * MODEL["fps_threads"]
    assert "static inline int64_t fps_npad(int64_t N) { return psam_cdiv(N, 4 * FPS_THREADS) * (4 * FPS_THREADS); }" in src
    assert "const int64_t groups = fps_npad(N) / (4 * FPS_THREADS);" in src and "const int groups = (int)(npad / (4 * FPS_THREADS));" in src
    assert "const int coop_mode = k_fps_coop.get();" in src and "const int coop = coop_mode ? fps_coop_ppt4(B, N, &W) : 0;" in src
    assert "if (n_band > KNN_CAND) {" in src and "if (eq_total != need_eq) {" in src and "if (eq_total == need_eq) {" in src
    assert 'PSAM_REQUIRE(K <= KNN_MAXK, PSAM_EINVAL, "psam_knn: K > 1024 unsupported");' in src
    assert 'PSAM_REQUIRE((size_t)G * 12 <= 144 * 1024, PSAM_EINVAL, "psam_three_nn: G too large for LDS staging");' in src
    # the hand-over key: 12-bit tag above a 20-bit index field, slots reset to all ones
    assert "const unsigned tag = (unsigned)j & 0xFFFu;" in src and "if (i < n) cand[i] = ~0ull;" in src
    for old, new in (('"PSAM_FPS_COOP_MIN_GROUPS", 8)', '"PSAM_FPS_COOP_MIN_GROUPS", 6)'), ('"PSAM_FPS_COOP_PPT4", 4)', '"PSAM_FPS_COOP_PPT4", 8)'), ("|| w > 64 ||", "|| w > 32 ||"), ("if (w <= 16) break;", "if (w <= 8) break;"),
                     ("if (B > 2 || ppt4_max < 1) return 0;", "if (B > 4 || ppt4_max < 1) return 0;"), ("N > (1 << 20)", "N > (1 << 19)"),
                     ("<= psam_cu_count() / 8 && coop_mode != 2", "<= psam_cu_count() / 4 && coop_mode != 2"), ("KNN_CAND = 2048;", "KNN_CAND = 4096;"),
                     ("KNN_MAXK = 1024;", "KNN_MAXK = 2048;"), ("ppt4 <= 4 && ppt4 <= ppt4_max", "ppt4 <= 8 && ppt4 <= ppt4_max")):
        assert src.count(old) == 1, old
        assert pinned_constants(src.replace(old, new)) != MODEL, old


# the steps that FPS and kNN kernels share, each by a piece of text only its one implementation contains
SINGLE_COPY = ("fps_sub_bcast(",                        # the scan of one group of four points (a call; the definition's own name is not in a body)
               "__hip_atomic_store(",                   # the hand-over: publishing the key ...
               "__builtin_amdgcn_s_sleep(",             # ... and polling the slots
               "0xFFFFFu -",                            # the key's index field, packed and unpacked
               "(blockIdx.x & 7) != (b & 7)",           # the one-XCD placement
               "const int ixj = i ^ jj;",               # the bitonic network
               "remaining <= before + loc[i]",          # the bin that holds rank `remaining`
               "? INFINITY : -1.0f")                    # the padding rule of the running minima
# the kernels that keep a step in place, by name, and why (profiles/tokenizer/README.md)
COOP = ("fps_coop_kernel", "fps_coop_pruned_kernel")      # placement, key and hand-over as functions: 1 - 3 % slower calls on four of six instances
KEPT_IN_PLACE = {"__hip_atomic_store(": COOP, "__builtin_amdgcn_s_sleep(": COOP, "0xFFFFFu -": COOP, "(blockIdx.x & 7) != (b & 7)": COOP,
                 "? INFINITY : -1.0f": ("fps_coop_pruned_kernel",),      # its initialisation also feeds the bounding box; with fps_md_init: other code, slower
                 "remaining <= before + loc[i]": ("knn_band_kernel",)}      # its first bin search: through knn_locate_bin the kernel needs 52 VGPRs, not 47


def function_bodies(src):
    """[(name, body)] of every function defined at file scope, comments stripped: a body is a brace block at depth 0 whose header ends in a parameter list."""
    text = re.sub(r"/\*.*?\*/", "", re.sub(r"//[^\n]*", "", src), flags=re.S)
    out, depth, start, prev = [], 0, 0, 0
    for i, ch in enumerate(text):
        if ch == "{":
            if depth == 0:
                start = i
            depth += 1
        elif ch == "}":
            depth -= 1
            assert depth >= 0, text[max(0, i - 200):i]
            if depth == 0:
                head = re.sub(r"__launch_bounds__\(\w+\)|__attribute__\(\(.*?\)\)", "", text[prev:start])
                head = head[head.rfind(";") + 1:]
                m = re.search(r"(\w+)\s*\(", head)
                if m and head.rstrip().endswith(")"):
                    out.append((m.group(1), text[start:i + 1]))
                prev = i + 1
    assert depth == 0
    return out


def holders(src, needle, kept=False):
    """The functions whose body contains `needle` (white space normalised): those listed in KEPT_IN_PLACE for it (kept=True), or all others."""
    squash = lambda s: re.sub(r"\s+", " ", s)
    return [name for name, body in function_bodies(src) if squash(needle) in squash(body) and (name in KEPT_IN_PLACE.get(needle, ())) == kept]


def test_each_shared_step_has_one_copy():
    """The scan of a group, the hand-over, the key layout, the one-XCD placement, the bitonic sort, the bin search and the padding rule are bit-exact by
    contract and were once pasted into two to four kernels each: each now sits in exactly one function body, and a copy planted back is seen."""
    src = _src()
    names = [n for n, _ in function_bodies(src)]
    for k in KERNELS + ("fps_coop_reset_kernel", "knn_select_full", "psam_fps", "psam_knn", "three_nn_kernel"):
        assert names.count(k) == 1, (k, names)
    where = {needle: holders(src, needle) for needle in SINGLE_COPY}
    for needle, v in where.items():      # one shared function; none where every kernel that needs the step keeps it in place
        assert len(v) == (0 if KEPT_IN_PLACE.get(needle) == COOP else 1), where
        assert sorted(holders(src, needle, kept=True)) == sorted(KEPT_IN_PLACE.get(needle, ())), needle      # no exception outlives its copy
    assert not set(sum(where.values(), [])) & set(KERNELS), where      # in helpers, not in a kernel
    # a copy pasted into another function
    anchor = "__global__ void fps_coop_reset_kernel(unsigned long long* cand, int n) {"
    assert src.count(anchor) == 1
    for needle in SINGLE_COPY:
        assert sorted(holders(src.replace(anchor, anchor + "\n    " + needle + " 0);"), needle)) == sorted(where[needle] + ["fps_coop_reset_kernel"]), needle
    # a call replaced by what it stands for, as the kernels had it
    for call, inline, needle, kernel in (
            ("for (int g = 0; g < PPT4; ++g) fps_visit(md[g], rx[g], ry[g], rz[g], c2x, c2y, c2z, best);",
             "for (int g = 0; g < PPT4; ++g) { const f32x4 dx = fps_sub_bcast(rx[g], c2x), dy = fps_sub_bcast(ry[g], c2y), dz = fps_sub_bcast(rz[g], c2z); }",
             "fps_sub_bcast(", "fps_coop_kernel"),
            ("md[g] = fps_md_init((gg * FPS_THREADS + tid) * 4, N);", "for (int e = 0; e < 4; ++e) md[g][e] = base + e < N ? INFINITY : -1.0f;", "? INFINITY : -1.0f",
             "fps_coop_kernel"),
            ("knn_locate_bin(hist, remaining, s_wave, sm);", "if (remaining > before && remaining <= before + loc[i]) { sm[0] = tid * 8 + i; sm[1] = before; }",
             "remaining <= before + loc[i]", "knn_pass_tail")):
        assert call in src, call
        planted = src.replace(call, inline, 1)
        assert sorted(holders(planted, needle)) == sorted(where[needle] + [kernel]), (needle, holders(planted, needle))


def test_queries_report_minus_one_before_a_launch_and_after_a_refusal():
    """No GPU needed: a thread that never launched reads -1 from the three queries, and so does one whose call was refused on the host (null pointers)."""
    from point_sam_amd import _lib
    lib = _lib.load()
    seen = []
    t = threading.Thread(target=lambda: seen.extend(getattr(lib, q)() for q in QUERIES))
    t.start(); t.join()
    assert seen == [-1, -1, -1]
    assert lib.psam_fps(None, 1, 8, 4, None, None, None, 0, None) != 0
    assert lib.psam_knn(None, None, 1, 1, 8, 4, None, None) != 0
    assert [getattr(lib, q)() for q in QUERIES] == [-1, -1, -1]


# ------------------------------------------------------------------------------------------------ 2. clouds
KINDS = ("surface", "lattice", "planted")
PLANTED_MAX_N = 150000


def planted_layout(N):
    """(far, orig, copy): the indices that hold far points -- the first and last index of every 4096-point group and N - 1 -- and one exact duplicate: the far
    point at index 4095 again in the middle of the last group (of the last but one when the last holds fewer than three points).  A cloud of one group (or
    of 4097 points) gets an extra far point at index 1 instead and its copy at N / 2: another wave of the same workgroup."""
    groups = fps_groups(N)
    far = {g * GROUP for g in range(groups)} | {min(g * GROUP + GROUP - 1, N - 1) for g in range(groups)} | {N - 1}
    last0 = (groups - 1) * GROUP
    orig = copy = None
    if groups >= 2 and N - last0 >= 3:
        orig, copy = GROUP - 1, last0 + (N - last0) // 2
    elif groups >= 3:
        orig, copy = GROUP - 1, (groups - 2) * GROUP + GROUP // 2
    elif N >= 16:
        far.add(1)
        orig, copy = 1, N // 2
    assert copy is None or (copy not in far and orig in far and orig < copy < N)
    return sorted(far), orig, copy


def _planted_cloud(B, N, seed):
    """A ball of radius 0.1 around the origin plus far points on the unit sphere (a rotated Fibonacci lattice: pairwise squared distance > 0.09, asserted).
    Once one ball point is chosen every ball point's min-distance is <= 0.2^2, below every far point's: FPS returns all far points in its first
    len(far) + 1 choices, the copy (min-distance 0 from the moment its original is chosen) never before every other point has distance 0."""
    far, orig, copy = planted_layout(N)
    g = torch.Generator().manual_seed(seed)
    n = len(far)
    i = torch.arange(n, dtype=torch.float64)
    z = 1 - (2 * i + 1) / n
    phi = i * math.pi * (3 - math.sqrt(5))
    sphere = torch.stack([(1 - z * z).sqrt() * phi.cos(), (1 - z * z).sqrt() * phi.sin(), z], 1)
    xyz = torch.empty(B, N, 3)
    for b in range(B):
        v = torch.randn(N, 3, generator=g, dtype=torch.float64)
        xyz[b] = (v / v.norm(dim=1, keepdim=True) * 0.1 * torch.rand(N, 1, generator=g, dtype=torch.float64) ** (1 / 3)).float()
        q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
        pts = (sphere @ q.T)[torch.randperm(n, generator=g)].float()
        if n > 1:
            assert (torch.cdist(pts.double(), pts.double()) + 4 * torch.eye(n)).min() ** 2 > 0.09
        xyz[b, far] = pts
        if copy is not None:
            xyz[b, copy] = xyz[b, orig]
    return xyz


@functools.lru_cache(maxsize=None)
def fps_cloud(kind, B, N, seed, extra=""):
    """[B, N, 3] fp32 on the CPU.  extra: "dup500" = 500 exact duplicates in a surface cloud; "far_last" = the farthest point of the cloud at index N - 1
    (lattice: and a duplicate of it at a lower index, in another workgroup's part of the cloud)."""
    if kind == "surface":
        xyz = O.synthetic_batch(B, N, seed=seed)[0] if N > 1 else torch.full((B, 1, 3), 0.375)      # (a cloud of one point normalises to 0 / 0)
        if extra == "dup500":
            g = torch.Generator().manual_seed(seed + 99)
            src, dst = torch.randint(0, N, (500,), generator=g), torch.randint(0, N, (500,), generator=g)
            xyz[:, dst] = xyz[:, src]
    elif kind == "lattice":
        xyz = _clustered_cloud(B, N, seed=seed)
    else:
        assert kind == "planted" and not extra
        xyz = _planted_cloud(B, N, seed)
    if extra == "far_last":
        xyz[:, N - 1] = 3.0
        if kind == "lattice":
            xyz[:, N // 2 + 5] = 3.0
    return xyz.contiguous()


def fps_G(kind, N, G):
    """The number of samples of a case: the table's, raised for a planted cloud to the number of far points + 2 (never above N)."""
    return min(N, max(G, len(planted_layout(N)[0]) + 2)) if kind == "planted" else G


@functools.lru_cache(maxsize=None)
def fps_reference(kind, B, N, G, seed, extra=""):
    """(cloud, the oracle's indices, its centres): computed once per case, shared by the CPU and the GPU tests, never modified."""
    xyz = fps_cloud(kind, B, N, seed, extra)
    want = O.fps(xyz, G)
    return xyz, want, O.batch_index_select(xyz, want)


def greedy_replay(xyz, idx):
    """The fp64 greedy-validity replay of one cloud [N, 3] and its G chosen indices: the first is 0 and every later one holds, in fp64 arithmetic on the fp32
    coordinates, a min-distance to the earlier ones within 2^-20 (relative) of the largest.  Returns the smallest md[chosen] / max(md) seen."""
    p = xyz.double().numpy()
    idx = idx.numpy()
    assert idx[0] == 0
    md = np.full(p.shape[0], np.inf)
    worst = 1.0
    for j in range(1, len(idx)):
        d = p - p[idx[j - 1]]
        np.minimum(md, np.einsum("ij,ij->i", d, d), out=md)
        m = md.max()
        assert md[idx[j]] >= m * (1 - 2.0 ** -20), f"choice {j} = point {idx[j]}: min-distance {md[idx[j]]!r}, the largest is {m!r} (point {int(md.argmax())})"
        if m > 0:
            worst = min(worst, md[idx[j]] / m)
    return worst


# ------------------------------------------------------------------------------------------------ 3. FPS cases
# single workgroup: (instance, B, N, G, forced, extra).  forced: psam_fps_set_cooperative(0), where 8 groups (or more) would otherwise go cooperative.
FpsCase = namedtuple("FpsCase", "inst B N G forced extra")
SINGLE_CASES = [FpsCase(p, 2, N, min(64, N), p == 8, "") for p in range(1, 9) for N in (GROUP * (p - 1) + 1, GROUP * p - 3)] + [
    FpsCase(1, 1, 1, 1, False, ""), FpsCase(1, 1, 3, 3, False, ""), FpsCase(1, 1, 64, 64, False, ""),
    FpsCase(2, 1, 4100, 4100, False, "dup500"),
    FpsCase(8, 3, 28673, 64, False, ""), FpsCase(8, 3, 32768, 64, False, ""),      # more than two clouds of eight groups: never cooperative
    FpsCase(0, 1, 32769, 64, True, ""),
    FpsCase(0, 30, 33000, 6, False, ""),                                          # 30 clouds x 9 workgroups exceed the CUs
    FpsCase(0, 1, (1 << 20) + 1, 4, False, ""),                                   # one past the 20-bit index field
]
# cooperative: (PPT4, W, B, N, G, extra), each with pruning off / on and psam_fps_set_cooperative(1 / 2)
CoopCase = namedtuple("CoopCase", "ppt4 W B N G extra")
COOP_CASES = [
    CoopCase(1, 8, 1, 28673, 48, ""), CoopCase(1, 8, 2, 32768, 48, ""), CoopCase(1, 9, 3, 32769, 32, ""),
    CoopCase(1, 17, 1, 69629, 32, ""),           # W > 16: the wave-wide key maximum
    CoopCase(1, 33, 1, 135165, 24, ""),          # W > 32: no one-XCD placement
    CoopCase(1, 9, 9, 33000, 12, ""),            # nine clouds: two dealt to one XCD
    CoopCase(2, 9, 1, 73725, 32, ""), CoopCase(2, 17, 1, 139261, 24, ""),
    CoopCase(4, 9, 1, 147453, 24, ""), CoopCase(4, 17, 1, 278525, 16, ""),
    CoopCase(4, 64, 1, 1 << 20, 8, "far_last"),  # index 0xFFFFF: key field 0, what a wave of pure padding publishes
]
TAG_WRAP = CoopCase(1, 8, 1, 32768, 4200, "")    # iteration 4095 carries the tag the slots are reset to, 4096 carries tag 0
REFERENCE_CUS = 256


def _kinds(N, extra=""):
    return [k for k in KINDS if k != "planted" or (N <= PLANTED_MAX_N and extra in ("", "dup500"))]


def _seed(c):
    return c.N + 7 * c.G + c.B


def _extra(c, kind):
    return "" if (kind == "planted" or (c.extra == "dup500" and kind != "surface")) else c.extra


SINGLE_PARAMS = [(c, k) for c in SINGLE_CASES for k in _kinds(c.N, c.extra)]
COOP_PARAMS = [(c, k) for c in COOP_CASES for k in _kinds(c.N, c.extra)]
TAG_PARAMS = [(TAG_WRAP, k) for k in ("surface", "lattice")]


def _id(v):
    return "-".join(str(x) for x in v if x != "") if isinstance(v, tuple) else str(v)


def test_cases_reach_every_instance():
    """With 256 CUs the tables, through the dispatch model, name every code of the registry, W <= 16 and W > 16 of each cooperative PPT4, both placements
    (grid 8 W and W wide), both ends of every single-workgroup instance, and the sizes the cases were built for."""
    cus = REFERENCE_CUS
    codes = {("knn", 0), ("knn", 1)}
    for c in SINGLE_CASES:
        assert c.G <= c.N
        natural = fps_dispatch(c.B, c.N, cus, 1, 1)[0]
        assert c.forced == (natural >= 100), (c, "set_cooperative(0) exactly where the case would otherwise go cooperative")
        code, grid = fps_dispatch(c.B, c.N, cus, 0 if c.forced else 1, 1)
        assert (code, grid) == (c.inst, 0), c
        codes.add(("fps", code))
    for p in range(1, 9):
        sizes = {c.N for c in SINGLE_CASES if c.inst == p}
        assert {GROUP * (p - 1) + 1, GROUP * p - 3} <= sizes, p
        assert fps_groups(GROUP * (p - 1) + 1) == p == fps_groups(GROUP * p) and fps_groups(GROUP * p + 1) == p + 1
    assert any(c.inst == 8 and not c.forced and c.N == 28673 for c in SINGLE_CASES) and any(c.inst == 8 and not c.forced and c.N == 32768 for c in SINGLE_CASES)
    assert {(c.B, c.N, c.forced) for c in SINGLE_CASES if c.inst == 0} == {(1, 32769, True), (30, 33000, False), (1, (1 << 20) + 1, False)}
    seen = set()
    for c in COOP_CASES + [TAG_WRAP]:
        assert fps_coop_ppt4(c.B, c.N, cus) == (c.ppt4, c.W), c
        for prune in (0, 1):
            for mode in (1, 2):
                code, grid = fps_dispatch(c.B, c.N, cus, mode, prune)
                assert code == (200 if prune else 100) + c.ppt4 and grid in (c.W, 8 * c.W) and (mode == 1 or grid == c.W), c
                codes.add(("fps", code))
                seen.add((c.ppt4, c.W <= 16, grid // c.W))
    assert codes == {(i.family, i.code) for i in INSTANCES.values()}
    assert seen >= {(p, row, xs) for p in (1, 2, 4) for row in (True, False) for xs in (1,)} | {(p, True, 8) for p in (1, 2, 4)}
    assert {c.W for c in COOP_CASES} >= {8, 9, 17, 33, 64}
    assert fps_dispatch(1, 135165, cus, 1, 0) == (101, 33) and fps_dispatch(1, 69629, cus, 1, 0) == (101, 17 * 8)      # xs = 1 reached without the test hook
    assert fps_dispatch(9, 33000, cus, 1, 1) == (201, 72)
    assert (1 << 20) - 1 == 0xFFFFF and fps_coop_ppt4(1, (1 << 20) + 1, cus) == (0, 0)
    assert TAG_WRAP.G > 4097 and fps_dispatch(TAG_WRAP.B, TAG_WRAP.N, cus, 1, 1) == (201, 64)
    # the bounds of the issue: upload <= 12 MiB + one point, oracle work <= about 1.4e8 distance evaluations per case
    for c, k in SINGLE_PARAMS + COOP_PARAMS + TAG_PARAMS:
        assert c.B * c.N * 12 <= 12 * (1 << 20) + 12 and c.B * c.N * fps_G(k, c.N, c.G) <= 1.4e8, (c, k)


def test_planted_clouds_are_sampled_at_every_planted_index():
    """O.fps of every planted cloud returns every far point (first and last index of every 4096-point group, N - 1) and prefers the original to its exact
    copy in a later group: a kernel that loses a group's edge, or takes the higher index of a tie, cannot equal the oracle on these clouds."""
    n = 0
    for c, k in SINGLE_PARAMS + COOP_PARAMS:
        if k != "planted":
            continue
        G = fps_G(k, c.N, c.G)
        far, orig, copy = planted_layout(c.N)
        assert G >= min(c.N, len(far) + 2)
        xyz, want, _ = fps_reference(k, c.B, c.N, G, _seed(c), "")
        for b in range(c.B):
            got = want[b].tolist()
            assert set(far) <= set(got), (c, b, sorted(set(far) - set(got)))
            if copy is not None:
                assert torch.equal(xyz[b, copy], xyz[b, orig])
                assert copy not in got or (G == c.N and got.index(orig) < got.index(copy)), (c, b)
        n += 1
    assert n >= 16 + 7


# ------------------------------------------------------------------------------------------------ 4. kNN cases
KnnCase = namedtuple("KnnCase", "name N K overflow tie")
KNN_N = (1, 3, 5, 255, 256, 257, 1021, 1024)
KNN_K = (1, 2, 255, 256, 257, 1023, 1024)
KNN_G = (1, 5)
KNN_GRID = [KnnCase("random", N, K, False, False) for N in KNN_N for K in sorted({k for k in KNN_K if k <= N} | {N})]


def _d2_bits(centre, cloud):
    """uint32 patterns of the fp32 squared distances in the oracle's order, (dx dx + dy dy) + dz dz, every operation rounded to fp32."""
    c, x = centre.numpy().astype(np.float32), cloud.numpy().astype(np.float32)
    dx, dy, dz = x[:, 0] - c[0], x[:, 1] - c[1], x[:, 2] - c[2]
    d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == np.float32
    return d2.view(np.uint32)


def knn_path(centre, cloud, K):
    """(band population, eq_total, need_eq) of the selection for one centre: the points that share the top 11 bits of the K-th smallest pattern, the points
    that equal it, and how many of those belong to the answer."""
    u = _d2_bits(centre, cloud)
    T = np.sort(u)[K - 1]
    return int((u >> MODEL["knn_top_shift"] == T >> MODEL["knn_top_shift"]).sum()), int((u == T).sum()), int(K - (u < T).sum())


def _shell(g, centre, n, copies=1):
    """n x copies points at radius 1.01 .. 1.10 around `centre`: squared distances in [1.02, 1.21], inside [1, 1.25), where the top 11 bits are equal."""
    v = torch.randn(n, 3, generator=g, dtype=torch.float64)
    pts = centre.double() + v / v.norm(dim=1, keepdim=True) * (1.01 + 0.09 * torch.rand(n, 1, generator=g, dtype=torch.float64))
    return pts.float().repeat_interleave(copies, 0)


@functools.lru_cache(maxsize=None)
def knn_inputs(name, N, G):
    """(centres [3, G, 3], clouds [3, N, 3]): three clouds, so with N % 4 != 0 clouds 1 and 2 start off 16-byte boundaries."""
    g = torch.Generator().manual_seed(1000 * N + G + len(name))
    B = 3
    if name == "random":
        return torch.rand(B, G, 3, generator=g) * 2 - 1, torch.rand(B, N, 3, generator=g) * 2 - 1
    if name in ("overflow", "overflow+tie"):
        assert G == 1 and N == 2305
        centres = torch.rand(B, 1, 3, generator=g) * 0.4 - 0.2
        clouds = torch.empty(B, N, 3)
        for b in range(B):
            pts = _shell(g, centres[b, 0], 2304) if name == "overflow" else _shell(g, centres[b, 0], 9, copies=256)
            pts = torch.cat([pts, centres[b] + torch.tensor([[3.0, 0.0, 0.0]])])
            clouds[b] = pts[torch.randperm(N, generator=g)]
        return centres, clouds
    if name == "tie":
        assert G == 2 and N == 729
        axis = torch.arange(-4, 5) / 4.0
        grid = torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3)
        clouds = torch.stack([grid[torch.randperm(N, generator=g)] for _ in range(B)])
        return torch.tensor([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0]]).expand(B, 2, 3).contiguous(), clouds
    assert name == "identical"
    return torch.tensor([0.5, 0.25, 0.25]).expand(B, G, 3).contiguous(), torch.full((B, N, 3), 0.25)


def _tied_K(name, N, G, start):
    """The first K >= start inside a tie class for every (centre, cloud) of the case."""
    centres, clouds = knn_inputs(name, N, G)
    for K in range(start, N):
        paths = [knn_path(centres[b, j], clouds[b], K) for b in range(centres.shape[0]) for j in range(G)]
        if all(eq != need for _, eq, need in paths):
            return K
    raise AssertionError((name, start))


KNN_SPECIAL = [
    (KnnCase("overflow", 2305, 10, True, False), 1), (KnnCase("overflow", 2305, 1024, True, False), 1),
    (KnnCase("tie", 729, _tied_K("tie", 729, 2, 3), False, True), 2), (KnnCase("tie", 729, _tied_K("tie", 729, 2, 300), False, True), 2),
    (KnnCase("overflow+tie", 2305, 10, True, True), 1), (KnnCase("overflow+tie", 2305, 1000, True, True), 1),
    (KnnCase("identical", 500, 37, False, True), 4), (KnnCase("identical", 2500, 37, True, True), 4), (KnnCase("identical", 5, 5, False, False), 1),
]
KNN_PARAMS = [(c, G) for c in KNN_GRID for G in KNN_G] + KNN_SPECIAL


def test_knn_preconditions_hold_for_every_case():
    """Every kNN case takes the inner path it was built for, for each of its (centre, cloud) pairs: the band holds <= KNN_CAND points or more, and the K-th
    value is tied (eq_total != need_eq: the cut by index) or not -- from the fp32 patterns numpy computes in the oracle's order."""
    paths = set()
    for c, G in KNN_PARAMS:
        assert 0 < c.K <= c.N and c.K <= MODEL["knn_maxk"], c
        centres, clouds = knn_inputs(c.name, c.N, G)
        assert clouds.shape == (3, c.N, 3) and centres.shape == (3, G, 3)
        for b in range(3):
            for j in range(G):
                band, eq, need = knn_path(centres[b, j], clouds[b], c.K)
                assert (band > MODEL["knn_cand"]) == c.overflow, (c, b, j, band)
                assert (eq != need) == c.tie and 1 <= need <= eq, (c, b, j, eq, need)
        paths.add((c.overflow, c.tie))
        if c.name == "random":
            assert not (clouds[:, None] == centres[:, :, None]).all(-1).any(), "centres are not points of the cloud"
    assert paths == {(False, False), (True, False), (False, True), (True, True)}
    grid = {(c.N, c.K) for c in KNN_GRID}
    assert {N for N, _ in grid} == set(KNN_N) and all((N, K) in grid for N in KNN_N for K in KNN_K + (N,) if K <= N)
    assert any(c.N % 4 for c, _ in KNN_PARAMS) and {1, MODEL["knn_maxk"], 255, 256, 257} <= {c.K for c, _ in KNN_PARAMS}
    assert sum(c.name == "tie" for c, _ in KNN_SPECIAL) == 2 and len({c.K for c, _ in KNN_SPECIAL if c.name == "tie"}) == 2


# ------------------------------------------------------------------------------------------------ GPU plumbing
@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    set_ = [e for e in TUNING_ENV if e in os.environ]
    assert not set_, f"{set_} set in the environment: the library reads them once and the dispatch model of this file would be wrong"
    from point_sam_amd import ops as _ops
    _ops._lib.load()
    return _ops


SENTINEL = -7.25      # what buffers hold where no kernel may write
SEEN = {}             # (family, code) -> the first case that confirmed it by a `last_instance` query after a launch


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _run_fps(ops, x, G, mode, prune):
    """One psam_fps under the two test hooks -> (indices, centres, (code, grid_x) as the queries report them)."""
    L = ops._lib.load()
    L.psam_fps_set_cooperative(mode)
    L.psam_fps_set_pruning(prune)
    try:
        idx, centres = ops.fps(x, G)
        ran = (L.psam_fps_last_instance(), L.psam_fps_last_grid_x())
    finally:
        L.psam_fps_set_cooperative(1)
        L.psam_fps_set_pruning(-1)
    return idx, centres, ran


def _fps_case(ops, c, kind, runs, what):
    """The four assertions of an FPS case for every (mode, prune) of `runs`: oracle bit for bit (indices and centres), the predicted instance and grid
    width, a second run with the same result; once per case the fp64 greedy-validity replay of what was returned."""
    G = fps_G(kind, c.N, c.G)
    xyz, want, want_c = fps_reference(kind, c.B, c.N, G, _seed(c), _extra(c, kind))
    x = xyz.cuda()
    codes = set()
    for mode, prune in runs:
        tag = f"{what} {kind} B={c.B} N={c.N} G={G} set_cooperative({mode}) set_pruning({prune})"
        idx, centres, ran = _run_fps(ops, x, G, mode, prune)
        predicted = fps_dispatch(c.B, c.N, _cus(), mode, prune)
        assert ran == predicted, f"{tag}: the library ran (code, grid_x) = {ran}, the model says {predicted}"
        got = idx.cpu()
        if not torch.equal(got, want):
            first = (got != want).nonzero()[0].tolist()
            raise AssertionError(f"{tag} (instance {ran[0]}): {(got != want).sum().item()} of {got.numel()} indices differ from the oracle, first at {first}: "
                                 f"got {got[tuple(first)]} want {want[tuple(first)]}")
        assert torch.equal(centres.cpu(), want_c), f"{tag}: centres differ from the points at the indices"
        idx2, centres2, ran2 = _run_fps(ops, x, G, mode, prune)
        assert ran2 == ran and torch.equal(idx2, idx) and torch.equal(centres2, centres), f"{tag}: a second run differs"
        SEEN.setdefault(("fps", ran[0]), tag)
        codes.add(ran[0])
    worst = min(greedy_replay(xyz[b], want[b]) for b in range(c.B))
    print(f"| {what} {kind} B={c.B} N={c.N} G={G} | instances {sorted(codes)} | fp64 replay: smallest md[chosen] / max md = 1 - {1 - worst:.2e} |")
    return codes


@gpu
@pytest.mark.parametrize("c,kind", SINGLE_PARAMS, ids=_id)
def test_fps_single_workgroup_instances(ops, c, kind):
    """fps_kernel<1 .. 8> at the first and the last N of each (N = 4096 (p - 1) + 1: the last group holds one point; 4096 p - 3: the last float4 of the last
    thread is ragged), N = 1, N = 3, G = N, duplicates, and fps_kernel<0> (forced, by 30 clouds, by N > 2^20)."""
    codes = _fps_case(ops, c, kind, [(0 if c.forced else 1, 1)], f"fps_kernel<{c.inst}>")
    assert codes == {c.inst}, (codes, "on this device the case did not run as the instance it is listed for")


@gpu
@pytest.mark.parametrize("c,kind", COOP_PARAMS, ids=_id)
def test_fps_cooperative_instances(ops, c, kind):
    """fps_coop_kernel<PPT4> and fps_coop_pruned_kernel<PPT4> (pruning off / on), with the one-XCD placement where the model grants it and without."""
    codes = _fps_case(ops, c, kind, [(mode, prune) for prune in (0, 1) for mode in (1, 2)], f"cooperative <{c.ppt4}> W={c.W}")
    if _cus() == REFERENCE_CUS:
        assert codes == {100 + c.ppt4, 200 + c.ppt4}, codes


@gpu
@pytest.mark.parametrize("c,kind", TAG_PARAMS, ids=_id)
def test_fps_cooperative_tag_wrap(ops, c, kind):
    """G = 4200: iteration 4095 carries tag 0xFFF, the value the slots are reset to, and iteration 4096 tag 0 again."""
    codes = _fps_case(ops, c, kind, [(1, 0), (1, 1)], "tag wrap")
    if _cus() == REFERENCE_CUS:
        assert codes == {101, 201}, codes


# ------------------------------------------------------------------------------------------------ kNN
def _knn_partition(centres, clouds, idx, what):
    """The fp64 partition check: K distinct indices per centre; max d64(returned) <= min d64(not returned) (1 + 2^-20); ascending within the same slack."""
    slack = 1 + 2.0 ** -20
    B, G, K = idx.shape
    N = clouds.shape[1]
    for b in range(B):
        d = (clouds[b].double()[None] - centres[b].double()[:, None]).square().sum(-1)      # [G, N]
        for j in range(G):
            ids = idx[b, j]
            assert ids.min() >= 0 and ids.max() < N and ids.unique().numel() == K, f"{what}: cloud {b} centre {j}: indices not distinct or out of range"
            dr = d[j, ids]
            rest = torch.ones(N, dtype=torch.bool)
            rest[ids] = False
            if rest.any():
                assert dr.max() <= d[j, rest].min() * slack, f"{what}: cloud {b} centre {j}: a nearer point was left out"
            assert (dr[:-1] <= dr[1:] * slack).all(), f"{what}: cloud {b} centre {j}: not ascending"


@gpu
@pytest.mark.parametrize("c,G", KNN_PARAMS, ids=_id)
def test_knn_instances(ops, c, G):
    """knn_kernel and knn_band_kernel on one case, each confirmed by psam_knn_last_instance: the oracle's indices bit for bit, each other's, and the fp64
    partition check.  The CPU test above proves which inner path of the kernels the case takes."""
    L = ops._lib.load()
    centres, clouds = knn_inputs(c.name, c.N, G)
    _, want = O.knn(centres, clouds, c.K, "exact")
    what = f"kNN {c.name} N={c.N} K={c.K} G={G}"
    cd, xd = centres.cuda(), clouds.cuda()
    out = {}
    try:
        for mode in (0, 1):
            L.psam_knn_force_band(mode)
            out[mode] = ops.knn(cd, xd, c.K)
            assert L.psam_knn_last_instance() == mode, (what, mode, L.psam_knn_last_instance())
            SEEN.setdefault(("knn", mode), what)
    finally:
        L.psam_knn_force_band(-1)
    for mode in (0, 1):
        got = out[mode].cpu()
        if not torch.equal(got, want):
            rows = (got != want).any(-1).nonzero()
            raise AssertionError(f"{what} {'knn_band_kernel' if mode else 'knn_kernel'}: {len(rows)} of {3 * G} groups differ from the oracle; first {rows[0].tolist()}: "
                                 f"got {got[tuple(rows[0])][:8]} want {want[tuple(rows[0])][:8]}")
    assert torch.equal(out[0], out[1]), what
    _knn_partition(centres, clouds, out[1].cpu(), what)
    if c.name == "identical":
        assert torch.equal(out[1].cpu(), torch.arange(c.K).expand(3, G, c.K)), what + ": every distance equal -> the K lowest indices"


# ------------------------------------------------------------------------------------------------ 3-NN
# (name, B, N, G): "dup": centre 4 is a copy of centre 1, centre 7 of centre 2, and point 5 of cloud 0 lies on centres 1 and 4; G > 5461: more than 64 KiB of dynamic LDS
THREE_NN_CASES = [("random", 3, N, 3) for N in (1, 255, 256, 257)] + [("dup", 2, 257, 8), ("random", 2, 300, 5461), ("random", 2, 300, 5462), ("dup", 2, 300, 12288)]
THREE_NN_EPS = 1e-8


@functools.lru_cache(maxsize=None)
def three_nn_inputs(name, B, N, G):
    g = torch.Generator().manual_seed(N + 7 * G)
    xyz, centres = torch.rand(B, N, 3, generator=g) * 2 - 1, torch.rand(B, G, 3, generator=g) * 2 - 1
    if name == "dup":
        centres[:, 4] = centres[:, 1]
        centres[:, 7] = centres[:, 2]
        xyz[0, 5] = centres[0, 1]
    return xyz, centres


@gpu
@pytest.mark.parametrize("name,B,N,G", THREE_NN_CASES, ids=_id)
def test_three_nn_cases(ops, name, B, N, G):
    """three_nn_kernel: the oracle's indices exactly (equal distance keeps the lower centre index), weights within 1e-6 (the project's bound) of an fp64
    evaluation at those indices and summing to 1 within 1e-6, guard rows untouched.  G = 5461 / 5462 / 12288 stage 65532 / 65544 / 147456 bytes of
    centres in dynamic LDS: just under 64 KiB, just over it, and the limit the host admits."""
    L = ops._lib.load()
    xyz, centres = three_nn_inputs(name, B, N, G)
    want_i, _ = O.interp_weights(xyz, centres, "exact", eps=THREE_NN_EPS)
    xd, cd = xyz.cuda(), centres.cuda()
    rows = B * N
    idx = torch.full((rows + 2, 3), -77, dtype=torch.int64, device="cuda")
    w = torch.full((rows + 2, 3), SENTINEL, device="cuda")
    what = f"3-NN {name} B={B} N={N} G={G} ({G * 12} bytes of LDS)"
    rc = L.psam_three_nn(xd.data_ptr(), cd.data_ptr(), B, N, G, THREE_NN_EPS, idx.data_ptr(), w.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, f"{what}: refused with status {rc}: {L.psam_last_error_string().decode()}"
    torch.cuda.synchronize()
    print(f"| {what} | launched |")
    assert (idx[rows:] == -77).all() and (w[rows:] == SENTINEL).all(), what + ": guard rows written"
    got_i, got_w = idx[:rows].view(B, N, 3).cpu(), w[:rows].view(B, N, 3).cpu().double()
    assert torch.equal(got_i, want_i), f"{what}: {(got_i != want_i).sum().item()} index mismatches"
    d2 = (xyz.double()[:, :, None] - O.batch_index_select(centres, want_i.reshape(B, -1)).view(B, N, 3, 3).double()).square().sum(-1)
    v = 1.0 / d2.clamp(min=float(np.float32(THREE_NN_EPS)))
    ref = v / v.sum(-1, keepdim=True)
    err = (got_w - ref).abs().max().item()
    print(f"| {what} | max |w - fp64| {err:.2e} | max |sum w - 1| {(got_w.sum(-1) - 1).abs().max().item():.2e} |")
    assert err <= 1e-6, f"{what}: weights differ from fp64 by {err:.3e}"
    assert ((got_w.sum(-1) - 1).abs() <= 1e-6).all(), what
    if name == "dup":
        for k in range(3):      # a copy (4, 7) only ever after the lower-indexed centre of the same place (1, 2)
            assert not ((got_i[..., k] == 4) & ~(got_i[..., :k] == 1).any(-1)).any() and not ((got_i[..., k] == 7) & ~(got_i[..., :k] == 2).any(-1)).any(), what
        assert got_i[0, 5].tolist()[:2] == [1, 4] and got_w[0, 5, 0] == got_w[0, 5, 1] and got_w[0, 5, 0] > 0.49, (what, "the point on two coincident centres: both clamp to eps")


# ------------------------------------------------------------------------------------------------ border farthest
def _border_regions(name, N):
    """(xyz [1, N, 3], regions [Z, N] bool)."""
    g = torch.Generator().manual_seed(N)
    if name == "equal":
        # background 0 at the origin and 1 at (10, 0, 0), the rest far away on the y axis; members on the x axis: 10 at distance 1 from background 0 and 500
        # (another 256-block) at distance 1 from background 1, every other member nearer to background 0: two maxima, the lower index wins
        assert N == 600
        xyz = torch.zeros(1, N, 3)
        xyz[0, :, 1] = 50.0 + torch.arange(N)
        region = torch.zeros(1, N, dtype=torch.bool)
        members = torch.tensor(sorted(set(range(2, N, 7)) | {10, 500}))
        region[0, members] = True
        xyz[0, members] = torch.stack([torch.rand(len(members), generator=g) * 0.875, torch.zeros(len(members)), torch.zeros(len(members))], 1)
        xyz[0, 0] = torch.tensor([0.0, 0.0, 0.0]); xyz[0, 1] = torch.tensor([10.0, 0.0, 0.0])
        xyz[0, 10] = torch.tensor([1.0, 0.0, 0.0]); xyz[0, 500] = torch.tensor([9.0, 0.0, 0.0])
        return xyz, region
    xyz = O.synthetic_batch(1, N, seed=N)[0] if N > 1 else torch.full((1, 1, 3), 0.375)      # (a cloud of one point normalises to 0 / 0)
    one = torch.zeros(N, dtype=torch.bool)
    one[N // 2] = True
    return xyz, torch.stack([xyz[0, :, 0] > 0.1, one, ~one, torch.zeros(N, dtype=torch.bool), torch.ones(N, dtype=torch.bool)])


@gpu
@pytest.mark.parametrize("name,N", [("random", 1), ("random", 255), ("random", 256), ("random", 257), ("equal", 600)], ids=_id)
def test_border_farthest_edges(ops, name, N):
    """One block, one block exactly, one point more; a region of one member, of everything but one point, empty and full; two members at equal
    nearest-background distance in different 256-blocks.  (index, distance) equal O.border_farthest exactly."""
    xyz, regions = _border_regions(name, N)
    idx, dist = ops.border_farthest(xyz.cuda(), regions.cuda())
    for z in range(regions.shape[0]):
        wi, wd = O.border_farthest(xyz[0], regions[z])
        assert int(idx[z]) == wi and float(dist[z]) == wd, (name, N, z, int(idx[z]), wi, float(dist[z]), wd)
    if name == "equal":
        assert int(idx[0]) == 10 and float(dist[0]) == 1.0


@gpu
def test_every_registry_instance_was_confirmed(ops):
    """Runs last: the GPU tests above confirmed, by `last_instance`, every code of the registry at least once."""
    want = {(i.family, i.code) for i in INSTANCES.values()}
    print()
    for key in sorted(SEEN):
        print(f"| {key[0]} {key[1]} | {SEEN[key]} |")
    assert set(SEEN) == want, f"never confirmed: {sorted(want - set(SEEN))}; not in the registry: {sorted(set(SEEN) - want)}"
