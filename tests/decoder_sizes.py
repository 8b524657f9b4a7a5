"""The sizes at which the decoder's small-row kernels take another trip of a loop or another branch, read from the sources: the second half of
csrc/gemm.hip (linear_skinny, linear_skinny_multi, linear_rows_multi<FULL>, linear_skinny_ln, linear_ln256: rounds of 16 * SK_CH k, the K ranges of
skinny_ln_ksplit, the `K % 128` dispatch of the two rows_multi instances, the K <= 512 of linear_ln256) and the end of csrc/rowops.hip (mlp3 / mlp3_pair:
chunks of 256 input columns, blocks of MLP3_OB * MLP3_NW outputs, MLP3_MAXD).
The literal lists below are what tests/test_gpu_decoder_rows.py runs; tests/test_decoder_rows_cpu.py derives the same lists from the parsed constants,
so a changed constant without a matching size fails without a GPU."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "point_sam_amd", "csrc")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pointsam_hip.h")

K_SIZES = (16, 112, 128, 144, 272)                                   # linear_skinny, linear_skinny_multi, linear_rows_multi
LN_K_SIZES = K_SIZES + (528, 2048, 2064, 4096)                       # linear_skinny_ln (256 + 16 = 272 is in K_SIZES already)
LN256_K_SIZES = (16, 112, 128, 144, 272, 512)                        # linear_ln256
MLP3_IN_SIZES = (4, 252, 256, 260, 516, 1024)                        # din and dh of mlp3
MLP3_OUT_SIZES = (1, 15, 16, 17, 255, 257, 300)                      # dout of mlp3
MLP3_TALL = 300                                                      # a dout past one block of outputs that is no multiple of MLP3_OB


def _read(name, csrc=None):
    return open(os.path.join(csrc or CSRC, name)).read()


def _constants(src, names):
    """`constexpr int A = 1, B = 2;` declarations -> {name: value}; every name exactly once."""
    found = {}
    for decl in re.findall(r"constexpr\s+int\s+([^;]+);", src):
        for n, v in re.findall(r"(\w+)\s*=\s*(\d+)", decl):
            if n in names:
                assert n not in found, n
                found[n] = int(v)
    assert set(found) == set(names), (names, found)
    return found


def constants(csrc=None):
    """-> dict: SK_CH, R (k per load round), LN_RANGE and LN_CAP (k per K range and most ranges of skinny_ln_ksplit), FULL_MASK (rows_multi runs <true> when
    K & FULL_MASK == 0), LN256_MAX_K, MLP3_MAXD / MLP3_OB / MLP3_NW, MLP3_CHUNK (input columns per trip of the kc loop), OBW, MAX_JOBS."""
    g, r = _read("gemm.hip", csrc), _read("rowops.hip", csrc)
    c = _constants(g, ("SK_CH",))
    c["R"] = 16 * c["SK_CH"]
    assert g.count("kc += 16 * SK_CH") == 5, "one round of 16 * SK_CH k in each of the five kernels"
    m = re.search(r"static int skinny_ln_ksplit\(int K\) \{ const int s = \(K \+ (\d+)\) / (\d+); return s < 1 \? 1 : \(s > (\d+) \? (\d+) : s\); \}", g)
    assert m, "skinny_ln_ksplit: a body this parser does not understand"
    a, b, cap, cap2 = map(int, m.groups())
    assert a == b - 1 and cap == cap2
    c["LN_RANGE"], c["LN_CAP"] = b, cap
    assert "const int kper = ((K + ksplit - 1) / ksplit + 15) & ~15;" in g and "dim3(N / 16, ksplit)" in g      # ln_split() below
    host = g[g.index("PSAM_API int32_t psam_linear_rows_multi("):]
    host = host[:host.index("\n}\n")]
    m = re.findall(r"if \(\(K & (\d+)\) == 0\) hipLaunchKernelGGL\(linear_rows_multi_kernel<true>,[^\n]*\n\s*else hipLaunchKernelGGL\(linear_rows_multi_kernel<false>,", host)
    assert len(m) == 1 and host.count("linear_rows_multi_kernel<") == 2, "the dispatch of psam_linear_rows_multi"
    c["FULL_MASK"] = int(m[0])
    host = g[g.index("PSAM_API int32_t psam_linear_ln256("):]
    m = re.findall(r"K > 0 && K <= (\d+) && \(K & 15\) == 0", host[:host.index("\n}\n")])
    assert len(m) == 1
    c["LN256_MAX_K"] = int(m[0])
    c.update(_constants(r, ("MLP3_MAXD", "MLP3_OB", "MLP3_NW")))
    m = re.findall(r"for \(int kc = 0; kc < ni; kc \+= (\d+)\) \{\s*const int k = kc \+ 4 \* lane,", r)
    assert len(m) == 1
    c["MLP3_CHUNK"] = int(m[0])
    assert c["MLP3_CHUNK"] == 4 * 64      # a float4 per lane
    assert "ob += MLP3_NW * MLP3_OB" in r
    c["OBW"] = c["MLP3_OB"] * c["MLP3_NW"]
    m = re.findall(r"#define PSAM_SKINNY_MAX_JOBS (\d+)", open(HEADER).read())
    assert len(m) == 1
    c["MAX_JOBS"] = int(m[0])
    return c


def k_sizes(c):
    """One slot; a round one slot short; one full round; a ragged round after a full one; a ragged round after two."""
    R = c["R"]
    return (16, R - 16, R, R + 16, 2 * R + 16)


def ln_k_sizes(c):
    """k_sizes and: two and three K ranges with a rounded kper and a shorter last range; the first K with LN_CAP ranges; the first K at the cap with a
    rounded kper; four rounds per range."""
    P, cap = c["LN_RANGE"], c["LN_CAP"]
    return tuple(sorted(set(k_sizes(c)) | {P + 16, 2 * P + 16, cap * P, cap * P + 16, cap * 4 * c["R"]}))


def ln256_k_sizes(c):
    return tuple(sorted(set(k_sizes(c)) | {c["LN256_MAX_K"]}))


def ln_split(c, K):
    """(ksplit, kper) of psam_linear_skinny_ln for K."""
    s = (K + c["LN_RANGE"] - 1) // c["LN_RANGE"]
    ksplit = 1 if s < 1 else min(s, c["LN_CAP"])
    return ksplit, ((K + ksplit - 1) // ksplit + 15) & ~15


def ln_ranges(c, K):
    """The [k0, k1) of every workgroup row of linear_skinny_ln_kernel's grid."""
    ksplit, kper = ln_split(c, K)
    return [(y * kper, min(y * kper + kper, K)) for y in range(ksplit)]


def rows_multi_full(c, K):
    """Whether psam_linear_rows_multi launches linear_rows_multi_kernel<true> for K."""
    return K & c["FULL_MASK"] == 0


def mlp3_in_sizes(c):
    """din, dh: one float4; a chunk one float4 short; one chunk; a second chunk of one float4 (kw clamped on 63 lanes); a third; the most."""
    C = c["MLP3_CHUNK"]
    return (4, C - 4, C, C + 4, 2 * C + 4, c["MLP3_MAXD"])


def mlp3_out_sizes(c):
    """dout: one row (every other load clamped to it); both sides of a wave's MLP3_OB rows; both sides of one trip of the ob loop; a second trip that ends
    inside a wave's rows."""
    OB, OBW = c["MLP3_OB"], c["OBW"]
    return (1, OB - 1, OB, OB + 1, OBW - 1, OBW + 1, MLP3_TALL)
