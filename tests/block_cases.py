"""The shape-dependent decisions of the five coarse entries of csrc/blocks.hip (psam_eva_block, psam_eva_gelu_block, psam_patch_encoder,
psam_upscale_masks, psam_twoway_decoder) mirrored in plain Python, the thresholds behind them read from the sources (constants(), as
tests/decoder_sizes.py does), and the literal case lists tests/test_gpu_blocks.py runs, one list per entry.  Every case names the routes it is meant to
take (`want`); tests/test_blocks_cpu.py keeps the names equal to the mirrors and the mirrors equal to the sources, so a changed literal in blocks.hip or
in psam_attention_small without a changed case fails without a GPU."""
import os
import re
from collections import namedtuple

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "point_sam_amd", "csrc")

# What constants() must find in the sources; the case lists below were written against these values.
THRESHOLDS = dict(
    PACKED_MIN_M=256,        # host_linear: M >= 256 rows and a packed weight -> the packed-operand GEMM; key_fast / fast: I >= 256; tokens: R >= 256
    SKINNY_MAX_M=64,         # host_linear: M <= 64 -> psam_linear_skinny; tok_fast: R <= 64
    ROWS_MULTI_MAX=2048,     # rows_multi_fits: rows of ONE cloud <= 2048 -> the exact-fp32 row kernel; small_rows
    K_MASK=15,               # rows_multi_fits, the skinny route, tok_fast and fast: (K & 15) == 0
    PACKED_MIN_NK=128,       # psam_twoway_decoder packs a weight when N >= 128 && K >= 128
    FAST_E=256, FAST_IX_MIN=128, FAST_IX_MAX=512,      # the terms of `fast`
    ROW_LN_H1=512, ROW_LN_ROWS=128,                    # psam_patch_encoder: h1 == 512 && rows % 128 == 0 (&& the library has the 128x512 tile)
    PART_ROWS=64,            # psam_patch_encoder: Kp = K <= 64 ? K : 64
    EVA_M_TILE=256, GELU_MIN_M=256, GELU_FUSED_M=256, GELU_FUSED_H=128,
    DIM_MIN=256, DIM_MAX=4096, EVA_DIM_TILE=128, MIN_HIDDEN=128,
    TW_MAX_KEYS=8192,        # psam_twoway_decoder's own limit on T and G ...
    ATTN_LDS_BYTES=128 * 1024, ATTN_BYTES_PER_KEY=16,      # ... which is psam_attention_small's Lk * 16 <= 128 KiB
    FEWKEYS_MAX_LK=16, FEWKEYS_MIN_LQ=64, SPLIT_MIN_LK=128, SPLIT_MAX_WAVES=2048, SPLIT_MAX_HD=64,
    UPSCALE_DIM=256, UPSCALE_MAX_C=4, UPSCALE_N_TILE=32, UPSCALE_ROWS=256, PATCH_ROWS=256, PATCH_H0=128, PATCH_H1_MIN=256, PATCH_H1_MAX=4096, PATCH_STEP=128,
)
T = THRESHOLDS


def _one(pattern, src, what):
    m = re.findall(pattern, src)
    assert len(m) == 1, f"{what}: {len(m)} matches of {pattern!r}"
    return m[0]


def constants(csrc=None):
    """THRESHOLDS as the sources have them: every literal is found by the statement it stands in, exactly once."""
    b = open(os.path.join(csrc or CSRC, "blocks.hip")).read()
    r = open(os.path.join(csrc or CSRC, "rowops.hip")).read()
    i = lambda *a: int(_one(*a))
    c = {}
    rows, mask = _one(r"return k_rows_multi\.get\(\) != 0 && rows_per_cloud <= (\d+) && \(K & (\d+)\) == 0;", b, "rows_multi_fits")
    c["ROWS_MULTI_MAX"] = int(rows)
    c["PACKED_MIN_M"] = i(r"if \(M >= (\d+) && l\.packed\) \{", b, "host_linear, packed")
    sk, mask2 = _one(r"if \(M <= (\d+) && \(l\.K & (\d+)\) == 0\) return psam_linear_skinny\(", b, "host_linear, skinny")
    tf, mask3 = _one(r"const bool tok_fast = R <= (\d+) && \(E & (\d+)\) == 0;", b, "tok_fast")
    assert sk == tf, "tok_fast and the skinny route share their row limit"
    c["SKINNY_MAX_M"] = int(sk)
    nmin, kmin = _one(r"if \(l\.N >= (\d+) && l\.K >= (\d+)\) \{ l\.packed = ", b, "packed weights of the two-way decoder")
    assert nmin == kmin
    c["PACKED_MIN_NK"] = int(nmin)
    fast = _one(r"const bool fast = tok_fast && !sd && tw_fast != 0 && E == (\d+) && IX >= (\d+) && 2 \* IX <= E && IX <= (\d+) && I >= (\d+) && \(mlp & (\d+)\) == 0 && "
                r"\(IX & (\d+)\) == 0 &&\s+plan->o_cat_packed\[0\] != 0 && counters != nullptr;", b, "fast")
    c["FAST_E"], c["FAST_IX_MIN"], c["FAST_IX_MAX"] = int(fast[0]), int(fast[1]), int(fast[2])
    assert {mask, mask2, mask3, fast[4], fast[5]} == {mask}, "one K mask"
    c["K_MASK"] = int(mask)
    kf = re.findall(r"I >= (\d+) && (?:ck\.packed && jq\.packed && cvl\.packed|fk\.packed && fv\.packed|fk\.packed\))", b)
    assert len(kf) == 3 and set(kf) == {fast[3], str(c["PACKED_MIN_M"])}, "key_fast, the fork and the final attention share host_linear's row limit"
    assert "const bool small_rows = tw_fast >= 2 && rows_multi_fits(G, E);" in b
    h1, rr = _one(r"if \(h1 == (\d+) && rows % (\d+) == 0 && psam_gemm_f16x3p_fused_row_ln\(h1\)\) \{", b, "fused conv2.0")
    c["ROW_LN_H1"], c["ROW_LN_ROWS"] = int(h1), int(rr)
    a, a2 = _one(r"const int Kp = K <= (\d+) \? K : (\d+), parts = K / Kp;", b, "Kp")
    assert a == a2
    c["PART_ROWS"] = int(a)
    pk, pr = _one(r"\(K == 32 \|\| \(K > 0 && K % (\d+) == 0\)\) && rows % (\d+) == 0 && rows <", b, "psam_patch_encoder shapes")
    assert pk == a
    c["PATCH_ROWS"] = int(pr)
    p = _one(r"h0 == (\d+) && h1 >= (\d+) && h1 % (\d+) == 0 && h1 <= (\d+) && cout >= (\d+) && cout % (\d+) == 0 && cin >= 4", b, "psam_patch_encoder_prepare")
    assert p[2] == p[4] == p[5]
    c["PATCH_H0"], c["PATCH_H1_MIN"], c["PATCH_STEP"], c["PATCH_H1_MAX"] = int(p[0]), int(p[1]), int(p[2]), int(p[3])
    c["EVA_M_TILE"] = i(r"B > 0 && L > 0 && M % (\d+) == 0 && M < \(\(int64_t\)1 << 31\), PSAM_EINVAL, \"psam_eva_block:", b, "psam_eva_block rows")
    c["GELU_MIN_M"] = i(r"B > 0 && L > 0 && M >= (\d+) && M < \(\(int64_t\)1 << 31\), PSAM_EINVAL, \"psam_eva_gelu_block:", b, "psam_eva_gelu_block rows")
    fm, fh = _one(r"const bool fused_gelu = \(M % (\d+) == 0\) && \(H % (\d+) == 0\) && psam_gemm_f16x3p_splitk\(\(int32_t\)M, H, Dp, PSAM_ACT_GELU\) == 1;", b, "fused_gelu")
    c["GELU_FUSED_M"], c["GELU_FUSED_H"] = int(fm), int(fh)
    lo, hi, tile = _one(r"PSAM_REQUIRE\(D >= (\d+) && D <= (\d+) && D % (\d+) == 0, PSAM_EINVAL, WHO \": need 256 <= dim", b, "psam_eva_block_prepare dim")
    glo, ghi, gh = _one(r"PSAM_REQUIRE\(D >= (\d+) && D <= (\d+) && D % 32 == 0 && H >= (\d+) && H % 32 == 0 && heads > 0", b, "psam_eva_gelu_block_prepare dim")
    hp = i(r"PSAM_REQUIRE\(Hp % 64 == 0 && Hp >= (\d+), PSAM_EINVAL,", b, "psam_eva_block_prepare hidden")
    assert (lo, hi) == (glo, ghi) and int(gh) == hp
    c["DIM_MIN"], c["DIM_MAX"], c["EVA_DIM_TILE"], c["MIN_HIDDEN"] = int(lo), int(hi), int(tile), hp
    tk, gk = _one(r"PSAM_REQUIRE\(T <= (\d+) && G <= (\d+), PSAM_EINVAL, \"psam_twoway_decoder:", b, "psam_twoway_decoder keys")
    assert tk == gk
    c["TW_MAX_KEYS"] = int(tk)
    per, kib = _one(r"PSAM_REQUIRE\(\(size_t\)Lk \* (\d+) <= (\d+) \* 1024, PSAM_EINVAL, \"psam_attention_small: Lk too large\"\);", r, "psam_attention_small Lk")
    c["ATTN_BYTES_PER_KEY"], c["ATTN_LDS_BYTES"] = int(per), int(kib) * 1024
    assert _one(r"attention_small_kernel, dim3\(\(unsigned\)psam_cdiv\(waves, 4\)\), dim3\(256\), \(size_t\)Lk \* (\d+), stream", r, "LDS of attention_small_kernel") == per
    fk = _one(r"if \(Lk <= (\d+) && Lq >= (\d+) && aligned && \(hd == 16 \|\| hd == 32\) && Z <= 65535 && H <= 65535\) \{", r, "few-keys kernel")
    c["FEWKEYS_MAX_LK"], c["FEWKEYS_MIN_LQ"] = int(fk[0]), int(fk[1])
    sp = _one(r"if \(k_attn_small_split\.get\(\) && Lk >= (\d+) && waves <= (\d+) && aligned && \(hd & 3\) == 0 && hd <= (\d+) && \(64 % \(hd >> 2\)\) == 0\) \{", r, "split kernel")
    c["SPLIT_MIN_LK"], c["SPLIT_MAX_WAVES"], c["SPLIT_MAX_HD"] = int(sp[0]), int(sp[1]), int(sp[2])
    c["UPSCALE_DIM"] = i(r"PSAM_REQUIRE\(wt->dim == (\d+), PSAM_EINVAL, WHO \": transformer_dim must be", b, "psam_upscale_masks_prepare")
    u = _one(r"C > 0 && C <= (\d+) && \(Z \* N\) % (\d+) == 0 && N % (\d+) == 0 && Z \* N <", b, "psam_upscale_masks shapes")
    c["UPSCALE_MAX_C"], c["UPSCALE_ROWS"], c["UPSCALE_N_TILE"] = int(u[0]), int(u[1]), int(u[2])
    return c


def kpad32(k):
    return (k + 31) // 32 * 32


# ------------------------------------------------------------------------------------------------ the decisions
def host_linear_route(M, cloud_rows, act, K, packed):
    """host_linear of blocks.hip: the kernel one nn.Linear runs on."""
    if cloud_rows > 0 and act == 0 and cloud_rows <= T["ROWS_MULTI_MAX"] and (K & T["K_MASK"]) == 0:
        return "rows_multi"
    if M >= T["PACKED_MIN_M"] and packed:
        return "packed"
    if M <= T["SKINNY_MAX_M"] and (K & T["K_MASK"]) == 0:
        return "skinny"
    return "linear"


def eva_gelu_fused(M, H, splitk):
    """psam_eva_gelu_block: fc1 hands GELU(.) to fc2 packed (True) or fc1 -> psam_scale_pack_rows_g8 -> fc2 (False).  splitk: the library's
    psam_gemm_f16x3p_splitk(M, H, dim, GELU), 1 for every K < 1024."""
    return M % T["GELU_FUSED_M"] == 0 and H % T["GELU_FUSED_H"] == 0 and splitk == 1


def patch_route(h1, rows, K, fused_row_ln=False):
    """psam_patch_encoder -> (row_ln_fused, Kp, parts).  fused_row_ln: psam_gemm_f16x3p_fused_row_ln(h1), which is 0 for every h1 != 256 in the default
    build (the 128x512 tile is an experiments-build configuration), so the default build always runs conv2.0 and the packed LayerNorm as two launches."""
    Kp = K if K <= T["PART_ROWS"] else T["PART_ROWS"]
    return (h1 == T["ROW_LN_H1"] and rows % T["ROW_LN_ROWS"] == 0 and bool(fused_row_ln)), Kp, K // Kp


def attention_small_instance(Z, H, Lq, Lk, hd):
    """psam_attention_small on aligned operands -> what psam_attention_small_last_instance reports: 4 / 8 the few-keys kernels, 1 the split kernel, 0 one
    wave per query, "refused" past the key limit."""
    if Lk * T["ATTN_BYTES_PER_KEY"] > T["ATTN_LDS_BYTES"]:
        return "refused"
    if Lk <= T["FEWKEYS_MAX_LK"] and Lq >= T["FEWKEYS_MIN_LQ"] and hd in (16, 32):
        return 4 if hd == 16 else 8
    if Lk >= T["SPLIT_MIN_LK"] and Z * H * Lq <= T["SPLIT_MAX_WAVES"] and hd % 4 == 0 and hd <= T["SPLIT_MAX_HD"] and 64 % (hd >> 2) == 0:
        return 1
    return 0


def twoway_route(Z, Tk, G, E, downsample, mlp, counters, tw_fast, heads=8):
    """psam_twoway_decoder (default build: no fork) -> dict: tok_fast, fast, small_rows, key_fast (the same in every layer: the packed weights depend on
    the dimensions only), token_linear (the route of a Linear on the R token rows in the operator sequence), and the psam_attention_small instance of
    each attention of a layer -- self (tokens), t2i (tokens -> patches), i2t (patches -> tokens) -- and of the final one, which is launched last."""
    R, I, IX = Z * Tk, Z * G, E // downsample
    packed = lambda N, K: N >= T["PACKED_MIN_NK"] and K >= T["PACKED_MIN_NK"]
    tok_fast = R <= T["SKINNY_MAX_M"] and (E & T["K_MASK"]) == 0
    fast = (tok_fast and tw_fast != 0 and E == T["FAST_E"] and IX >= T["FAST_IX_MIN"] and 2 * IX <= E and IX <= T["FAST_IX_MAX"] and I >= T["PACKED_MIN_M"]
            and (mlp & T["K_MASK"]) == 0 and (IX & T["K_MASK"]) == 0 and bool(counters))
    small_rows = fast and tw_fast >= 2 and G <= T["ROWS_MULTI_MAX"] and (E & T["K_MASK"]) == 0
    key_fast = I >= T["PACKED_MIN_M"] and packed(IX, E)
    inst = {"self": attention_small_instance(Z, heads, Tk, Tk, E // heads), "t2i": attention_small_instance(Z, heads, Tk, G, IX // heads),
            "i2t": attention_small_instance(Z, heads, G, Tk, IX // heads)}
    inst["final"] = inst["t2i"]
    return dict(tok_fast=tok_fast, fast=fast, small_rows=small_rows, key_fast=key_fast, token_linear=host_linear_route(R, 0, 0, E, packed(E, E)), attn=inst)


# ------------------------------------------------------------------------------------------------ the shape conditions of the entries
def eva_prepare_ok(dim, heads, hidden):
    hp = kpad32(hidden)
    return (dim > 0 and hidden > 0 and heads > 0 and dim % heads == 0 and dim // heads == 64 and T["DIM_MIN"] <= dim <= T["DIM_MAX"] and dim % T["EVA_DIM_TILE"] == 0
            and hp % 64 == 0 and hp >= T["MIN_HIDDEN"])


def eva_run_ok(B, L):
    return B > 0 and L > 0 and (B * L) % T["EVA_M_TILE"] == 0


def gelu_prepare_ok(dim, heads, hidden):
    if not (T["DIM_MIN"] <= dim <= T["DIM_MAX"] and dim % 32 == 0 and hidden >= T["MIN_HIDDEN"] and hidden % 32 == 0 and heads > 0 and dim % heads == 0):
        return False
    hd = dim // heads
    return hd == 64 or (64 < hd <= 128 and hd % 8 == 0)


def gelu_run_ok(B, L):
    return B > 0 and L > 0 and B * L >= T["GELU_MIN_M"]


def patch_prepare_ok(h0, h1, cout, cin=4):
    return (h0 == T["PATCH_H0"] and T["PATCH_H1_MIN"] <= h1 <= T["PATCH_H1_MAX"] and h1 % T["PATCH_STEP"] == 0 and cout >= T["PATCH_STEP"] and cout % T["PATCH_STEP"] == 0
            and cin >= 4)


def patch_run_ok(B, rep, G, K, C, centralize, cin, h0=128, h1=512, cout=512):
    rows, groups = B * rep * G * K, B * rep * G
    if not (B > 0 and rep > 0 and G > 0 and (K == 32 or (K > 0 and K % T["PART_ROWS"] == 0)) and rows % T["PATCH_ROWS"] == 0):
        return False
    if cin != 3 + C * (2 if centralize else 1):
        return False
    parts = patch_route(h1, rows, K)[2]      # the partial maxima reuse x3 [rows, h1] and x1 [rows, h0]
    return parts == 1 or (groups * parts * h0 <= rows * kpad32(h1) and groups * parts * cout <= rows * kpad32(h0))


def upscale_run_ok(Z, N, G, C, rep):
    return rep > 0 and Z > 0 and Z % rep == 0 and N > 0 and G > 0 and 0 < C <= T["UPSCALE_MAX_C"] and (Z * N) % T["UPSCALE_ROWS"] == 0 and N % T["UPSCALE_N_TILE"] == 0


def twoway_prepare_ok(depth, E, heads, mlp, downsample):
    return (0 < depth <= 4 and E > 0 and E % 32 == 0 and heads > 0 and mlp > 0 and mlp % 32 == 0 and downsample > 0 and E % downsample == 0
            and (E // downsample) % heads == 0 and E % heads == 0)


def twoway_run_ok(Z, Tk, G, rep):
    return rep > 0 and Z > 0 and Z % rep == 0 and 0 < Tk <= T["TW_MAX_KEYS"] and 0 < G <= T["TW_MAX_KEYS"]


# ------------------------------------------------------------------------------------------------ the cases
# want: the routes the case is meant to take (checked against the mirrors above by tests/test_blocks_cpu.py); refused: None, or the call that must
# answer PSAM_EINVAL ("prepare" / "run").  seed: of the case's weights and inputs.
EvaCase = namedtuple("EvaCase", "dim hidden B L heavy want refused seed", defaults=(False, None, None, 0))          # heads = dim / 64; want: Hp != hidden
GeluCase = namedtuple("GeluCase", "dim heads hidden B L keysplit counters want refused seed", defaults=(4, True, None, None, 0))      # want: (fused, head dim)
PatchCase = namedtuple("PatchCase", "h1 cout B rep G K C centralize radius N heavy want refused cin seed",
                       defaults=(500, False, None, None, None, 0))      # want: (Kp, parts, route of the pooled half); cin: None = what C and centralize give
UpscaleCase = namedtuple("UpscaleCase", "Z N G C rep heavy want refused dim seed", defaults=(False, None, None, 256, 0))      # want: the route of the first Linear
TwowayCase = namedtuple("TwowayCase", "Z T G rep edge depth E heads mlp downsample mode counters heavy want refused seed",
                        defaults=("", 2, 256, 8, 2048, 2, -1, True, False, None, None, 0))
# want of a TwowayCase: (tok_fast, fast, small_rows, key_fast, token_linear, self / t2i / i2t instance)

EVA_SHAPES = ((1, 256), (256, 1), (8, 96), (64, 100))
EVA_CASES = tuple(EvaCase(dim, hidden, B, L, want=hp, seed=100 + 10 * i + j)
                  for i, (dim, hidden, hp) in enumerate(((256, 170, True), (256, 192, False), (384, 170, True))) for j, (B, L) in enumerate(EVA_SHAPES)) + (
    EvaCase(256, 170, 2, 128, heavy=True, want=True, seed=190),
)
EVA_REFUSED = (
    EvaCase(256, 170, 3, 100, refused="run", seed=1),          # M = 300
    EvaCase(256, 96, 1, 256, refused="prepare", seed=1),       # Hp % 64
    EvaCase(256, 64, 1, 256, refused="prepare", seed=1),       # Hp = 64: below the K of a packed-operand GEMM
    EvaCase(128, 170, 2, 128, refused="prepare", seed=1),      # heads 2: below the packed LayerNorm
    EvaCase(4160, 170, 1, 256, refused="prepare", seed=1),     # heads 65: above it
    EvaCase(320, 170, 1, 256, refused="prepare", seed=1),      # 3 * 320 = 7.5 column tiles: no fused epilogue
    EvaCase(448, 170, 1, 256, refused="prepare", seed=1),      # 3 * 448 = 10.5 column tiles
    EvaCase(448, 341, 1, 256, refused="prepare", seed=1),      # and Hp = 352 is no multiple of 64
)

_G = GeluCase
GELU_DIMS = ((256, 4), (288, 4), (352, 4), (512, 4))      # head dim 64 / 72 / 88 / 128
GELU_HIDDEN = (128, 160, 256)
GELU_SHAPES = ((1, 256), (2, 150), (1, 257), (256, 1), (1, 512))      # M = 256, 300, 257; one key per cloud; a single cloud long enough for the key split
# every (dim, heads) x hidden x (B, L) with the counters and the key split the stage prepares (4); (1, 512) also with the split capped at 1; two without counters.
# One weight set per (dim, heads, hidden).  fused: whole 256-row tiles AND whole 128-column tiles of fc1.
GELU_CASES = tuple(_G(d, h, hidden, B, L, want=(B * L % 256 == 0 and hidden % 128 == 0, d // h), seed=200 + 10 * i + j)
                   for i, (d, h) in enumerate(GELU_DIMS) for j, hidden in enumerate(GELU_HIDDEN) for B, L in GELU_SHAPES) + tuple(
    _G(d, h, hidden, 1, 512, keysplit=1, want=(hidden % 128 == 0, d // h), seed=200 + 10 * i + j) for i, (d, h) in enumerate(GELU_DIMS) for j, hidden in enumerate(GELU_HIDDEN)) + (
    _G(352, 4, 256, 1, 512, counters=False, want=(True, 88), seed=222), _G(256, 4, 160, 2, 150, counters=False, want=(False, 64), seed=201),
)
GELU_REFUSED = (
    _G(256, 4, 128, 1, 255, refused="run", seed=1),           # M = 255
    _G(544, 8, 128, 1, 256, refused="prepare", seed=1),       # head dim 68
    _G(256, 4, 96, 1, 256, refused="prepare", seed=1),        # hidden below the K of a packed-operand GEMM
)

_P = PatchCase
PATCH_CASES = (
    _P(512, 512, 1, 1, 8, 32, 3, False, 0.0, want=(32, 1, "rows_multi"), seed=300),                  # the smallest: 256 rows
    _P(256, 128, 1, 2, 4, 64, 1, False, 0.1, want=(64, 1, "rows_multi"), seed=301),
    _P(384, 256, 2, 1, 1, 128, 3, True, 0.0, want=(64, 2, "rows_multi"), seed=302),                  # one group per cloud, two parts
    _P(1024, 384, 1, 1, 4, 192, 1, True, 0.1, want=(64, 3, "rows_multi"), seed=303),                 # three parts; row-bias groups of 192 rows over 128- / 256-row tiles
    _P(512, 512, 1, 2, 2, 192, 3, False, 0.1, want=(64, 3, "rows_multi"), seed=304),                 # three parts at h1 == 512
    _P(256, 128, 1, 1, 2048, 32, 1, False, 0.0, N=4096, want=(32, 1, "rows_multi"), seed=305),       # the last G of the row kernel
    _P(256, 128, 1, 1, 2056, 32, 1, False, 0.0, N=4096, want=(32, 1, "packed"), seed=306),           # the first G past it with rows % 256 == 0
    _P(512, 128, 1, 1, 2304, 32, 3, False, 0.0, N=4096, want=(32, 1, "packed"), seed=307),
    _P(512, 512, 1, 1, 8, 32, 3, False, 0.0, heavy=True, want=(32, 1, "rows_multi"), seed=308),
)
PATCH_REFUSED = (
    _P(512, 512, 1, 1, 16, 48, 3, False, 0.0, refused="run", seed=1),                # K = 48 (rows = 768)
    _P(512, 512, 1, 1, 5, 32, 3, False, 0.0, refused="run", seed=1),                 # rows = 160
    _P(320, 512, 1, 1, 8, 32, 3, False, 0.0, refused="prepare", seed=1),             # h1 = 320
    _P(512, 512, 1, 1, 8, 32, 1, False, 0.0, refused="run", cin=6, seed=1),          # the first Linear has 6 inputs, the call brings 3 + 1
)

_U = UpscaleCase
UPSCALE_CASES = (
    _U(1, 256, 3, 1, 1, want="rows_multi", seed=400),
    _U(8, 32, 16, 4, 2, want="rows_multi", seed=401),
    _U(3, 768, 37, 3, 3, want="rows_multi", seed=402),
    _U(1, 2304, 2304, 2, 1, want="packed", seed=403),
    _U(1, 256, 3, 1, 1, heavy=True, want="rows_multi", seed=404),
)
UPSCALE_REFUSED = (
    _U(1, 48, 3, 1, 1, refused="run", seed=1),
    _U(1, 256, 3, 5, 1, refused="run", seed=1),
    _U(1, 256, 3, 1, 1, refused="prepare", dim=128, seed=1),
)

_T = TwowayCase
TWOWAY_CASES = (
    _T(1, 7, 256, 1, "I = 256", want=(True, True, True, True, "skinny", 0, 1, 4), seed=500),
    _T(1, 7, 255, 1, "I = 255", want=(True, False, False, False, "skinny", 0, 1, 4), seed=501),
    _T(2, 5, 32, 1, "small G", want=(True, False, False, False, "skinny", 0, 0, 0), seed=502),
    _T(8, 8, 32, 1, "R = 64", want=(True, True, True, True, "skinny", 0, 0, 0), seed=503),
    _T(5, 13, 52, 1, "R = 65", want=(False, False, False, True, "linear", 0, 0, 0), seed=504),
    _T(32, 8, 8, 1, "R = 256", want=(False, False, False, True, "packed", 0, 0, 0), seed=505),
    _T(4, 7, 64, 2, "rep = 2", want=(True, True, True, True, "skinny", 0, 0, 4), seed=506),
    _T(1, 1, 256, 1, "T = 1", want=(True, True, True, True, "skinny", 0, 1, 4), seed=507),
    _T(1, 16, 256, 1, "T = 16", want=(True, True, True, True, "skinny", 0, 1, 4), seed=508),
    _T(1, 17, 256, 1, "T = 17", want=(True, True, True, True, "skinny", 0, 1, 0), seed=509),
    _T(1, 7, 2048, 1, "G = 2048", want=(True, True, True, True, "skinny", 0, 1, 4), seed=510),
    _T(1, 7, 2049, 1, "G = 2049", want=(True, True, False, True, "skinny", 0, 1, 4), seed=511),
    _T(1, 7, 8192, 1, "Lk limit", want=(True, True, False, True, "skinny", 0, 1, 4), seed=512),
    # the three launch sequences and NULL counters at both sides of small_rows
    _T(1, 7, 256, 1, "I = 256, operator sequence", mode=0, want=(True, False, False, True, "skinny", 0, 1, 4), seed=500),
    _T(1, 7, 256, 1, "I = 256, regrouped, packed GEMMs", mode=1, want=(True, True, False, True, "skinny", 0, 1, 4), seed=500),
    _T(1, 7, 256, 1, "I = 256, regrouped, row kernel", mode=2, want=(True, True, True, True, "skinny", 0, 1, 4), seed=500),
    _T(1, 7, 256, 1, "I = 256, NULL counters", counters=False, want=(True, False, False, True, "skinny", 0, 1, 4), seed=500),
    _T(1, 7, 2049, 1, "G = 2049, operator sequence", mode=0, want=(True, False, False, True, "skinny", 0, 1, 4), seed=511),
    _T(1, 7, 2049, 1, "G = 2049, regrouped, packed GEMMs", mode=1, want=(True, True, False, True, "skinny", 0, 1, 4), seed=511),
    _T(1, 7, 2049, 1, "G = 2049, regrouped, row kernel asked", mode=2, want=(True, True, False, True, "skinny", 0, 1, 4), seed=511),
    _T(1, 7, 2049, 1, "G = 2049, NULL counters", counters=False, want=(True, False, False, True, "skinny", 0, 1, 4), seed=511),
    _T(1, 7, 256, 1, "depth 1", depth=1, want=(True, True, True, True, "skinny", 0, 1, 4), seed=520),
    _T(1, 7, 256, 1, "downsample 1", downsample=1, want=(True, False, False, True, "skinny", 0, 1, 8), seed=521),
    _T(1, 7, 256, 1, "downsample 4", downsample=4, want=(True, False, False, False, "skinny", 0, 1, 0), seed=522),      # head dim 8: the split kernel takes it, the few-keys kernels do not
    _T(1, 7, 256, 1, "E = 128", E=128, heads=4, mlp=96, want=(True, False, False, False, "skinny", 0, 1, 4), seed=523),
    _T(2, 5, 32, 1, "small G, heavy-tailed", heavy=True, want=(True, False, False, False, "skinny", 0, 0, 0), seed=525),      # (seeds 524 and 526 give softmaxes the fp32 oracle itself misses by 1e-4)
)
TWOWAY_REFUSED = (
    _T(1, 7, 8193, 1, "G = 8193", refused="run", seed=1),
    _T(3, 7, 32, 2, "Z % rep", refused="run", seed=1),
)


# (dim, heads, hidden) of the two block entries and (h0, h1, cout) of the patch encoder: supported(...) is true exactly when *_prepare returns 0
SUPPORTED_GRID = tuple((dim, heads, hidden) for dim, heads in ((64, 1), (128, 2), (192, 3), (256, 4), (288, 4), (272, 4), (320, 5), (384, 6), (448, 7), (512, 4), (512, 8), (352, 4))
                       for hidden in (64, 96, 128, 160, 170, 192, 341)) + ((4096, 64, 128), (4096, 32, 128), (4160, 65, 128))
PATCH_GRID = tuple((h0, h1, cout) for h0 in (64, 128) for h1 in (128, 256, 320, 384, 512, 4096, 4224) for cout in (64, 128, 192, 384))


def twoway_want(c):
    """The routes of a TwowayCase as its `want` tuple names them."""
    r = twoway_route(c.Z, c.T, c.G, c.E, c.downsample, c.mlp, c.counters, 2 if c.mode < 0 else c.mode, c.heads)
    return (r["tok_fast"], r["fast"], r["small_rows"], r["key_fast"], r["token_linear"], r["attn"]["self"], r["attn"]["t2i"], r["attn"]["i2t"])


def patch_cin(c):
    return c.cin if c.cin is not None else 3 + c.C * (2 if c.centralize else 1)
