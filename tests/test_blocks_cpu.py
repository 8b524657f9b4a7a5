"""The case lists of tests/block_cases.py (what tests/test_gpu_blocks.py runs on the GPU) follow from the dispatch decisions of csrc/blocks.hip and of
psam_attention_small in csrc/rowops.hip: the thresholds are read from the source text, every decision takes each of its values in some case, every
threshold has a case on it and one a step past it, every case passes (or, where it says so, misses) the entry's shape conditions, and the fp64 reference
of tests/block_reference.py is well conditioned on every case's inputs.  Nothing here touches a GPU."""
import pytest
import torch

import block_cases as BC
import block_reference as BR

ALL_OK = BC.EVA_CASES + BC.GELU_CASES + BC.PATCH_CASES + BC.UPSCALE_CASES + BC.TWOWAY_CASES
ALL_REFUSED = BC.EVA_REFUSED + BC.GELU_REFUSED + BC.PATCH_REFUSED + BC.UPSCALE_REFUSED + BC.TWOWAY_REFUSED


def test_thresholds_match_the_sources():
    c = BC.constants()
    assert c == BC.THRESHOLDS, {k: (c.get(k), v) for k, v in BC.THRESHOLDS.items() if c.get(k) != v}
    assert (c["PACKED_MIN_M"], c["SKINNY_MAX_M"], c["ROWS_MULTI_MAX"], c["K_MASK"], c["PACKED_MIN_NK"], c["PART_ROWS"]) == (256, 64, 2048, 15, 128, 64)
    assert (c["ROW_LN_H1"], c["ROW_LN_ROWS"], c["FAST_E"], c["FAST_IX_MIN"], c["FAST_IX_MAX"]) == (512, 128, 256, 128, 512)
    assert (c["FEWKEYS_MAX_LK"], c["FEWKEYS_MIN_LQ"], c["SPLIT_MIN_LK"], c["SPLIT_MAX_WAVES"]) == (16, 64, 128, 2048)
    # the two-way decoder's own limit is the key limit of the attention it is built from
    assert c["TW_MAX_KEYS"] * c["ATTN_BYTES_PER_KEY"] == c["ATTN_LDS_BYTES"] and c["TW_MAX_KEYS"] == 8192


def test_a_changed_literal_is_noticed(tmp_path):
    """An edited copy of the sources: each threshold literal changed alone makes constants() differ from THRESHOLDS (or the parser refuse the text)."""
    import os
    srcs = {n: open(os.path.join(BC.CSRC, n)).read() for n in ("blocks.hip", "rowops.hip")}
    edits = [("blocks.hip", "rows_per_cloud <= 2048", "rows_per_cloud <= 1024"), ("blocks.hip", "if (M >= 256 && l.packed) {", "if (M >= 512 && l.packed) {"),
             ("blocks.hip", "const bool tok_fast = R <= 64 ", "const bool tok_fast = R <= 32 "), ("blocks.hip", "if (l.N >= 128 && l.K >= 128) {", "if (l.N >= 256 && l.K >= 128) {"),
             ("blocks.hip", "IX <= 512 && I >= 256 &&", "IX <= 512 && I >= 128 &&"), ("blocks.hip", "const int Kp = K <= 64 ? K : 64,", "const int Kp = K <= 32 ? K : 32,"),
             ("blocks.hip", "if (h1 == 512 && rows % 128 == 0", "if (h1 == 256 && rows % 128 == 0"), ("blocks.hip", "PSAM_REQUIRE(T <= 8192 && G <= 8192,", "PSAM_REQUIRE(T <= 8192 && G <= 16384,"),
             ("blocks.hip", "const bool key_fast = I >= 256 &&", "const bool key_fast = I >= 64 &&"), ("blocks.hip", "(M % 256 == 0) && (H % 128 == 0)", "(M % 256 == 0) && (H % 64 == 0)"),
             ("rowops.hip", "(size_t)Lk * 16 <= 128 * 1024, PSAM_EINVAL", "(size_t)Lk * 16 <= 64 * 1024, PSAM_EINVAL"), ("rowops.hip", "if (Lk <= 16 && Lq >= 64 && aligned", "if (Lk <= 32 && Lq >= 64 && aligned"),
             ("rowops.hip", "Lk >= 128 && waves <= 2048 && aligned", "Lk >= 128 && waves <= 4096 && aligned")]
    for name, old, new in edits:
        assert srcs[name].count(old) == 1, old
        d = tmp_path / ("e%d" % edits.index((name, old, new)))
        d.mkdir()
        for n, s in srcs.items():
            (d / n).write_text(s.replace(old, new) if n == name else s)
        try:
            changed = BC.constants(str(d)) != BC.THRESHOLDS
        except AssertionError:
            changed = True
        assert changed, old


def test_every_case_names_the_routes_it_takes():
    for c in BC.EVA_CASES:
        assert c.want == (BC.kpad32(c.hidden) != c.hidden), c
    for c in BC.GELU_CASES:
        assert c.want == (BC.eva_gelu_fused(c.B * c.L, c.hidden, 1), c.dim // c.heads), c      # K = dim < 1024: the library never splits K here
    for c in BC.PATCH_CASES:
        groups = c.B * c.rep * c.G
        fused, Kp, parts = BC.patch_route(c.h1, groups * c.K, c.K)
        assert not fused and c.want == (Kp, parts, BC.host_linear_route(groups, c.G, 0, 128, True)), c
    for c in BC.UPSCALE_CASES:
        assert c.want == BC.host_linear_route(c.Z * c.G, c.G, 0, c.dim, True), c
    for c in BC.TWOWAY_CASES:
        assert c.want == BC.twoway_want(c), (c, BC.twoway_want(c))


def test_every_decision_goes_both_ways():
    T = BC.THRESHOLDS
    assert {c.want for c in BC.EVA_CASES} == {True, False}
    assert {(c.B, c.L) for c in BC.EVA_CASES} >= set(BC.EVA_SHAPES) and {(c.dim, c.hidden) for c in BC.EVA_CASES} == {(256, 170), (256, 192), (384, 170)}
    assert any((3 * c.dim // T["EVA_DIM_TILE"]) % 2 for c in BC.EVA_CASES)      # an odd number of 128-column tiles under the packed-output epilogue
    assert {c.want[0] for c in BC.GELU_CASES} == {True, False} and {c.want[1] for c in BC.GELU_CASES} == {64, 72, 88, 128}
    assert {c.hidden for c in BC.GELU_CASES} == {128, 160, 256} and {(c.B, c.L) for c in BC.GELU_CASES} == {(1, 256), (2, 150), (1, 257), (256, 1), (1, 512)}
    assert {(c.dim, c.heads, c.hidden, c.B, c.L) for c in BC.GELU_CASES} == {(d, h, hid, B, L) for d, h in BC.GELU_DIMS for hid in BC.GELU_HIDDEN for B, L in BC.GELU_SHAPES}
    assert {c.keysplit for c in BC.GELU_CASES if (c.B, c.L) == (1, 512)} == {1, 4} and {c.counters for c in BC.GELU_CASES} == {True, False}
    assert any(c.B * c.L % T["GELU_FUSED_M"] and c.hidden % T["GELU_FUSED_H"] == 0 for c in BC.GELU_CASES)      # unfused by the rows alone
    assert any(c.B * c.L % T["GELU_FUSED_M"] == 0 and c.hidden % T["GELU_FUSED_H"] for c in BC.GELU_CASES)      # unfused by the hidden width alone
    P = BC.PATCH_CASES
    assert {c.K for c in P} == {32, 64, 128, 192} and {c.want[1] for c in P} == {1, 2, 3} and {c.want[2] for c in P} == {"rows_multi", "packed"}
    assert {(c.h1, c.cout) for c in P} >= {(512, 512), (256, 128), (384, 256), (1024, 384)} and {c.C for c in P} == {1, 3} and {c.centralize for c in P} == {True, False}
    assert {c.radius for c in P} == {0.0, 0.1} and {c.rep for c in P} == {1, 2}
    assert {c.h1 == T["ROW_LN_H1"] for c in P if c.K == 192} == {True, False}
    assert min(c.B * c.rep * c.G * c.K for c in P) == T["PATCH_ROWS"] and any(c.G == 2304 and c.K == 32 for c in P)
    assert {c.G for c in P} >= {T["ROWS_MULTI_MAX"], T["ROWS_MULTI_MAX"] + 8}      # 2056: the first G past the limit with G * 32 % 256 == 0
    assert {(c.Z, c.N, c.G, c.C, c.rep) for c in BC.UPSCALE_CASES} == {(1, 256, 3, 1, 1), (8, 32, 16, 4, 2), (3, 768, 37, 3, 3), (1, 2304, 2304, 2, 1)}
    assert {c.want for c in BC.UPSCALE_CASES} == {"rows_multi", "packed"}
    W = [c.want for c in BC.TWOWAY_CASES]
    for i in range(4):
        assert {w[i] for w in W} == {True, False}, i
    assert {w[4] for w in W} == {"skinny", "linear", "packed"}
    assert {w[5] for w in W} == {0} and {w[6] for w in W} == {0, 1} and {w[7] for w in W} == {0, 4, 8}      # the tokens never are 128 keys here (the split kernel runs for the patch keys)
    tw = BC.TWOWAY_CASES
    shapes = {(c.Z, c.T, c.G, c.rep) for c in tw}
    assert shapes == {(1, 7, 256, 1), (1, 7, 255, 1), (2, 5, 32, 1), (8, 8, 32, 1), (5, 13, 52, 1), (32, 8, 8, 1), (4, 7, 64, 2), (1, 1, 256, 1), (1, 16, 256, 1), (1, 17, 256, 1),
                      (1, 7, 2048, 1), (1, 7, 2049, 1), (1, 7, 8192, 1)}
    # every threshold: a case on it and a case one step past it
    assert {c.Z * c.G for c in tw} >= {T["PACKED_MIN_M"] - 1, T["PACKED_MIN_M"]} and {c.Z * c.T for c in tw} >= {T["SKINNY_MAX_M"], T["SKINNY_MAX_M"] + 1, T["PACKED_MIN_M"]}
    assert {c.G for c in tw} >= {T["ROWS_MULTI_MAX"], T["ROWS_MULTI_MAX"] + 1, T["TW_MAX_KEYS"]} and {c.G for c in BC.TWOWAY_REFUSED} >= {T["TW_MAX_KEYS"] + 1}
    assert {c.T for c in tw if c.G >= T["FEWKEYS_MIN_LQ"]} >= {T["FEWKEYS_MAX_LK"], T["FEWKEYS_MAX_LK"] + 1}
    for shape in ((1, 7, 256, 1), (1, 7, 2049, 1)):
        assert {(c.mode, c.counters) for c in tw if (c.Z, c.T, c.G, c.rep) == shape and (c.depth, c.downsample, c.E) == (2, 2, 256)} >= {(-1, True), (0, True), (1, True), (2, True), (-1, False)}
    assert {c.depth for c in tw} == {1, 2} and {c.downsample for c in tw} == {1, 2, 4} and {(c.E, c.heads, c.mlp) for c in tw} == {(256, 8, 2048), (128, 4, 96)}
    assert {2 * (c.E // c.downsample) <= c.E for c in tw} == {True, False} and {c.E // c.downsample >= T["FAST_IX_MIN"] for c in tw} == {True, False}
    heavy = [c for c in ALL_OK if getattr(c, "heavy", False)]
    assert len(heavy) == 4 and {type(c) for c in heavy} == {BC.EvaCase, BC.PatchCase, BC.UpscaleCase, BC.TwowayCase}


def _accepted(c):
    """(prepare accepted, run accepted) by the mirrored shape conditions."""
    if isinstance(c, BC.EvaCase):
        return BC.eva_prepare_ok(c.dim, c.dim // 64, c.hidden), BC.eva_run_ok(c.B, c.L)
    if isinstance(c, BC.GeluCase):
        return BC.gelu_prepare_ok(c.dim, c.heads, c.hidden), BC.gelu_run_ok(c.B, c.L)
    if isinstance(c, BC.PatchCase):
        return BC.patch_prepare_ok(128, c.h1, c.cout, BC.patch_cin(c)), BC.patch_run_ok(c.B, c.rep, c.G, c.K, c.C, c.centralize, BC.patch_cin(c), 128, c.h1, c.cout)
    if isinstance(c, BC.UpscaleCase):
        return c.dim == BC.T["UPSCALE_DIM"], BC.upscale_run_ok(c.Z, c.N, c.G, c.C, c.rep)
    return BC.twoway_prepare_ok(c.depth, c.E, c.heads, c.mlp, c.downsample), BC.twoway_run_ok(c.Z, c.T, c.G, c.rep)


def test_every_case_passes_the_shape_conditions_of_its_entry():
    for c in ALL_OK:
        assert c.refused is None and _accepted(c) == (True, True), c
    for c in ALL_REFUSED:
        prep, run = _accepted(c)
        assert c.refused in ("prepare", "run")
        assert (not prep) if c.refused == "prepare" else (prep and not run), c      # a run case is refused by the run alone: its prepare must succeed
    # none of the accepted two-way cases reaches an attention psam_attention_small would refuse in mid-sequence
    for c in BC.TWOWAY_CASES:
        assert "refused" not in c.want
    assert BC.attention_small_instance(1, 8, 7, 8193, 16) == "refused" and BC.attention_small_instance(1, 8, 7, 8192, 16) == 1


def test_supported_mirrors_agree_with_ops():
    """EvaBlock / EvaGeluBlock / CPatchEncoder.supported are the mirrored prepare conditions (tests/test_gpu_blocks.py holds both against *_prepare)."""
    from point_sam_amd import ops
    for dim, heads, hidden in BC.SUPPORTED_GRID:
        assert ops.EvaBlock.supported(dim, heads, hidden) == BC.eva_prepare_ok(dim, heads, hidden), (dim, heads, hidden)
        assert ops.EvaGeluBlock.supported(dim, heads, hidden) == BC.gelu_prepare_ok(dim, heads, hidden), (dim, heads, hidden)
    for h0, h1, cout in BC.PATCH_GRID:
        assert ops.CPatchEncoder.supported(h0, h1, cout) == BC.patch_prepare_ok(h0, h1, cout), (h0, h1, cout)
    assert {BC.eva_prepare_ok(*g) for g in BC.SUPPORTED_GRID} == {BC.gelu_prepare_ok(*g) for g in BC.SUPPORTED_GRID} == {BC.patch_prepare_ok(*g) for g in BC.PATCH_GRID} == {True, False}


@pytest.mark.parametrize("case", [c for c in ALL_OK if BR._key(c) not in {BR._key(d) for d in ALL_OK[:ALL_OK.index(c)]}], ids=lambda c: "-".join(str(v) for v in BR._key(c)[:8]))
def test_the_reference_alone_is_healthy(case):
    """e32 = max |y32 - y64| / max(1, max |y64|) of the fp32 oracle on the case's inputs: 0 < e32 < 1e-5 -- a condition on the inputs (no near-constant row
    into a LayerNorm, no cancelling sum), so the GPU test's allowance c * e32 cannot hide a failure."""
    _, _, y64, e32 = BR.problem(case)
    assert all(torch.isfinite(y).all() for y in y64)
    print(f"\n[{type(case).__name__}] e32 {['%.2e' % e for e in e32]} max|y64| {['%.1f' % y.abs().max() for y in y64]}")
    assert all(0.0 < e < 1e-5 for e in e32), (case, e32)
