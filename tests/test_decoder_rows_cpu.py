"""The size lists of tests/decoder_sizes.py (what tests/test_gpu_decoder_rows.py runs on the GPU) follow from the constants of the decoder's small-row
kernels in csrc/gemm.hip and csrc/rowops.hip: a changed SK_CH, MLP3_OB / MLP3_NW / MLP3_MAXD, K range or range cap of skinny_ln_ksplit, `K & 127`
dispatch or K limit of linear_ln256 fails here, without a GPU, until the lists cover the new boundaries."""
import decoder_sizes as DS
import test_gpu_decoder_rows as G      # the case lists only: nothing below touches a GPU


def test_tested_sizes_follow_from_the_kernel_sources():
    c = DS.constants()
    assert (c["SK_CH"], c["R"], c["LN_RANGE"], c["LN_CAP"], c["FULL_MASK"], c["LN256_MAX_K"]) == (8, 128, 256, 8, 127, 512)
    assert (c["MLP3_MAXD"], c["MLP3_OB"], c["MLP3_NW"], c["MLP3_CHUNK"], c["OBW"]) == (1024, 16, 16, 256, 256)
    assert DS.k_sizes(c) == DS.K_SIZES
    assert DS.ln_k_sizes(c) == DS.LN_K_SIZES
    assert DS.ln256_k_sizes(c) == DS.LN256_K_SIZES
    assert DS.mlp3_in_sizes(c) == DS.MLP3_IN_SIZES
    assert DS.mlp3_out_sizes(c) == DS.MLP3_OUT_SIZES
    R = c["R"]
    for Ks in (DS.K_SIZES, DS.LN_K_SIZES, DS.LN256_K_SIZES):
        assert all(K % 16 == 0 for K in Ks)
    # rounds of the K loop: one ragged, one full, a ragged one after one and after two full ones
    assert [(-(-K // R), K % R != 0) for K in DS.K_SIZES] == [(1, True), (1, True), (1, False), (2, True), (3, True)]
    # both instances of linear_rows_multi run, and <false> with a ragged round behind a full one; FULL means what the kernel's comment says
    assert c["FULL_MASK"] == R - 1
    assert {DS.rows_multi_full(c, K) for K in DS.K_SIZES} == {True, False}
    assert any(not DS.rows_multi_full(c, K) and K > R for K in DS.K_SIZES)
    assert max(DS.LN256_K_SIZES) == c["LN256_MAX_K"] and c["LN256_MAX_K"] + 16 not in DS.LN256_K_SIZES
    # mlp3: trips of the kc loop and of the ob loop, the clamps of a ragged last chunk and of a ragged last block of rows
    C, OB, OBW = c["MLP3_CHUNK"], c["MLP3_OB"], c["OBW"]
    assert [-(-n // C) for n in DS.MLP3_IN_SIZES] == [1, 1, 1, 2, 3, 4] and all(n % 4 == 0 for n in DS.MLP3_IN_SIZES)
    assert [-(-n // OBW) for n in DS.MLP3_OUT_SIZES] == [1, 1, 1, 1, 1, 2, 2]
    assert DS.MLP3_TALL > OBW and DS.MLP3_TALL % OB not in (0, 1)
    assert c["MLP3_MAXD"] % C == 0 and c["MLP3_MAXD"] > OBW      # dh = MLP3_MAXD: the ob loop's fourth trip


def test_skinny_ln_ranges_cover_k():
    """(ksplit, kper) as psam_linear_skinny_ln computes them: every K range of the grid is non-empty, starts on a 16-k slot, and the ranges tile [0, K)."""
    c = DS.constants()
    splits = {K: DS.ln_split(c, K) for K in DS.LN_K_SIZES}
    assert splits == {16: (1, 16), 112: (1, 112), 128: (1, 128), 144: (1, 144), 272: (2, 144), 528: (3, 176), 2048: (8, 256), 2064: (8, 272), 4096: (8, 512)}
    for K in sorted(set(DS.LN_K_SIZES) | set(range(16, 8192 + 16, 16))):
        ksplit, kper = DS.ln_split(c, K)
        assert 1 <= ksplit <= c["LN_CAP"] and kper % 16 == 0
        rs = DS.ln_ranges(c, K)
        assert len(rs) == ksplit and rs[0][0] == 0 and rs[-1][1] == K
        assert all(k0 < k1 for k0, k1 in rs), (K, rs)
        assert all(a[1] == b[0] for a, b in zip(rs, rs[1:]))
    R = c["R"]
    rounds = {K: max(-(-(k1 - k0) // R) for k0, k1 in DS.ln_ranges(c, K)) for K in DS.LN_K_SIZES}
    assert rounds[2064] == 3 and rounds[4096] == 4 and rounds[2048] == 2      # past two load rounds per range only above the cap
    assert any(len({k1 - k0 for k0, k1 in DS.ln_ranges(c, K)}) == 2 for K in (272, 528, 2064))      # a shorter last range


def test_skinny_jobs_struct_matches_the_header():
    import ctypes

    from point_sam_amd import _lib
    c = DS.constants()
    assert _lib.SkinnyJobs.job.size == c["MAX_JOBS"] * ctypes.sizeof(_lib.SkinnyJob)
    assert len(_lib.SkinnyJobs().job) == c["MAX_JOBS"]


# ------------------------------------------------------------------------------------------------ the cases of tests/test_gpu_decoder_rows.py
def test_skinny_cases_cover_every_axis():
    assert {c[0] for c in G.SKINNY_CASES} >= set(G.SKINNY_M) and {c[1] for c in G.SKINNY_CASES} >= set(G.SKINNY_N)
    assert {c[2] for c in G.SKINNY_CASES} == set(DS.K_SIZES) and {c[3] for c in G.SKINNY_CASES} == {0, 1, 2}
    assert {c[4:] for c in G.SKINNY_CASES} == {(False, False), (True, True), (True, False), (False, True)}
    for K in DS.K_SIZES:      # every ragged K meets a ragged M and a ragged N
        if K % 128:
            assert any(c[2] == K and c[0] % 16 and c[1] % 16 for c in G.SKINNY_CASES), K


def test_rows_multi_cases_cover_every_axis():
    c = DS.constants()
    assert {m for m, _, _, _ in G.ROWS_CASES} == {1, 31, 32, 33, 77 * 3} and {k for _, _, _, k in G.ROWS_CASES} == set(DS.K_SIZES)
    assert {rep for _, _, rep, _ in G.ROWS_CASES} == {1, 3} and all(M % (rps * rep) == 0 for M, rps, rep, _ in G.ROWS_CASES)
    assert {DS.rows_multi_full(c, K) for _, _, _, K in G.ROWS_CASES} == {True, False}
    assert any(rep == 1 and rps % 32 and M > rps for M, rps, rep, _ in G.ROWS_CASES)      # a 32-row block across two addend sets


def test_ln_cases_cover_every_axis():
    assert {m for m, _ in G.SKINNY_LN_CASES} == set(G.SKINNY_LN_M) and {k for _, k in G.SKINNY_LN_CASES} == set(DS.LN_K_SIZES)
    assert {m for m, _ in G.LN256_CASES} == {1, 15, 16, 17, 33} and {k for _, k in G.LN256_CASES} == set(DS.LN256_K_SIZES)


def test_mlp3_cases_cover_every_axis():
    c = DS.constants()
    assert {a[0] for a in G.MLP3_CASES} == {a[1] for a in G.MLP3_CASES} == set(DS.MLP3_IN_SIZES) and {a[2] for a in G.MLP3_CASES} == set(DS.MLP3_OUT_SIZES)
    assert {a[3] for a in G.MLP3_CASES} == {a[4] for a in G.MLP3_CASES} == {1, 3}
    assert any(din % c["MLP3_CHUNK"] and dh > c["OBW"] and dout > 1 and dout % c["MLP3_OB"] for din, dh, dout, _, _ in G.MLP3_CASES)

