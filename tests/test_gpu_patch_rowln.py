"""psam_linear128_ln_gelu_pack (csrc/patch_rowln.hip): PatchEncoder's per-row half of conv2.0 (128 -> 512), conv2.1's LayerNorm and its GELU as ONE
persistent register-row kernel that writes g8-packed rows, against fp64 on the exactly decoded packed inputs.  The yardstick is the two-launch sequence it
replaces -- the packed-operand GEMM with a bias row per group (ops.linear) and the packing LayerNorm (ops.layernorm, psam_layernorm_ex) -- on the same
inputs: the new kernel's maximum error against fp64 may be at most twice that sequence's own (the factor covers the different summation order of the row
statistics; the products and their order are the GEMM's).  Run with ``pytest -m gpu -s`` to see the table (profiles/blocks/patch_rowln.md)."""
import functools
import math

import pytest
import torch

from g8_reference import unpack_g8

pytestmark = pytest.mark.gpu

H0, H1, EPS = 128, 512, 1e-5
# (name, rows, group size K, special): K = 64 one bias row per 64-row block; K = 32 the bias row changes inside a block; K = 256 one bias row spans four
# blocks (cfg #3's group size); 256 x 301 rows = 1204 blocks, more than any grid of two workgroups per CU: every workgroup takes a second trip, some a third;
# special: a block of all-zero rows under a zero bias row (variance 0: eps decides), one row with a single input 1e4 x the others, one gamma 50 x the rest
CASES = [("one trip", 256, 64, False), ("bias row changes inside a block", 256, 32, False), ("bias row spans four blocks", 1024, 256, False),
         ("1204 blocks", 256 * 301, 64, False), ("zero variance, input and gamma outliers", 256, 64, True)]
IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd import ops as _ops
    _ops._lib.load()
    return _ops


def _gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """The case's packed inputs on the device, decoded exactly, and its fp64 result -- built once, shared by the tests, never written."""
    from point_sam_amd import ops
    _, rows, K, special = CASES[IDS.index(name)]
    g = torch.Generator().manual_seed(1000 + IDS.index(name))
    x = torch.randn(rows, H0, generator=g) * torch.exp(0.5 * torch.randn(rows, 1, generator=g))
    W = torch.randn(H1, H0, generator=g) / 11
    gamma, beta = 1.0 + 0.1 * torch.randn(H1, generator=g), 0.1 * torch.randn(H1, generator=g)
    g1 = torch.randn(rows // K, H1, generator=g)
    if special:
        x[:64] = 0.0; g1[0] = 0.0          # block 0: y == 0 in every column
        x[100, 7] *= 1e4                   # one input 1e4 x the row's others
        gamma[13] *= 50.0
    xp, sx = ops.scale_pack_rows_g8(x.cuda())
    fw = ops.F16Weight(W.cuda().contiguous())
    gamma, beta, g1 = gamma.cuda(), beta.cuda(), g1.cuda().contiguous()
    bound = 1.001 * ops.row_ln_bound(gamma, beta) + 1e-30
    xd = unpack_g8(xp.view(torch.int32), sx, H0)
    wd = unpack_g8(fw.packed.view(torch.int32), fw.scale, H0)
    y = xd @ wd.T + g1.double().repeat_interleave(K, dim=0)
    mu = y.mean(dim=1, keepdim=True)
    var = ((y - mu) ** 2).mean(dim=1, keepdim=True)
    want = _gelu64((y - mu) / torch.sqrt(var + EPS) * gamma.double() + beta.double())
    return dict(rows=rows, K=K, xp=xp, sx=sx, fw=fw, gamma=gamma, beta=beta, g1=g1, bound=bound, want=want)


@pytest.fixture(scope="module", autouse=True)
def _free_inputs():
    yield
    _inputs.cache_clear()      # the largest case holds a few hundred MB of device memory


def _run(ops, c):
    out = torch.empty(c["rows"], H1, dtype=torch.float32, device="cuda")
    rs = torch.empty(c["rows"], dtype=torch.float32, device="cuda")
    with ops.gemm_mode("f16x3"):
        ops.linear128_ln_gelu_pack(c["xp"], c["sx"], c["fw"], c["g1"], c["K"], c["gamma"], c["beta"], EPS, c["bound"], out, rs)
    return out, rs


def _pair(ops, c):
    """The two launches the kernel replaces."""
    with ops.gemm_mode("f16x3"):
        h = ops.linear(c["xp"], c["fw"], None, rowbias=c["g1"], rowgroup=c["K"], x_scale=c["sx"], x_packed=True)
        rs = torch.empty(c["rows"], dtype=torch.float32, device="cuda")
        out = ops.layernorm(h, c["gamma"], c["beta"], EPS, act=ops.ACT_GELU, out=torch.empty_like(h), scale_out=rs, pack=True)
    return out, rs


@pytest.mark.parametrize("name", IDS)
def test_error_against_fp64_within_twice_the_two_launch_sequence(ops, name):
    c = _inputs(name)
    out, rs = _run(ops, c)
    ref, rs2 = _pair(ops, c)
    got = unpack_g8(out.view(torch.int32), rs, H1)
    err = float((got - c["want"]).abs().max())
    err_pair = float((unpack_g8(ref.view(torch.int32), rs2, H1) - c["want"]).abs().max())
    print(f"\n| {name} | {c['rows']} | {c['K']} | {err:.3e} | {err_pair:.3e} | {err / err_pair:.2f} |")
    assert torch.isfinite(got).all()
    # one scale for every row: the power of two that puts the a-priori bound into [2^14, 2^15)
    s = 2.0 ** (14 - math.floor(math.log2(c["bound"])))
    assert torch.equal(rs, torch.full_like(rs, s))
    assert err <= 2.0 * err_pair, (err, err_pair)
    if CASES[IDS.index(name)][3]:
        # variance 0: (y - mean) rstd == 0 whatever rstd = 1 / sqrt(eps) is, so the rows are gelu(beta).  Tolerance from the formats: erff to a few fp32
        # ulps (4 x 2^-24) and the hi + lo split to 2^-22, both relative to values below 1
        zero = got[:64]
        assert torch.isfinite(zero).all()
        assert float((zero - _gelu64(c["beta"].double())[None]).abs().max()) <= 4 * 2.0 ** -24 + 2.0 ** -22


def test_two_runs_are_bit_equal(ops):
    c = _inputs("1204 blocks")
    a, b = _run(ops, c), _run(ops, c)
    torch.cuda.synchronize()
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def test_bitwise_stable_beside_a_gemm_loop_on_another_stream(ops):
    """The same bits alone and while another stream's GEMM workgroups share the CUs (the pattern of test_fused_mlp_bitwise_stable_beside_other_streams)."""
    c = _inputs("1204 blocks")
    g = torch.Generator().manual_seed(7)
    M, D = 4096, 1024
    with ops.gemm_mode("f16x3"):
        hp, sh = ops.scale_pack_rows_g8(torch.randn(M, D, generator=g).cuda())
        wq, bq = ops.F16Weight((torch.randn(3 * D, D, generator=g) / 32).cuda()), torch.zeros(3 * D, device="cuda")
        ops.linear(hp, wq, bq, x_scale=sh, x_packed=True)      # the weight is packed on first use, outside the loop
        ref = _run(ops, c)
        torch.cuda.synchronize()
        s2 = torch.cuda.Stream()
        for it in range(4):
            s2.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s2):
                for _ in range(6):
                    ops.linear(hp, wq, bq, x_scale=sh, x_packed=True)
            out = _run(ops, c)
            torch.cuda.synchronize()
            assert torch.equal(out[0].view(torch.int32), ref[0].view(torch.int32)) and torch.equal(out[1], ref[1]), it
