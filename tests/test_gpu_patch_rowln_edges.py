"""psam_linear128_ln_gelu_pack (csrc/patch_rowln.hip) at its edges.  Most of what the kernel promises is exact: every output row depends on its own input
row, its scale, its bias row and the column constants only, in an arithmetic order that does not depend on where the row sits, on the leading dimensions,
on how many rows share a bias row or on which trip of which workgroup computes it.  Those tests compare int32 views with torch.equal -- no tolerance.  The
cases (patch_rowln_cases.py) are packed on the CPU, so their bits are known without a GPU; out and out_scale always lie between guard words, and every run
checks them.  The tests against fp64 keep test_gpu_patch_rowln.py's yardstick: at most twice the error of the GEMM + LayerNorm pair on the same bits.
Run with ``pytest -m gpu -s`` to see the table (profiles/blocks/patch_rowln.md)."""
import functools
import math

import pytest
import torch

import patch_rowln_cases as PC
from g8_reference import unpack_g8

pytestmark = pytest.mark.gpu

H0, H1, EPS = PC.H0, PC.H1, PC.EPS


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd import ops as _ops
    _ops._lib.load()
    return _ops


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _trip_pool():
    return PC.trip_case(4 * _cus() + 1)


@pytest.fixture(scope="module", autouse=True)
def _free_pool():
    yield
    _trip_pool.cache_clear()


def _launch(ops, d, K, bound, eps=EPS, lo=0, hi=None):
    """One launch on rows lo .. hi - 1 of the placed operands (multiples of 64 and of K: the pointers stay aligned, the bias rows in step)."""
    hi = d.rows if hi is None else hi
    assert lo % 64 == 0 and hi % 64 == 0 and lo % K == 0 and hi % K == 0
    with ops.gemm_mode("f16x3"):
        ops.linear128_ln_gelu_pack(d.x[lo:hi], d.sx[lo:hi], d.fw, d.g1[lo // K:hi // K], K, d.gamma, d.beta, eps, bound, d.out[lo:hi], d.rs[lo:hi])


def _result(d):
    """(out as int32 [rows, 512], out_scale) of a placed run, after checking everything around them."""
    torch.cuda.synchronize()
    assert PC.guards_intact(d), "a write outside out[:, :512] or out_scale"
    return d.out.contiguous().view(torch.int32).clone(), d.rs.clone()


def _go(ops, c, K=None, bound=None, **kw):
    d = PC.place(c, **kw)
    _launch(ops, d, c["rowgroup"] if K is None else K, c["bound"] if bound is None else bound)
    return _result(d)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


# ---- bit for bit

def test_cpu_packing_yields_the_devices_containers_and_scales(ops):
    """What every other test here rests on: g8_reference packs the operands as ops.scale_pack_rows_g8 and ops.F16Weight do."""
    c = PC.build("plain")
    xp, sx = ops.scale_pack_rows_g8(c["x"].cuda())
    fw = ops.F16Weight(c["W"].cuda().contiguous())
    assert torch.equal(xp.view(torch.int32).cpu(), c["xp"]) and torch.equal(sx.cpu(), c["sx"])
    assert torch.equal(fw.packed.view(torch.int32).cpu(), c["wp"]) and torch.equal(fw.scale.cpu(), c["sw"])


LDS = dict(ldx=160, ldw=136, ldrb=528, ldo=520)


@pytest.mark.parametrize("which", ["all four", "ldx", "ldw", "ldrb", "ldo"])
def test_leading_dimensions_change_no_bit(ops, which):
    """Views into wider buffers, the inputs' padding columns NaN, out's the guard word: the same bits as contiguous, the padding untouched."""
    c = PC.build("plain")
    kw = LDS if which == "all four" else {which: LDS[which]}
    assert _same(_go(ops, c, **kw), _go(ops, c))


@pytest.mark.parametrize("G", [64, 96, 128, 160, 256])
def test_rowgroup_equals_its_bias_rows_repeated_per_32_rows(ops, G):
    c = PC.build(f"rowgroup {G}")
    assert c["rowgroup"] == G and c["rows"] // 64 >= 3
    c32 = dict(c, rowgroup=32, g1=c["g1"].repeat_interleave(G // 32, dim=0))
    got = _go(ops, c)
    assert _same(got, _go(ops, c32))
    # Both of those runs index a bias row per 32-row tile, and a kernel that took the block's first tile for both would get both wrong alike.  One
    # launch per bias row, with that row for ALL rows (rowgroup = rows: there is no index to compute), gives the rows of its group the same bits.
    for g in range(c["rows"] // G):
        one = _go(ops, dict(c, rowgroup=c["rows"], g1=c["g1"][g:g + 1]))
        assert torch.equal(one[0][g * G:(g + 1) * G], got[0][g * G:(g + 1) * G]), g


def test_rows_permute_with_their_inputs(ops):
    c = PC.build("one bias row")
    perm = c["perm"]
    out, rs = _go(ops, c)
    outp, rsp = _go(ops, dict(c, xp=c["xp"][perm], sx=c["sx"][perm]))
    assert torch.equal(outp, out[perm.cuda()]) and torch.equal(rsp, rs)


def test_a_non_finite_row_stays_alone(ops):
    c = PC.build("one bias row")
    out, rs = _go(ops, c)
    outn, rsn = _go(ops, PC.with_nan_row(c))
    keep = torch.arange(c["rows"], device="cuda") != PC.NAN_ROW
    assert torch.equal(outn[keep], out[keep]) and torch.equal(rsn, rs)


@pytest.mark.parametrize("which", ["1", "2", "3", "2C", "2C+1", "4C+1"])
def test_trips_equal_single_trip_launches_on_slices(ops, which):
    """The grid is min(nblocks, 2 C): 2 C blocks is the last single-trip launch, 2 C + 1 sends one workgroup on a second trip, 4 C + 1 one on a third
    (stage 0 and bias slot 0 again).  Launches on consecutive slices of at most C blocks are single-trip by construction."""
    C = _cus()
    nblocks = {"1": 1, "2": 2, "3": 3, "2C": 2 * C, "2C+1": 2 * C + 1, "4C+1": 4 * C + 1}[which]
    c = PC.head(_trip_pool(), nblocks)
    whole = _go(ops, c)
    steps = [C, 1] if nblocks == 3 else [C]
    for step in steps:
        d = PC.place(c)
        for b in range(0, nblocks, step):
            _launch(ops, d, 64, c["bound"], lo=64 * b, hi=64 * min(b + step, nblocks))
        assert _same(_result(d), whole), step


def test_guards_around_out_and_out_scale_survive_192_rows(ops):
    c = PC.build("rowgroup 96")
    d = PC.place(c)
    before = d.out_buf.clone()
    _launch(ops, d, c["rowgroup"], c["bound"])
    torch.cuda.synchronize()
    assert PC.guards_intact(d)
    # and the run did write: no output word is the guard word any more
    assert not bool((d.out.contiguous().view(torch.int32) == PC.GUARD_WORD).any()) and not torch.equal(before, d.out_buf)
    assert bool((d.rs > 0).all())


def test_small_operands_in_one_nan_arena_change_no_bit(ops):
    """x_scale, g1, gamma, beta and w_scale inside one NaN-filled arena: a read one element past any of them would be a NaN."""
    c = PC.build("rowgroup 96")
    a, b = _go(ops, c, arena=True), _go(ops, c)
    assert _same(a, b)
    assert torch.isfinite(unpack_g8(a[0], a[1], H1)).all()


def test_scale_is_the_bounds_power_of_two(ops):
    c = PC.build("plain")
    assert c["bound"] < 30.0
    below = float(torch.nextafter(torch.tensor(32.0), torch.tensor(0.0)))      # in fp32, what the entry takes
    assert below == 32.0 - 2.0 ** -19
    bounds = [below, 32.0, 33.0]
    runs = [_go(ops, c, bound=b) for b in bounds]
    for (out, rs), s in zip(runs, (2.0 ** 10, 2.0 ** 9, 2.0 ** 9)):
        assert torch.equal(rs, torch.full_like(rs, s))
    assert _same(runs[1], runs[2])      # the bound enters through the scale alone
    # the g8 format's resolution at the coarser scale: the hi + lo split's 2^-22 relative to the bound
    dec = [unpack_g8(out, rs, H1) for out, rs in runs]
    assert float((dec[0] - dec[1]).abs().max()) <= 2.0 ** -22 * 32.0


# ---- against fp64

def _pair(ops, c):
    """The two launches the kernel replaces, on the same bits.  ops.linear takes packed rows from 256 rows up: a smaller case is repeated to that many
    (whole groups, so every row keeps its bias row) and its first copy kept -- the GEMM and the LayerNorm treat every row on its own."""
    rows, K = c["rows"], c["rowgroup"]
    reps = -(-256 // rows)
    xp = c["xp"].repeat(reps, 1).cuda().view(torch.float32)
    sx, g1 = c["sx"].repeat(reps).cuda(), c["g1"].repeat(reps, 1).cuda()
    fw = ops.F16Weight(c["W"].cuda().contiguous())
    assert torch.equal(fw.packed.view(torch.int32).cpu(), c["wp"]) and torch.equal(fw.scale.cpu(), c["sw"])
    with ops.gemm_mode("f16x3"):
        h = ops.linear(xp, fw, None, rowbias=g1, rowgroup=K, x_scale=sx, x_packed=True)
        rs = torch.empty(rows * reps, dtype=torch.float32, device="cuda")
        out = ops.layernorm(h, c["gamma"].cuda(), c["beta"].cuda(), EPS, act=ops.ACT_GELU, out=torch.empty_like(h), scale_out=rs, pack=True)
    return unpack_g8(out.view(torch.int32), rs, H1)[:rows]


def _errors(ops, c):
    out, rs = _go(ops, c)
    got = unpack_g8(out, rs, H1)
    assert torch.isfinite(got).all()
    # one scale for every row: the power of two that puts the a-priori bound into [2^14, 2^15)
    assert torch.equal(rs, torch.full_like(rs, 2.0 ** (14 - math.floor(math.log2(c["bound"])))))
    want = c["want"].cuda()
    return got, (got - want).abs(), (_pair(ops, c) - want).abs()


def _line(name, c, err, err_pair):
    print(f"\n| {name} | {c['rows']} | {c['rowgroup']} | {err:.3e} | {err_pair:.3e} | {err / err_pair:.2f} |")


@pytest.mark.parametrize("name", ["one block", "rowgroup 96", "rowgroup 160", "variance near eps", "row magnitudes"])
def test_error_against_fp64_within_twice_the_two_launch_sequence(ops, name):
    c = PC.build(name)
    got, e, e_pair = _errors(ops, c)
    err, err_pair = float(e.max()), float(e_pair.max())
    _line(name, c, err, err_pair)
    assert err <= 2.0 * err_pair, (err, err_pair)
    if name == "variance near eps":
        # eps is half of what is under the square root here: the result without it is far away
        no_eps, _ = PC.reference(c["xp"], c["sx"], c["wp"], c["sw"], c["g1"], c["rowgroup"], c["gamma"], c["beta"], eps=0.0)
        away = float((got - no_eps.cuda()).abs().max())
        print(f"  (from the fp64 result without eps: {away:.3e})")
        assert away > 100.0 * err, (away, err)


def test_gamma_outlier_column_and_the_other_511_each_within_twice(ops):
    """gamma[13] is 50 x the rest and sets the maximum error of kernel and pair alike: the bar is held on column 13 and on the others separately."""
    c = PC.build("gamma outlier")
    got, e, e_pair = _errors(ops, c)
    others = torch.arange(H1, device="cuda") != 13
    for label, cols in (("column 13", ~others), ("the other 511 columns", others)):
        err, err_pair = float(e[:, cols].max()), float(e_pair[:, cols].max())
        _line(f"gamma outlier, {label}", c, err, err_pair)
        assert err <= 2.0 * err_pair, (label, err, err_pair)
    # the block of zero rows under a zero bias row: gelu(beta) to the formats' precision, as in test_gpu_patch_rowln.py
    assert float((got[:64] - PC.gelu64(c["beta"].double().cuda())[None]).abs().max()) <= 4 * 2.0 ** -24 + 2.0 ** -22
