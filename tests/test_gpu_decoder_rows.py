"""The decoder's small-row kernels where their loops take a second trip: the second half of csrc/gemm.hip (linear_skinny, linear_skinny_multi,
linear_rows_multi<FULL>, linear_skinny_ln, linear_ln256) and the end of csrc/rowops.hip (mlp3, mlp3_pair, sum_planes), at the sizes of
tests/decoder_sizes.py (derived from the sources; tests/test_decoder_rows_cpu.py keeps the lists equal to the constants), plus the prompt encodings
pos_l1 and fourier_pe.  Every kernel of the family is run
  (a) on integer-valued fp32 inputs whose every partial sum is exact in fp32 (sum |terms| < 2**24, asserted on the CPU): the result must be
      torch.equal to the fp64 reference in ANY summation order -- a swapped k-slot, a dropped round or a chunk read twice cannot hide in a tolerance;
  (b) on random-normal inputs against fp64 at the tolerance the kernel's test in test_gpu_kernels.py uses;
  (c) into views of wider sentinel-filled buffers (ldy > N, rows after M) that must keep every sentinel, from column slices of wider buffers whose
      other cells are NaN (ldx, ldw > K): a load outside [0, K) of a row shows as NaN;
  (d) with inf in x[r, 0] at a K with a ragged last round (the padded k-slots re-read slot 0 against a zeroed weight): every other row keeps its bits,
      row r is non-finite wherever the reference is."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import decoder_sizes as DS

pytestmark = pytest.mark.gpu

SENT = -54321.0
LIMIT = float(2 ** 24)
EXACT_MAX = {}      # kernel -> largest sum |terms| its exact cases reached (printed by the last test)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd import ops as _ops
    _ops._lib.load()
    return _ops


def cu(t):
    return None if t is None else t.cuda().contiguous()


def _close(got, want, atol, rtol=0.0, what=""):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = (got - want).abs()
    bad = ~(err <= atol + rtol * want.abs())      # (a NaN is a mismatch)
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} mismatches, max abs err {err.max():.3e} (max |want| {want.abs().max():.3e})"


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def guarded(rows, cols, left=4, right=4, top=1, bottom=2):
    """A [rows, cols] view into a sentinel-filled [top + rows + bottom, left + cols + right] buffer -> (buffer, view)."""
    buf = torch.full((top + rows + bottom, left + cols + right), SENT, device="cuda")
    return buf, buf[top:top + rows, left:left + cols]


def guards_kept(buf, view):
    """Every cell of buf outside view still holds the sentinel."""
    off = (view.data_ptr() - buf.data_ptr()) // 4
    top, left = off // buf.stride(0), off % buf.stride(0)
    c = buf.clone()
    c[top:top + view.shape[0], left:left + view.shape[1]] = SENT
    return bool((c == SENT).all())


def sliced(t, left=16, right=12):
    """t [rows, K] (CPU) as a column slice of a wider GPU buffer whose other cells are NaN; the slice starts 16-byte aligned and ld % 4 == 0."""
    if t is None:
        return None
    rows, K = t.shape
    buf = torch.full((rows, left + K + right), float("nan"))
    buf[:, left:left + K] = t
    return buf.cuda()[:, left:left + K]


def rnd(g, *shape, ints=None):
    if ints is None:
        return torch.randn(*shape, generator=g)
    return torch.randint(-ints, ints + 1, shape, generator=g).float()


def act_ref(y, act):
    return F.gelu(y) if act == 1 else (F.relu(y) if act == 2 else y)


def ref_linear(x, W, b=None, r=None, act=0):
    y = act_ref(F.linear(x.double(), W.double(), None if b is None else b.double()), act)
    return y if r is None else y + r.double()


def exact_bound(what, x, W, b=None, r=None):
    """sum_k |x_k w_k| + |b| + |r| per output, asserted below 2**24: every partial sum of integer-valued inputs is then an integer fp32 holds exactly."""
    s = x.abs().double() @ W.abs().double().T
    if b is not None:
        s = s + b.abs().double()
    if r is not None:
        s = s + r.abs().double()
    m = float(s.max())
    for t in (x, W, b, r):
        assert t is None or torch.equal(t, t.round())
    assert m < LIMIT, (what, m)
    EXACT_MAX[what] = max(EXACT_MAX.get(what, 0.0), m)
    return m


def operands(g, M, N, K, ints, bias=True, res=True):
    """x, W, b, r on the CPU: integers in [-8, 8] / [-64, 64], or random normal with W scaled by K ** -0.5."""
    if ints:
        return rnd(g, M, K, ints=8), rnd(g, N, K, ints=8), rnd(g, N, ints=64) if bias else None, rnd(g, M, N, ints=64) if res else None
    return rnd(g, M, K), rnd(g, N, K) / K ** 0.5, rnd(g, N) if bias else None, rnd(g, M, N) if res else None


def isolation(run, ref, x, r):
    """(d): run(x_gpu_slice) -> [M, N]; ref(x_cpu) -> fp64.  inf in x[r, 0]: the other rows keep their bits, row r is non-finite wherever ref is."""
    base = run(sliced(x))
    x2 = x.clone()
    x2[r, 0] = float("inf")
    got = run(sliced(x2))
    others = [i for i in range(x.shape[0]) if i != r]
    assert same_bits(got[others], base[others]), "a non-finite row leaked into its neighbours"
    assert torch.isfinite(base).all()
    nf = ~torch.isfinite(ref(x2)[r])
    assert nf.any()
    assert not torch.isfinite(got[r].cpu())[nf].any(), f"row {r}: finite where the reference is not ({int(torch.isfinite(got[r].cpu())[nf].sum())} of {int(nf.sum())})"


# ------------------------------------------------------------------------------------------------ psam_linear_skinny
def skinny(ops, x, W, b, r, y, act):
    M, K = x.shape
    ops._lib.check(ops._lib.load().psam_linear_skinny(x.data_ptr(), x.stride(0), W.data_ptr(), W.stride(0), ops._p(b), ops._p(r), 0 if r is None else r.stride(0),
                                                      y.data_ptr(), y.stride(0), M, W.shape[0], K, act, ops._stream()), "psam_linear_skinny")
    return y


SKINNY_M = (1, 16, 17, 48, 49, 64)
SKINNY_N = (1, 15, 16, 17, 250)
SKINNY_CASES = [(1, 1, 16, 0, False, False), (16, 16, 128, 0, True, True), (17, 15, 144, 2, True, True), (48, 17, 112, 1, True, False),
                (49, 250, 272, 0, True, True), (64, 250, 128, 2, False, True), (17, 17, 272, 1, False, True), (49, 15, 16, 2, True, False),
                (1, 250, 144, 0, False, False), (64, 1, 112, 0, True, True), (33, 17, 272, 2, True, True), (17, 250, 112, 0, True, True)]


@pytest.mark.parametrize("M,N,K,act,bias,res", SKINNY_CASES)
def test_linear_skinny(ops, M, N, K, act, bias, res):
    g = torch.Generator().manual_seed(M * 1000 + N * 10 + K)

    def run(xs, W, b, r, a):
        buf, y = guarded(M, N, left=3, right=4)      # a row stride that is no multiple of 4: the kernel stores scalars
        rb = None
        if r is not None:
            rb = guarded(M, N, left=1, right=2)[1]
            rb.copy_(r)
        skinny(ops, xs, sliced(W, left=4), cu(b), rb, y, a)
        assert guards_kept(buf, y)
        return y.clone()

    if act != 1:      # (a)
        x, W, b, r = operands(g, M, N, K, True, bias, res)
        exact_bound("linear_skinny", x, W, b, r)
        assert torch.equal(run(sliced(x), W, b, r, act).cpu(), ref_linear(x, W, b, r, act).float())
    x, W, b, r = operands(g, M, N, K, False, bias, res)      # (b), (c)
    _close(run(sliced(x), W, b, r, act), ref_linear(x, W, b, r, act), 1e-5, rtol=1e-5, what="linear_skinny")
    if K % 128:      # (d)
        isolation(lambda xs: run(xs, W, b, r, act), lambda xc: ref_linear(xc, W, b, r, act), x, M // 2)


# ------------------------------------------------------------------------------------------------ psam_linear_skinny_multi / psam_linear_rows_multi
MULTI_N = (16, 250, 40, 1, 17, 33)
MULTI_ACT = (0, 2, 1, 0, 2, 1)


def make_jobs(g, K, Ns, acts, ints, add_rows):
    """Per job: W, bias (None on job 1), xadd (even jobs; [add_rows, K]) on the CPU, and act."""
    jobs = []
    for i, (N, act) in enumerate(zip(Ns, acts)):
        W = rnd(g, N, K, ints=8) if ints else rnd(g, N, K) / K ** 0.5
        b = None if i == 1 else (rnd(g, N, ints=64) if ints else rnd(g, N))
        xadd = (rnd(g, add_rows, K, ints=8) if ints else rnd(g, add_rows, K)) if i % 2 == 0 else None
        jobs.append((W, b, xadd, act))
    return jobs


def gpu_jobs(jobs):
    """The jobs on the GPU, the weights rows of one wider buffer and the addends column slices of equally wide ones (shared ldw, ldxadd)."""
    K = jobs[0][0].shape[1]
    Wall = sliced(torch.cat([j[0] for j in jobs]), left=4)
    out, n0 = [], 0
    for W, b, xadd, act in jobs:
        out.append((Wall[n0:n0 + W.shape[0]], cu(b), sliced(xadd, left=8, right=8), act))
        n0 += W.shape[0]
    assert all(j[0].data_ptr() % 16 == 0 for j in out) and Wall.stride(0) > K
    return out


def launch_multi(fn, xs, jobs, **kw):
    M = xs.shape[0]
    bufs = [guarded(M, j[0].shape[0], left=3, right=2) for j in jobs]
    ys = fn(xs, gpu_jobs(jobs), outs=[v for _, v in bufs], **kw)
    for (buf, v), y in zip(bufs, ys):
        assert y.data_ptr() == v.data_ptr() and guards_kept(buf, v)
    return [y.clone() for y in ys]


@pytest.mark.parametrize("M,K,njobs", [(1, 16, 1), (17, 144, 3), (64, 256, DS.constants()["MAX_JOBS"]), (64, 144, 3), (17, 16, DS.constants()["MAX_JOBS"]), (1, 256, 3)])
def test_linear_skinny_multi(ops, M, K, njobs):
    """Up to PSAM_SKINNY_MAX_JOBS Linears of different N in one launch (the shorter jobs' last workgroups return early), xadd on the even jobs, no bias on
    job 1: exact, against fp64, guarded, and per job the bits of psam_linear_skinny on the pre-added input."""
    assert njobs in (1, 3, 6) and len(ops._lib.SkinnyJobs().job) == 6
    g = torch.Generator().manual_seed(M * 100 + K + njobs)
    Ns, acts = MULTI_N[:njobs], MULTI_ACT[:njobs]
    x = rnd(g, M, K, ints=8)      # (a)
    jobs = make_jobs(g, K, Ns, [0 if a == 1 else a for a in acts], True, M)
    got = launch_multi(ops.linear_skinny_multi, sliced(x), jobs)
    for i, (W, b, xadd, act) in enumerate(jobs):
        xin = x if xadd is None else x + xadd
        exact_bound("linear_skinny_multi", xin, W, b)
        assert torch.equal(got[i].cpu(), ref_linear(xin, W, b, None, act).float()), i
    x = rnd(g, M, K)      # (b), (c), and the promise of the kernel's comment
    jobs = make_jobs(g, K, Ns, acts, False, M)
    got = launch_multi(ops.linear_skinny_multi, sliced(x), jobs)
    for i, (W, b, xadd, act) in enumerate(jobs):
        xin = x if xadd is None else x + xadd      # one fp32 add, as the kernel makes it
        _close(got[i], ref_linear(xin, W, b, None, act), 1e-5, rtol=1e-5, what=f"linear_skinny_multi job {i}")
        one = skinny(ops, sliced(xin), sliced(W, left=4), cu(b), None, torch.empty(M, W.shape[0], device="cuda"), act)
        assert same_bits(got[i], one), f"job {i} differs from psam_linear_skinny on the pre-added input"
    if K % 128:      # (d): every job at once
        run = lambda xs: torch.cat(launch_multi(ops.linear_skinny_multi, xs, jobs), 1)
        ref = lambda xc: torch.cat([ref_linear(xc if xadd is None else xc + xadd, W, b, None, act) for W, b, xadd, act in jobs], 1)
        isolation(run, ref, x, M - 1)
    with pytest.raises(ops._lib.PointSamHipError):
        ops.linear_skinny_multi(torch.zeros(65, K, device="cuda"), [(torch.zeros(16, K, device="cuda"), None, None, 0)])      # M > 64


ROWS_N = (1, 16, 17, 33, 100)
ROWS_ACT = (0, 2, 1, 0, 2)
ROWS_CASES = [(1, 1, 1, 16), (31, 31, 1, 112), (32, 16, 1, 128), (33, 11, 3, 144), (231, 77, 1, 272), (231, 77, 3, 128), (33, 11, 1, 272)]


def rows_ref(x, jobs, rps, rep):
    M, K = x.shape
    Z = M // rps
    out = []
    for W, b, xadd, act in jobs:
        xin = x if xadd is None else (x.view(Z // rep, rep, rps, K) + xadd.view(Z // rep, 1, rps, K)).reshape(M, K)
        out.append((xin, ref_linear(xin, W, b, None, act)))
    return out


@pytest.mark.parametrize("M,rps,rep,K", ROWS_CASES)
def test_linear_rows_multi(ops, M, rps, rep, K):
    """Both instances of linear_rows_multi_kernel (K % 128 == 0 or not) with five jobs of different N in one launch and the addend broadcast over `rep`
    row sets."""
    g = torch.Generator().manual_seed(M * 10 + K + rep)
    sets = M // rps // rep
    kw = dict(xadd_rows_per_set=rps, xadd_rep=rep)
    x = rnd(g, M, K, ints=8)      # (a)
    jobs = make_jobs(g, K, ROWS_N, [0 if a == 1 else a for a in ROWS_ACT], True, sets * rps)
    got = launch_multi(ops.linear_rows_multi, sliced(x), jobs, **kw)
    for i, ((xin, want), (W, b, _, _)) in enumerate(zip(rows_ref(x, jobs, rps, rep), jobs)):
        exact_bound("linear_rows_multi", xin, W, b)
        assert torch.equal(got[i].cpu(), want.float()), i
    x = rnd(g, M, K)      # (b), (c)
    jobs = make_jobs(g, K, ROWS_N, ROWS_ACT, False, sets * rps)
    got = launch_multi(ops.linear_rows_multi, sliced(x), jobs, **kw)
    for i, (_, want) in enumerate(rows_ref(x, jobs, rps, rep)):
        _close(got[i], want, 1e-5, rtol=1e-5, what=f"linear_rows_multi job {i}")
    if K % 128 == 0:      # the two instances agree bit for bit: 16 more columns of zeros turn a <true> problem into a <false> one
        pad = lambda t: None if t is None else torch.cat([t, torch.zeros(t.shape[0], 16)], 1)
        again = launch_multi(ops.linear_rows_multi, sliced(pad(x)), [(pad(W), b, pad(xadd), act) for W, b, xadd, act in jobs], **kw)
        for i, (full, ragged) in enumerate(zip(got, again)):
            assert same_bits(full, ragged), f"job {i}: linear_rows_multi_kernel<true> and <false> differ"
    else:      # (d)
        run = lambda xs: torch.cat(launch_multi(ops.linear_rows_multi, xs, jobs, **kw), 1)
        ref = lambda xc: torch.cat([w for _, w in rows_ref(xc, jobs, rps, rep)], 1)
        isolation(run, ref, x, M // 2)


# ------------------------------------------------------------------------------------------------ psam_linear_skinny_ln / psam_linear_ln256
def ln_operands(g, M, K, ints):
    x, W, b, r = operands(g, M, 256, K, ints)
    return x, W, b, r, 1.0 + 0.1 * rnd(g, 256), 0.1 * rnd(g, 256)


def ref_ln(x, W, b, r, lw, lb, eps=1e-6):
    return F.layer_norm(ref_linear(x, W, b, r), (256,), lw.double(), lb.double(), eps)


def skinny_ln(ops, x, W, b, r, lw, lb, y, counters, K=None, eps=1e-6):
    """One launch with `tmp` of exactly psam_linear_skinny_ln_tmp_floats floats between sentinels; the PSAM_CNT_ROW word must read zero afterwards."""
    L = ops._lib.load()
    M = x.shape[0]
    K = x.shape[1] if K is None else K
    n = L.psam_linear_skinny_ln_tmp_floats(M, K)
    assert n == DS.ln_split(DS.constants(), K)[0] * M * 256
    tbuf = torch.full((n + 64,), SENT, device="cuda")
    tmp = tbuf[32:32 + n]
    ops._lib.check(L.psam_linear_skinny_ln(x.data_ptr(), x.stride(0), W.data_ptr(), W.stride(0), ops._p(b), ops._p(r), 0 if r is None else r.stride(0), lw.data_ptr(),
                                           lb.data_ptr(), eps, tmp.data_ptr(), y.data_ptr(), y.stride(0), M, 256, K, counters.data_ptr(), ops._stream()),
                   "psam_linear_skinny_ln")
    assert (tbuf[:32] == SENT).all() and (tbuf[32 + n:] == SENT).all(), "linear_skinny_ln wrote outside its scratch"
    assert not counters.any(), "the arrival counter is not back at zero"
    return y


SKINNY_LN_M = (1, 3, 4, 5, 16, 17, 64)
SKINNY_LN_CASES = [(1, 16), (3, 112), (4, 128), (5, 144), (16, 272), (17, 528), (64, 2048), (5, 2064), (17, 4096), (64, 4096), (3, 2064)]


@pytest.mark.parametrize("M,K", SKINNY_LN_CASES)
def test_linear_skinny_ln(ops, M, K):
    g = torch.Generator().manual_seed(M * 7 + K)
    counters = ops.new_counters("cuda")

    def run(xs, W, b, r, lw, lb, inplace=False):
        buf, y = guarded(M, 256)
        rs = sliced(r, left=4, right=8)
        if inplace:
            y.copy_(rs)
            rs = y
        skinny_ln(ops, xs, sliced(W, left=4), cu(b), rs, cu(lw), cu(lb), y, counters)
        assert guards_kept(buf, y)
        return y.clone()

    x, W, b, r, lw, lb = ln_operands(g, M, K, False)      # (b), (c)
    got = run(sliced(x), W, b, r, lw, lb)
    _close(got, ref_ln(x, W, b, r, lw, lb), 2e-5, what="linear_skinny_ln vs fp64")
    if K <= 256:      # one K range: the products and the order of linear_skinny
        two = ops.layernorm(ops.linear(cu(x), cu(W), cu(b)), cu(lw), cu(lb), 1e-6, residual=cu(r))
        _close(got, two, 2e-6, what="linear_skinny_ln vs two launches")
    assert same_bits(run(sliced(x), W, b, r, lw, lb, inplace=True), got), "in place on the residual"
    for rep in range(5):      # the counter is never reset between these
        assert same_bits(run(sliced(x), W, b, r, lw, lb), got), rep
    xi, Wi, bi, ri, _, _ = ln_operands(g, M, K, True)      # integers: the sums before the LayerNorm are exact whatever the split
    exact_bound("linear_skinny_ln", xi, Wi, bi, ri)
    goti = run(sliced(xi), Wi, bi, ri, lw, lb)
    two = ops.layernorm(ops.linear(cu(xi), cu(Wi), cu(bi)), cu(lw), cu(lb), 1e-6, residual=cu(ri))
    assert torch.equal(ops.linear(cu(xi), cu(Wi), cu(bi), residual=cu(ri)).cpu(), ref_linear(xi, Wi, bi, ri).float())
    _close(goti, two, 2e-6, what="linear_skinny_ln on integers vs linear + layernorm")
    _close(goti, ref_ln(xi, Wi, bi, ri, lw, lb), 2e-5, what="linear_skinny_ln on integers vs fp64")
    if K % 128:      # (d)
        isolation(lambda xs: run(xs, W, b, r, lw, lb), lambda xc: ref_ln(xc, W, b, r, lw, lb), x, M // 2)


LN256_CASES = [(1, 16), (15, 112), (16, 128), (17, 144), (33, 272), (33, 512), (1, 272), (17, 512)]


def ln256(ops, x, W, b, r, lw, lb, y, K=None, eps=1e-6):
    ops._lib.check(ops._lib.load().psam_linear_ln256(x.data_ptr(), x.stride(0), W.data_ptr(), W.stride(0), ops._p(b), ops._p(r), 0 if r is None else r.stride(0),
                                                     lw.data_ptr(), lb.data_ptr(), eps, y.data_ptr(), y.stride(0), x.shape[0], 256, x.shape[1] if K is None else K,
                                                     ops._stream()), "psam_linear_ln256")
    return y


@pytest.mark.parametrize("M,K", LN256_CASES)
def test_linear_ln256(ops, M, K):
    g = torch.Generator().manual_seed(M * 11 + K)

    def run(xs, W, b, r, lw, lb, inplace=False):
        buf, y = guarded(M, 256)
        rs = sliced(r, left=4, right=8)
        if inplace:
            y.copy_(rs)
            rs = y
        ln256(ops, xs, sliced(W, left=4), cu(b), rs, cu(lw), cu(lb), y)
        assert guards_kept(buf, y)
        return y.clone()

    x, W, b, r, lw, lb = ln_operands(g, M, K, False)      # (b), (c)
    got = run(sliced(x), W, b, r, lw, lb)
    _close(got, ref_ln(x, W, b, r, lw, lb), 2e-5, what="linear_ln256 vs fp64")
    assert same_bits(run(sliced(x), W, b, r, lw, lb, inplace=True), got), "in place on the residual"
    xi, Wi, bi, ri, _, _ = ln_operands(g, M, K, True)
    exact_bound("linear_ln256", xi, Wi, bi, ri)
    goti = run(sliced(xi), Wi, bi, ri, lw, lb)
    two = ops.layernorm(ops.linear(cu(xi), cu(Wi), cu(bi)), cu(lw), cu(lb), 1e-6, residual=cu(ri))
    _close(goti, two, 2e-6, what="linear_ln256 on integers vs linear + layernorm")
    _close(goti, ref_ln(xi, Wi, bi, ri, lw, lb), 2e-5, what="linear_ln256 on integers vs fp64")
    if K % 128:      # (d)
        isolation(lambda xs: run(xs, W, b, r, lw, lb), lambda xc: ref_ln(xc, W, b, r, lw, lb), x, M // 2)


def test_linear_ln256_refuses_a_long_k(ops):
    c = DS.constants()
    K = c["LN256_MAX_K"] + 16
    assert K == 528
    x, W = torch.zeros(4, K, device="cuda"), torch.zeros(256, K, device="cuda")
    v, y = torch.zeros(256, device="cuda"), torch.full((4, 256), SENT, device="cuda")
    with pytest.raises(ops._lib.PointSamHipError):
        ln256(ops, x, W, None, None, v, v, y)
    ln256(ops, x, W, None, None, v, v, y, K=K - 16)      # (the same buffers are fine one slot shorter)
    assert (y == 0).all()


# ------------------------------------------------------------------------------------------------ psam_mlp3 / psam_mlp3_pair
MLP3_CASES = [(4, 4, 1, 1, 1), (252, 256, 15, 3, 1), (256, 252, 16, 1, 3), (260, 516, 17, 3, 3), (516, 260, 255, 1, 1), (1024, 1024, 300, 1, 3),
              (260, 1024, 257, 3, 1), (4, 516, 300, 1, 1)]


def mlp3_layers(g, M, din, dh, dout, ints):
    if ints:
        return [[(rnd(g, o, i, ints=1), rnd(g, o, ints=3)) for i, o in ((din, dh), (dh, dh), (dh, dout))] for _ in range(M)]
    return [[(rnd(g, o, i) / i ** 0.5, rnd(g, o) * 0.1) for i, o in ((din, dh), (dh, dh), (dh, dout))] for _ in range(M)]


def mlp3_ref(x, layers, what=None):
    """x [Z, M, din] -> fp64 [Z, M, dout]; what: assert the exactness bound of every layer under that name."""
    out = []
    for m, mlp in enumerate(layers):
        h = x[:, m].double()
        for li, (W, b) in enumerate(mlp):
            if what:
                exact_bound(what, h.float(), W, b)
            h = F.linear(h, W.double(), b.double())
            if li < 2:
                h = F.relu(h)
        out.append(h)
    return torch.stack(out, 1)


def mlp3_buffers(x, M, dout):
    """x [Z, M, din] at row stride ldx > M * sx, sx = din + 1, between NaNs; the output rows at so = dout + 3, ldo = M * so + 5 between sentinels."""
    Z, _, din = x.shape
    sx = din + 1
    xb = torch.full((Z, M * sx + 7), float("nan"))
    for m in range(M):
        xb[:, m * sx:m * sx + din] = x[:, m]
    so = dout + 3
    ob = torch.full((Z + 1, M * so + 5), SENT, device="cuda")
    return xb.cuda(), sx, ob, so


def mlp3_result(ob, Z, M, dout, so):
    """The [Z, M, dout] outputs of the buffer, after checking every other cell kept its sentinel."""
    got = torch.stack([ob[:Z, m * so:m * so + dout] for m in range(M)], 1).clone()
    c = ob.clone()
    for m in range(M):
        c[:Z, m * so:m * so + dout] = SENT
    assert (c == SENT).all(), "mlp3 wrote outside its output rows"
    return got


@pytest.mark.parametrize("din,dh,dout,Z,M", MLP3_CASES)
def test_mlp3(ops, din, dh, dout, Z, M):
    g = torch.Generator().manual_seed(din + dh * 3 + dout)
    for ints in (True, False):
        x = rnd(g, Z, M, din, ints=1) if ints else rnd(g, Z, M, din)
        layers = mlp3_layers(g, M, din, dh, dout, ints)
        mw = ops.Mlp3Weights([[(cu(W), cu(b)) for W, b in mlp] for mlp in layers])
        xb, sx, ob, so = mlp3_buffers(x, M, dout)
        ops.mlp3(xb, xb.stride(0), sx, mw, ob, ob.stride(0), so, Z)
        got = mlp3_result(ob, Z, M, dout, so)
        if ints:      # fmaf chains over integers below 2**24: exact in any order
            assert torch.equal(got.cpu(), mlp3_ref(x, layers, "mlp3").float())
        else:
            _close(got, mlp3_ref(x, layers), 2e-6, what="mlp3")


def test_mlp3_pair_of_different_stacks(ops):
    """Stacks of different dimensions in one launch: the bits of two psam_mlp3 launches, and exact on integers."""
    g = torch.Generator().manual_seed(17)
    Z, (Ma, Mb), a, b = 3, (2, 1), (1024, 516, 17), (260, 256, 4)
    for ints in (True, False):
        xa, xb_ = (rnd(g, Z, M, d[0], ints=1) if ints else rnd(g, Z, M, d[0]) for M, d in ((Ma, a), (Mb, b)))
        la, lb = mlp3_layers(g, Ma, *a, ints), mlp3_layers(g, Mb, *b, ints)
        wa, wb = (ops.Mlp3Weights([[(cu(W), cu(v)) for W, v in mlp] for mlp in ls]) for ls in (la, lb))
        A, sxa, oa, soa = mlp3_buffers(xa, Ma, a[2])
        B, sxb, ob, sob = mlp3_buffers(xb_, Mb, b[2])
        ops.mlp3(A, A.stride(0), sxa, wa, oa, oa.stride(0), soa, Z)
        ops.mlp3(B, B.stride(0), sxb, wb, ob, ob.stride(0), sob, Z)
        one = mlp3_result(oa, Z, Ma, a[2], soa), mlp3_result(ob, Z, Mb, b[2], sob)
        oa.fill_(SENT), ob.fill_(SENT)
        ops.mlp3_pair(A, A.stride(0), sxa, wa, oa, oa.stride(0), soa, B, B.stride(0), sxb, wb, ob, ob.stride(0), sob, Z)
        two = mlp3_result(oa, Z, Ma, a[2], soa), mlp3_result(ob, Z, Mb, b[2], sob)
        assert same_bits(one[0], two[0]) and same_bits(one[1], two[1])
        if ints:
            assert torch.equal(two[0].cpu(), mlp3_ref(xa, la, "mlp3_pair").float()) and torch.equal(two[1].cpu(), mlp3_ref(xb_, lb, "mlp3_pair").float())
        else:
            _close(two[0], mlp3_ref(xa, la), 2e-6, what="mlp3_pair a")
            _close(two[1], mlp3_ref(xb_, lb), 2e-6, what="mlp3_pair b")


def test_mlp3_refusals(ops):
    """din > MLP3_MAXD, dh % 4 != 0 and a weight pointer 4 bytes off a 16-byte boundary are errors, in both entry points; nothing is written."""
    L, check, E = ops._lib.load(), ops._lib.check, ops._lib.PointSamHipError
    big = torch.zeros(1028 * 1028 + 8, device="cuda")
    out = torch.full((8,), SENT, device="cuda")
    p = big.data_ptr()

    def one(din, dh, w1=p, w2=p, w3=p):
        return check(L.psam_mlp3(p, din, din, w1, p, w2, p, w3, p, out.data_ptr(), 4, 4, 1, 1, din, dh, 4, ops._stream()), "psam_mlp3")

    def pair(din, dh, w1=p, w2=p, w3=p):
        good = ops._lib.Mlp3Args(p, p, p, p, p, p, p, out.data_ptr(), 256, 256, 4, 4, 1, 256, 256, 4)
        bad = ops._lib.Mlp3Args(p, w1, p, w2, p, w3, p, out.data_ptr() + 16, din, din, 4, 4, 1, din, dh, 4)
        for a, b in ((good, bad), (bad, good)):
            check(L.psam_mlp3_pair(ctypes.byref(a), ctypes.byref(b), 1, ops._stream()), "psam_mlp3_pair")

    for fn in (one, pair):
        for kw in (dict(din=1028, dh=256), dict(din=256, dh=258), dict(din=256, dh=256, w1=p + 4), dict(din=256, dh=256, w2=p + 4), dict(din=256, dh=256, w3=p + 4)):
            with pytest.raises(E):
                fn(**kw)
    assert (out == SENT).all()
    one(1024, 1024)      # (the limits themselves are fine)
    assert (out[:4] == 0).all() and (out[4:] == SENT).all()


# ------------------------------------------------------------------------------------------------ psam_sum_planes
@pytest.mark.parametrize("P", [1, 2, 5])
def test_sum_planes(ops, P):
    """out = ((p0 + p1) + p2) + ..: exact on integers, and on random planes the bits of that fixed-order fp32 sum; planes at a stride past `count`."""
    L, check = ops._lib.load(), ops._lib.check
    g = torch.Generator().manual_seed(P)
    for count in (4, 1020, 1024, 1028):
        pstride = count + 8
        for ints in (True, False):
            planes = rnd(g, P, count, ints=64) if ints else rnd(g, P, count)
            pb = torch.full((P, pstride), float("nan"))
            pb[:, :count] = planes
            pb = pb.cuda()
            ob = torch.full((count + 16,), SENT, device="cuda")
            out = ob[4:4 + count]
            check(L.psam_sum_planes(pb.data_ptr(), P, pstride, count, out.data_ptr(), ops._stream()), "psam_sum_planes")
            want = planes[0].clone()
            for q in range(1, P):
                want = want + planes[q]
            assert same_bits(out.cpu(), want), (count, ints)
            if ints:
                assert torch.equal(out.cpu(), planes.double().sum(0).float())
            assert (ob[:4] == SENT).all() and (ob[4 + count:] == SENT).all()
    with pytest.raises(ops._lib.PointSamHipError):
        check(L.psam_sum_planes(pb.data_ptr(), P, 8, 6, ob.data_ptr(), ops._stream()), "psam_sum_planes")
    assert (ob[:4] == SENT).all()


# ------------------------------------------------------------------------------------------------ prompt encodings
@pytest.mark.parametrize("rows", [1, 2, 3, 513])
def test_pos_l1(ops, rows):
    g = torch.Generator().manual_seed(rows)
    c, W, b = torch.rand(rows, 3, generator=g) * 2 - 1, rnd(g, 128, 3), rnd(g, 128)
    ob = torch.full((rows + 1, 128), SENT, device="cuda")
    ops.pos_l1(cu(c), cu(W), cu(b), out=ob)
    _close(ob[:rows], F.gelu(F.linear(c.double(), W.double(), b.double())), 1e-5, what="pos_l1")
    assert (ob[rows:] == SENT).all()


def fourier_ref(pts, Gm, lab, e0, e1):
    v = 2 * math.pi * (pts.double() @ Gm.double())
    pe = torch.cat([v.sin(), v.cos()], -1)
    if lab is not None:
        pe = pe + (lab == 0)[:, None] * e0.double() + (lab == 1)[:, None] * e1.double()
    return pe


@pytest.mark.parametrize("Z,P,Fq", [(1, 1, 1), (1, 3, 85), (2, 1, 128), (2, 2, 64), (257, 1, 1), (1, 1, 257)])
def test_fourier_pe(ops, Z, P, Fq):
    """rows * F of 1, 255, 256 and 257 threads; labels of {-1, 0, 1, 2} (-1 and 2 add no embedding); the rows placed behind two other tokens of each
    batch of a sentinel-filled token buffer."""
    assert Z * P * Fq in (1, 255, 256, 257)
    g = torch.Generator().manual_seed(Z * 1000 + P * 10 + Fq)
    rows, T, E = Z * P, P + 3, 2 * Fq
    pts, Gm = torch.rand(rows, 3, generator=g) * 2 - 1, rnd(g, 3, Fq)
    e0, e1 = rnd(g, 1, E), rnd(g, 1, E)
    lab = (torch.arange(rows) + int(torch.randint(0, 4, (1,), generator=g))) % 4 - 1      # every label occurs once rows >= 4
    tokens = torch.full((Z, T, E), SENT, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    for labels in (lab, None):
        tokens.fill_(SENT)
        ops.fourier_pe(cu(pts), cu(Gm), tokens.view(-1)[2 * E:], P, T * E, labels=cu(labels), emb0=cu(e0), emb1=cu(e1), flag=flag)
        _close(tokens[:, 2:2 + P].reshape(rows, E), fourier_ref(pts, Gm, labels, e0, e1), 3e-5, what="fourier_pe")
        assert (tokens[:, :2] == SENT).all() and (tokens[:, 2 + P:] == SENT).all() and flag.item() == 0
    if rows >= 4:
        assert set(lab.tolist()) == {-1, 0, 1, 2}


def test_fourier_pe_range_flag(ops):
    """The flag stays 0 for coordinates at +-1 and at the fp32 value of 1 + 1e-6, and is raised by the next fp32 value beyond, on every axis, either sign."""
    g = torch.Generator().manual_seed(3)
    Gm = rnd(g, 3, 8)
    hi = torch.tensor(1 + 1e-6, dtype=torch.float64).float()
    assert 1.0 < float(hi) < 1.000001 + 1e-7
    beyond = torch.nextafter(hi, torch.tensor(2.0))
    assert float(beyond) > float(hi)
    out = torch.empty(5, 16, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")

    def flagged(pts):
        flag.zero_()
        ops.fourier_pe(cu(pts), cu(Gm), out, 5, 0, flag=flag)
        return flag.item()

    base = torch.rand(5, 3, generator=g) * 2 - 1
    assert flagged(base) == 0
    for v in (1.0, float(hi)):
        for sgn in (1.0, -1.0):
            assert flagged(torch.full((5, 3), sgn * v)) == 0, (v, sgn)
    for row in (0, 4):
        for axis in range(3):
            for sgn in (1.0, -1.0):
                pts = base.clone()
                pts[row, axis] = sgn * beyond
                assert flagged(pts) == 1, (row, axis, sgn)
                pts[row, axis] = sgn * hi
                assert flagged(pts) == 0, (row, axis, sgn)


def test_exact_cases_stayed_below_2_pow_24(ops):
    """The largest sum |terms| the exact cases of this session reached, per kernel (asserted below 2**24 where it was computed)."""
    for k, v in sorted(EXACT_MAX.items()):
        print(f"exact cases of {k}: largest sum |terms| {v:.0f} = 2**24 / {LIMIT / v:.1f}")
        assert v < LIMIT
