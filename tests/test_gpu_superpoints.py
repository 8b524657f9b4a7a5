"""Normals, superpoints and mask snapping on the GPU (csrc/normals.hip, csrc/superpoints.hip, point_sam_amd/superpoints.py) against the plain numpy
reference in tests/superpoint_reference.py.  The scatter matrix is compared with exact Python integers -- equal to float(exact) bit for bit, also
where it rounds (the cases of tests/normal_cases.py) --, the normals with numpy.linalg.eigh of that matrix under the budget written at the check,
without an eigenvalue gap as an eigenvector of the smallest eigenvalue, and everything downstream of the normals -- labels, sizes, snapped bits --
by equality."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import normal_cases as NC
import region_reference as R
import scene_reference as SR
import superpoint_reference as SP

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd import ops
    return ops


def _np_words(t):
    return t.cpu().numpy().view(np.uint64)


def _dev_words(masks):
    return torch.from_numpy(SR.words(masks).view(np.int64)).cuda()


class Cloud:
    """A cloud, its reference graph and exact scatter matrices, and the device graph built by the code under test from the same points."""

    def __init__(self, xyz, h):
        from point_sam_amd import regions
        self.xyz, self.h = np.ascontiguousarray(xyz, dtype=f32), h
        self.ref = R.Graph(self.xyz, h)
        self.dxyz = torch.from_numpy(self.xyz).cuda()
        self.dev = regions.build_graph(self.dxyz, voxel_size=h)
        self.N, self.V = len(self.xyz), len(self.ref.keep_idx)
        assert np.array_equal(self.dev.inv.cpu().numpy(), self.ref.inv) and np.array_equal(self.dev.nbr.cpu().numpy(), self.ref.nbr)
        self._scatter = self._normals = self._device = None

    def scatter(self):
        if self._scatter is None:
            self._scatter = SP.scatter(self.xyz, self.ref.inv, self.ref.nbr)
        return self._scatter

    def normals(self):
        """The reference's eigenvectors, curvatures and eigenvalues in fp64 (eigh of the exact S), once."""
        if self._normals is None:
            count, _, S = self.scatter()
            self._normals = SP.eigen(count, S)
        return self._normals

    def device(self, ops):
        """The device's count, normal, curvature as numpy arrays, once: what the superpoint reference is fed."""
        if self._device is None:
            c, n, k, _ = ops.voxel_normals(self.dxyz, self.dev.inv, self.dev.nbr)
            self._device = (c, n, k, c.cpu().numpy(), n.cpu().numpy(), k.cpu().numpy())
        return self._device


_CLOUDS = {}


_plane = NC.plane


def _cloud(name):
    """Built once per session and never modified."""
    if name not in _CLOUDS:
        _CLOUDS[name] = Cloud(*NC.cloud_points(name))
    return _CLOUDS[name]


EXACT = ["box", "sphere", "uniform6000", "grid", "edge", "duplicates", "heavy", "small63", "small65", "small4"]


# ------------------------------------------------------------------------------------------------ 1. the scatter matrix
def _assert_scatter_is_the_rounded_integer(name, count, S, dcount, dS):
    """count is the reference's and every scatter entry IS float(exact), bit for bit.  The tolerance is zero by definition, not by measurement: the
    header promises one conversion of the exact integer, rounded to nearest even, and float(int) is that conversion."""
    assert np.array_equal(dcount.cpu().numpy(), count.astype(np.int32))
    got, want = dS.cpu().numpy(), SP.scatter_float(S)
    largest, above, rounded = NC.scatter_stats(S)
    print(f"{name}: V = {len(S)}, largest count {int(count.max())}, largest |S| = 2^{largest}, {above} of {6 * len(S)} entries above 64 bits, "
          f"{rounded} entries not representable")
    assert got.shape == want.shape and got.dtype == np.float64
    wrong = np.argwhere(got.view(np.int64) != want.view(np.int64))
    assert len(wrong) == 0, (name, len(wrong), [(int(v), int(k), S[v][k], float(got[v, k]).hex(), float(want[v, k]).hex()) for v, k in wrong[:4]])
    return largest, above, rounded


@pytest.mark.parametrize("name", EXACT)
def test_count_and_scatter_equal_the_exact_integers(ops, name):
    """count is the reference's and every scatter entry equals the exact integer: on these clouds every entry has at most 53 bits (kept on record by
    tests/test_superpoints_cpu.py), so a correct conversion returns it unchanged.  The entries that do round are further down."""
    c = _cloud(name)
    count, s, S = c.scatter()
    dcount, _, _, dS = ops.voxel_normals(c.dxyz, c.dev.inv, c.dev.nbr, scatter=True)
    _assert_scatter_is_the_rounded_integer(name, count, S, dcount, dS)
    got = dS.cpu().numpy()
    assert all(Fraction(float(got[v, k])) == S[v][k] for v in range(c.V) for k in range(6))
    if name == "heavy":
        # S itself is small (nearly all points coincide); the two products it is the difference of are not
        assert int(count.max()) == 5010 and int(s.max()) ** 2 > 1 << 64, "the case is meant to need more than 64 bits on the way"
    if name == "small4":
        assert int(count.max()) == 4


class Hand:
    """One neighbourhood built by hand (tests/normal_cases.py): V = 1, inv = 0, nbr = -1.  The exact scatter matrix and the device's outputs, once."""

    def __init__(self, name):
        self.name = name
        if name in NC.rounding_cases():
            self.xyz, self.inv, self.nbr = NC.two_cluster(*NC.rounding_cases()[name])
        else:
            self.xyz, self.inv, self.nbr = NC.degenerate(name)
        self.N, self.V = len(self.xyz), 1
        self.dxyz, self.dinv, self.dnbr = (torch.from_numpy(a).cuda() for a in (self.xyz, self.inv, self.nbr))
        self._scatter = self._device = None

    def scatter(self):
        if self._scatter is None:
            self._scatter = SP.scatter(self.xyz, self.inv, self.nbr)
        return self._scatter

    def device(self, ops):
        """(count, normal, curvature, scatter) as the device returned them."""
        if self._device is None:
            self._device = ops.voxel_normals(self.dxyz, self.dinv, self.dnbr, scatter=True)
        return self._device


_HANDS = {}
ROUNDING = sorted(NC.rounding_cases())
DEGENERATE = sorted(NC.degenerate_fixed())
WIDE = sorted(NC.WIDE)


def _case(name):
    """A hand-built neighbourhood or one of the clouds, built once per session and never modified: both have scatter() and device(ops)."""
    if name not in NC.rounding_cases() and name not in NC.degenerate_fixed():
        return _cloud(name)
    if name not in _HANDS:
        _HANDS[name] = Hand(name)
    return _HANDS[name]


def _device4(ops, c):
    """(count, normal, curvature, scatter) of the device for either kind of case."""
    return c.device(ops) if isinstance(c, Hand) else ops.voxel_normals(c.dxyz, c.dev.inv, c.dev.nbr, scatter=True)


@pytest.mark.parametrize("name", ROUNDING + DEGENERATE + WIDE)
def test_scatter_is_float_of_the_exact_integer_where_it_rounds(ops, name):
    """Entries above 2^53 and above 2^64, on rounding ties, just below half, and at half with the only lower bits beyond the top 64 -- for both signs
    and in both branches of the conversion -- equal float(exact) bit for bit; so do the small entries of the degenerate neighbourhoods."""
    c = _case(name)
    count, s, S = c.scatter()
    dcount, _, _, dS = _device4(ops, c)
    largest, above, rounded = _assert_scatter_is_the_rounded_integer(name, count, S, dcount, dS)
    if name in NC.rounding_cases():
        m, d = NC.rounding_cases()[name]
        want = name.split("_", 1)[1].replace("_neg", "")
        assert S == [NC.two_cluster_scatter(m, d)] and NC.pattern(S[0][1]) == want and (S[0][1] < 0) == name.endswith("_neg")
        assert (largest > 64) == name.startswith("high") and rounded >= 4
    if name in NC.WIDE:
        assert (largest, above, rounded) == NC.WIDE_COUNTS[name] and above > 0 and rounded > 0


# ------------------------------------------------------------------------------------------------ 2. normals and curvature
def _gap_ok(count, lam, min_points=5):
    valid = count >= min_points
    return valid, valid & (lam[:, 1] - lam[:, 0] >= 1e-4 * lam[:, 2])


@pytest.mark.parametrize("name", ["box", "sphere", "uniform6000", "grid", "edge", "duplicates", "heavy", "small63", "small65", "small4"])
def test_normals_and_curvature_against_eigh_of_the_exact_scatter(ops, name):
    """On voxels with count >= min_points and an eigenvalue gap l1 - l0 >= 1e-4 l2: |n_dev x n_ref| <= 1e-7, | |n| - 1 | <= 1e-7 and
    |curvature - ref| <= 1e-7, the reference in fp64.  Budget: fp32 rounding of a unit vector is at most sqrt(3) 2^-25 = 5.2e-8, the fp64 solver's
    share is below 1e-9 under the gap condition; the curvature is at most 1/3, its fp32 rounding 1.5e-8.
    Voxels without the gap may be left out, up to 1 % of the valid ones.  Below min_points: (0, 0, 0) and 0, exactly."""
    c = _cloud(name)
    count, s, S = c.scatter()
    rn, rk, lam = c.normals()                              # fp64: the budget below has room for ONE rounding to fp32, the device's
    _, _, _, dc, dn, dk = c.device(ops)
    valid, ok = _gap_ok(count, lam)
    assert np.array_equal(dc, count.astype(np.int32))
    assert not dn[~valid].any() and not dk[~valid].any(), "no normal below min_points"
    left_out = int(valid.sum() - ok.sum())
    print(f"{name}: {int(valid.sum())} valid voxels of {c.V}, {left_out} without the eigenvalue gap")
    assert left_out <= 0.01 * valid.sum()
    if name in ("box", "sphere", "uniform6000", "grid"):
        assert left_out == 0, "a CPU run of the reference left out none on these clouds"
        assert valid.sum() > 100
    if not ok.any():
        assert name in ("small4",), name
        return
    a, b = dn[ok].astype(np.float64), rn[ok]
    cross = np.linalg.norm(np.cross(a, b), axis=1)
    length = np.abs(np.linalg.norm(a, axis=1) - 1)
    dcurv = np.abs(dk[ok].astype(np.float64) - rk[ok])
    print(f"{name}: worst |n x n_ref| {cross.max():.3e}, worst | |n| - 1 | {length.max():.3e}, worst curvature difference {dcurv.max():.3e}")
    assert cross.max() <= 1e-7 and length.max() <= 1e-7 and dcurv.max() <= 1e-7
    # the sign rule, on the stored fp32 values themselves: the component of largest magnitude is positive, on a tie the lowest axis decides
    mag = np.abs(dn[valid])
    lead = np.where((mag[:, 0] >= mag[:, 1]) & (mag[:, 0] >= mag[:, 2]), 0, np.where(mag[:, 1] >= mag[:, 2], 1, 2))
    assert (dn[valid][np.arange(len(lead)), lead] > 0).all()
    if name == "grid":
        assert np.array_equal(dn[valid], np.tile(np.array([0, 0, 1], dtype=f32), (int(valid.sum()), 1))) and not dk.any(), "a lattice plane: exactly z and 0"


@pytest.mark.parametrize("name", DEGENERATE + ROUNDING + WIDE)
def test_normals_without_an_eigenvalue_gap_are_eigenvectors_of_the_smallest_eigenvalue(ops, name):
    """EVERY voxel with count >= min_points, whatever its spectrum: coincident points, lines, exact planes, isotropic neighbourhoods, rank-one
    matrices.  No eigenvector is pinned; with n the device's normal in fp64, M = float(S), l0 <= l1 <= l2 = eigvalsh(M), rho = n^T M n / n^T n:

        n finite, | |n| - 1 | <= 1e-7, the component of largest magnitude positive (on the stored fp32 values)
        |M n - rho n| <= 1e-7 l2      fp32 rounding of a unit vector moves it by at most sqrt(3) 2^-25 = 5.2e-8, times l2 - l0
        rho - l0 <= 1e-12 l2          second order in that rounding: 2.7e-15 (l2 - l0), plus the fp64 evaluation here and in eigvalsh (some 1e-15 l2)
        |curvature - max(l0, 0) / (l0 + l1 + l2)| <= 1e-7, and exactly 0 where the trace is 0

    Printed with -s: the worst (rho - l0) / l2, residual and curvature difference per case.  Measured on an MI355X when the test was written: the
    worst (rho - l0) / l2 was 8.5e-16 (high_tie_odd: a rank-one matrix of 68-bit entries), 1.7e-16 on wide and at most 1.1e-16 on the degenerate
    neighbourhoods; the worst residual 3.0e-8 l2 and the worst curvature difference 9.9e-9 (cubic: the fp32 rounding of 1 / 3)."""
    c = _case(name)
    count, s, S = c.scatter()
    dev = c.device(ops)
    dn, dk = dev[1].cpu().numpy(), dev[2].cpu().numpy()
    assert np.array_equal(dev[0].cpu().numpy(), count.astype(np.int32)) and (count >= 5).all() and dn.dtype == f32 and dk.dtype == f32
    Sf = SP.scatter_float(S)
    worst_rho = worst_res = worst_curv = 0.0
    for v in range(len(S)):
        xx, xy, xz, yy, yz, zz = Sf[v]
        M = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])
        lam = np.linalg.eigvalsh(M)
        n = dn[v].astype(np.float64)
        assert np.isfinite(n).all() and np.isfinite(dk[v]) and abs(np.linalg.norm(n) - 1) <= 1e-7, (name, v, dn[v], dk[v])
        mag = np.abs(dn[v])
        lead = 0 if (mag[0] >= mag[1] and mag[0] >= mag[2]) else (1 if mag[1] >= mag[2] else 2)
        assert dn[v][lead] > 0, (name, v, dn[v])
        rho = float(n @ M @ n) / float(n @ n)
        res = float(np.linalg.norm(M @ n - rho * n))
        assert res <= 1e-7 * lam[2], (name, v, res, lam)
        assert rho - lam[0] <= 1e-12 * lam[2], (name, v, rho, lam)
        trace = float(lam.sum())
        want = max(lam[0], 0.0) / trace if trace > 0 else 0.0
        assert abs(float(dk[v]) - want) <= 1e-7 and (trace > 0 or dk[v] == 0), (name, v, dk[v], want)
        if lam[2] > 0:
            worst_rho, worst_res = max(worst_rho, (rho - lam[0]) / lam[2]), max(worst_res, res / lam[2])
        worst_curv = max(worst_curv, abs(float(dk[v]) - want))
    largest, above, rounded = NC.scatter_stats(S)
    print(f"{name}: largest |S| = 2^{largest}, {rounded} entries not representable, worst (rho - l0) / l2 = {worst_rho:.3e}, "
          f"worst |M n - rho n| / l2 = {worst_res:.3e}, worst curvature difference {worst_curv:.3e}")
    # where the definition gives the value itself
    if name == "coincident":
        assert lam[2] == 0 and dk[0] == 0
    if name == "cubic":
        assert dk[0] == f32(1 / 3), "three equal eigenvalues"


@pytest.mark.parametrize("name,view", [("box", (0.9, 0.8, 0.7)), ("sphere", (0.0, 0.0, 0.0)), ("uniform6000", (-1.0, 2.0, 0.5))])
def test_normals_face_the_viewpoint(ops, name, view):
    """With a viewpoint the sign gives n . (viewpoint - mean) >= 0.  Compared with the reference where the reference's own |n . (w - m)| is at least
    1e-6 |w - m| (nearer to perpendicular the sign is decided by rounding); those voxels share the 1 % cap with the ones without the gap."""
    c = _cloud(name)
    count, s, S = c.scatter()
    rn, rk, lam, facing = SP.normals(count, s, S, viewpoint=view)
    dc, dn, dk, _ = ops.voxel_normals(c.dxyz, c.dev.inv, c.dev.nbr, viewpoint=view)
    dn = dn.cpu().numpy()
    valid, ok = _gap_ok(count, lam)
    ok &= facing >= 1e-6
    assert valid.sum() - ok.sum() <= 0.01 * valid.sum()
    dots = (dn[ok].astype(np.float64) * rn[ok].astype(np.float64)).sum(1)
    assert (dots > 0.999).all(), "the same direction AND the same sign"
    # and against the definition, from the device's own normals
    mean = (s[ok].astype(np.float64) / count[ok, None] - SP.ONE) / SP.ONE
    assert ((dn[ok].astype(np.float64) * (np.asarray(view, dtype=f32).astype(np.float64) - mean)).sum(1) > 0).all()
    if name == "sphere":                                  # seen from the centre every normal points inwards
        assert ((dn[ok].astype(np.float64) * mean).sum(1) < 0).all()
    # the unsigned outputs do not depend on the viewpoint
    _, dn0, dk0, _, _, _ = c.device(ops)
    assert torch.equal(dk, dk0) and torch.equal(torch.from_numpy(dn).cuda().abs(), dn0.abs())


# ------------------------------------------------------------------------------------------------ 3. reproducibility
def _labels(ops, c, dev_normals, **kw):
    from point_sam_amd.superpoints import SuperpointConfig
    cfg = SuperpointConfig(**kw)
    count, normal, curv = dev_normals
    return ops.superpoint_labels(c.dev.inv, c.dev.nbr, count, normal, curv, cfg.cos_angle, cfg.max_curvature, cfg.min_points, cfg.min_size, cfg.absorb_rounds)


@pytest.mark.parametrize("name", ["box", "uniform6000", "duplicates", "heavy"])
def test_two_runs_and_a_shuffled_copy_give_identical_bytes(ops, name):
    c = _cloud(name)
    first = ops.voxel_normals(c.dxyz, c.dev.inv, c.dev.nbr, scatter=True)
    second = ops.voxel_normals(c.dxyz, c.dev.inv, c.dev.nbr, scatter=True)
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(first, second))
    l1, l2 = _labels(ops, c, first[:3]), _labels(ops, c, first[:3])
    assert all(torch.equal(a, b) for a, b in zip(l1, l2))
    # another order of the same points: other voxel ranks, other atomic arrival orders -- point for point the same normal and curvature bytes
    perm = np.random.default_rng(1).permutation(c.N)
    s = Cloud(c.xyz[perm], c.h)
    third = ops.voxel_normals(s.dxyz, s.dev.inv, s.dev.nbr)
    back = torch.from_numpy(np.argsort(perm)).cuda()      # point i of the original is point back[i] of the shuffled copy
    n0, k0 = first[1][c.dev.inv], first[2][c.dev.inv]
    n1, k1 = third[1][s.dev.inv][back], third[2][s.dev.inv][back]
    assert torch.equal(n0.view(torch.int32), n1.view(torch.int32)) and torch.equal(k0.view(torch.int32), k1.view(torch.int32))
    # and the same partition into superpoints (the ids follow the voxel ranks, which moved)
    p0 = _labels(ops, c, first[:3])[1].cpu().numpy()
    p1 = _labels(ops, s, third[:3])[1][back].cpu().numpy()
    assert np.array_equal(SP.partition(p0), SP.partition(p1))
    assert len(set(p0.tolist())) > 1 or name == "heavy"


@pytest.mark.parametrize("name", ["wide", "high_tie_odd", "low_tie_even_neg"])
def test_rounded_scatter_is_identical_between_runs_and_orders_of_the_points(ops, name):
    """Where S is rounded, and with tens of thousands of points behind every word of the table: two runs, and a shuffled copy, give the same bytes
    of count, normal, curvature and scatter."""
    c = _case(name)
    inv, nbr = (c.dinv, c.dnbr) if isinstance(c, Hand) else (c.dev.inv, c.dev.nbr)
    first = ops.voxel_normals(c.dxyz, inv, nbr, scatter=True)
    second = ops.voxel_normals(c.dxyz, inv, nbr, scatter=True)
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(first, second))
    perm = np.random.default_rng(2).permutation(c.N)
    back = torch.from_numpy(np.argsort(perm)).cuda()      # point i of the original is point back[i] of the shuffled copy
    if isinstance(c, Hand):                               # one voxel: the outputs themselves
        inv2 = inv
        third = ops.voxel_normals(torch.from_numpy(c.xyz[perm]).cuda(), inv, nbr, scatter=True)
    else:                                                 # other voxel ranks: point for point
        s = Cloud(c.xyz[perm], c.h)
        inv2 = s.dev.inv[back]
        third = ops.voxel_normals(s.dxyz, s.dev.inv, s.dev.nbr, scatter=True)
    for a, b in zip(first, third):
        assert torch.equal(a[inv].contiguous().view(torch.uint8), b[inv2].contiguous().view(torch.uint8))


# ------------------------------------------------------------------------------------------------ 4. superpoints
def _check_superpoints(ops, c, partition_only=False, **kw):
    from point_sam_amd.superpoints import SuperpointConfig
    cfg = SuperpointConfig(**kw)
    dcount, dnormal, dcurv, count, normal, curv = c.device(ops)
    vl, pl, size, num = _labels(ops, c, (dcount, dnormal, dcurv), **kw)
    S = int(num.item())
    want = SP.superpoints(c.ref.inv, c.ref.nbr, count, normal, curv, cfg.cos_angle, cfg.max_curvature, cfg.min_points, cfg.min_size, cfg.absorb_rounds)
    if partition_only:
        assert np.array_equal(SP.partition(pl.cpu().numpy()), SP.partition(want[1]))
        assert S == want[3]
        return S, want
    assert S == want[3]
    assert np.array_equal(vl.cpu().numpy(), want[0]) and np.array_equal(pl.cpu().numpy(), want[1])
    assert np.array_equal(size[:S].cpu().numpy(), want[2]) and int(size[:S].sum()) == c.N
    return S, want


@pytest.mark.parametrize("name", ["box", "sphere", "grid", "edge", "duplicates", "heavy", "small63", "small65", "small4"])
@pytest.mark.parametrize("rounds,min_size", [(0, 50), (1, 50), (2, 50), (2, 0)])
def test_superpoints_equal_the_reference_fed_the_device_normals(ops, name, rounds, min_size):
    c = _cloud(name)
    S, want = _check_superpoints(ops, c, absorb_rounds=rounds, min_size=min_size, voxel_size=c.h)
    if name == "box" and rounds == 0:
        big = np.sort(want[2])[::-1]
        assert big[2] > 800 and S > 3, "union only: three large planes, and the voxels along the edges on their own"
    if name == "box" and rounds == 2 and min_size == 50:
        assert S < 40 and np.sort(want[2])[::-1][2] > 1500, "the absorb rounds hand the edge voxels to the planes"
    if name == "grid":
        assert S == 1
    if name == "small4":
        assert S == c.V, "no voxel has a normal: nothing joins, nobody is large enough to absorb"


def test_superpoints_where_the_curvature_test_cuts_voxels_out(ops):
    """max_curvature at the median (sphere) or the upper quartile (box: its edges) of the REFERENCE's curvatures: a good part of the voxels is not
    smooth, stays out of the union and is absorbed."""
    for name, q in (("sphere", 0.5), ("box", 0.75)):
        c = _cloud(name)
        mc = float(np.quantile(c.normals()[1], q))
        curv, count = c.device(ops)[5], c.device(ops)[3]
        rough = int(((curv > f32(mc)) & (count >= 5)).sum())
        assert 0.1 * c.V < rough < 0.9 * c.V, (name, rough)
        for rounds in (0, 2):
            _check_superpoints(ops, c, max_curvature=mc, absorb_rounds=rounds, min_size=30, voxel_size=c.h)


def test_more_than_1024_superpoints(ops):
    """A uniform cloud at angle_deg = 1: nearly nothing joins, so the compaction's scan runs over more than one block of labels in use."""
    c = _cloud("uniform20000")
    for rounds, min_size in ((0, 0), (2, 50)):
        S, _ = _check_superpoints(ops, c, angle_deg=1.0, absorb_rounds=rounds, min_size=min_size, voxel_size=c.h, max_curvature=1.0)
        assert S > 1024
    c = _cloud("large")
    S, _ = _check_superpoints(ops, c, partition_only=True, angle_deg=1.0, absorb_rounds=0, voxel_size=c.h, max_curvature=1.0)
    assert S > 1024


def test_a_large_voxel_graph_gives_the_reference_partition(ops):
    c = _cloud("large")
    assert c.V > 70000
    S, want = _check_superpoints(ops, c, partition_only=True, angle_deg=30.0, max_curvature=1.0, absorb_rounds=2, min_size=20, voxel_size=c.h)
    print(f"large: V = {c.V}, {S} superpoints, largest {int(want[2].max())} points")
    assert 1 < S < c.V


def test_points_without_a_cell_get_no_label(ops):
    """inv outside [0, V) -- what a crop hands to the points off its ball -- gives label -1, and the point counts nowhere."""
    c = _cloud("box")
    inv = c.dev.inv.clone()
    off = torch.arange(0, c.N, 7, device="cuda")
    inv[off] = -1
    count, normal, curv, _ = ops.voxel_normals(c.dxyz, inv, c.dev.nbr)
    ninv = inv.cpu().numpy()
    rc, rs, rS = SP.scatter(c.xyz, ninv, c.ref.nbr)
    assert np.array_equal(count.cpu().numpy(), rc.astype(np.int32))
    vl, pl, size, num = ops.superpoint_labels(inv, c.dev.nbr, count, normal, curv, SP.cos_of(15.0), 0.08, 5, 50, 2)
    want = SP.superpoints(ninv, c.ref.nbr, count.cpu().numpy(), normal.cpu().numpy(), curv.cpu().numpy(), SP.cos_of(15.0), 0.08, 5, 50, 2)
    S = int(num.item())
    assert S == want[3] and np.array_equal(pl.cpu().numpy(), want[1]) and np.array_equal(size[:S].cpu().numpy(), want[2])
    assert (pl[off] == -1).all() and int(size[:S].sum()) == c.N - len(off)


# ------------------------------------------------------------------------------------------------ 5. snap
def _superpoints_of(ops, c):
    from point_sam_amd.superpoints import SuperpointConfig, build_superpoints
    if not hasattr(c, "sp"):
        c.sp = build_superpoints(c.dev, c.dxyz, SuperpointConfig(voxel_size=c.h, min_size=20))
    return c.sp


def _snap_masks(c, K, seed):
    """Balls around random points of the cloud, radii from a tenth to half of its extent; row 0 empty and row 1 full where there is room."""
    rng = np.random.default_rng(seed)
    centres = c.xyz[rng.choice(c.N, K)]
    radii = rng.uniform(0.1, 0.5, K)
    masks = np.linalg.norm(c.xyz[None] - centres[:, None], axis=2) < radii[:, None]
    if K >= 3:
        masks[0], masks[1] = False, True
    return masks


@pytest.mark.parametrize("name", ["box", "small65"])
@pytest.mark.parametrize("K", [1, 3, 70])
def test_snap_equals_the_reference(ops, name, K):
    from point_sam_amd.superpoints import snap_bits
    c = _cloud(name)
    sp = _superpoints_of(ops, c)
    assert c.N % 64 != 0 and sp.num == sp.size.numel() and sp.num >= 1
    label, size = sp.labels.cpu().numpy(), sp.size.cpu().numpy()
    masks = _snap_masks(c, K, K)
    bits = _dev_words(masks)
    bits[:, -1] |= -1 << (c.N % 64)                           # rubbish past N in the input: ignored, and zero in the output
    for q16 in (0, 32768, 65535):
        out, area, changed = ops.superpoint_snap(bits, sp.labels, sp.size, q16)
        want, warea, wchanged = SP.snap(masks, label, size, q16)
        assert np.array_equal(_np_words(out), SR.words(want)), (name, K, q16)
        assert np.array_equal(area.cpu().numpy(), warea) and np.array_equal(changed.cpu().numpy(), wchanged)
        assert np.array_equal(area.cpu().numpy(), np.unpackbits(_np_words(out).view(np.uint8), axis=1).sum(1)), "area is the popcount of the output"
        # every output row is a union of whole superpoints
        for k in range(K):
            inside = np.bincount(label[want[k] & (label >= 0)], minlength=sp.num)
            assert ((inside == 0) | (inside == size)).all()
    # the chunked wrapper: min_fraction -> q16, several calls, the same rows
    whole = snap_bits(sp, bits, 0.5)
    parts = snap_bits(sp, bits, 0.5, chunk=2)
    want, warea, _ = SP.snap(masks, label, size, 32768)
    assert all(torch.equal(a, b) for a, b in zip(whole, parts)) and np.array_equal(_np_words(whole[0]), SR.words(want))
    assert np.array_equal(whole[1].cpu().numpy(), warea)
    if K == 70 and name == "box":
        touched = SP.snap(masks, label, size, 0)[0].sum(1)
        assert (touched[2:] >= want.sum(1)[2:]).all() and (touched[2:] > want.sum(1)[2:]).any(), "any touch selects more than a strict majority"


def test_disjoint_rows_stay_disjoint_at_a_strict_majority(ops):
    c = _cloud("box")
    sp = _superpoints_of(ops, c)
    # three slabs along the diagonal: a partition of the cloud that cuts across every plane
    t = c.xyz.sum(1)
    cut = np.quantile(t, [1 / 3, 2 / 3])
    masks = np.stack([t < cut[0], (t >= cut[0]) & (t < cut[1]), t >= cut[1]])
    out, area, changed = ops.superpoint_snap(_dev_words(masks), sp.labels, sp.size, 32768)
    got = _np_words(out)
    assert not (got[0] & got[1]).any() and not (got[0] & got[2]).any() and not (got[1] & got[2]).any()
    assert changed.cpu().numpy().all() and int(area.sum()) <= c.N
    loose = _np_words(ops.superpoint_snap(_dev_words(masks), sp.labels, sp.size, 0)[0])
    assert (loose[0] & loose[1]).any(), "below a half the rows may overlap: the bound is not vacuous here"


# ------------------------------------------------------------------------------------------------ 6. predictor
@pytest.fixture(scope="module")
def predictor(ops):
    from point_sam_amd.config import get_config
    from point_sam_amd.model import PointCloudSAM
    from point_sam_amd.predictor import PointSAMPredictor
    from point_sam_amd.weights import random_state_dict
    cfg = get_config("tiny")
    return PointSAMPredictor(PointCloudSAM(cfg, random_state_dict(cfg, 3), "cuda", precision="f16x3"))


def _room(n, seed):
    rng = np.random.default_rng(seed)
    xyz = np.concatenate([_plane(rng, n // 3, a, 0.002) for a in range(3)] + [_plane(rng, n - 3 * (n // 3), 0, 0.002)]).astype(f32)
    xyz = xyz[rng.permutation(n)]
    return torch.from_numpy(xyz).cuda(), torch.from_numpy(rng.uniform(-1, 1, (n, 3)).astype(f32)).cuda()


def test_predictor_superpoints_after_set_scene_have_the_scans_width_and_are_cached(ops, predictor):
    from point_sam_amd.superpoints import SuperpointConfig, snap_bits
    xyz, rgb = _room(6000, 11)
    predictor.set_scene(xyz, rgb, max_points=2048)
    assert predictor.scene.num_working < 6000
    cfg = SuperpointConfig(voxel_size=0.05)
    sp = predictor.superpoints(cfg)
    assert sp.labels.shape == (6000,) and sp.num == sp.size.numel() and int(sp.size.sum()) == 6000
    assert predictor.superpoints(SuperpointConfig(voxel_size=0.05)) is sp, "cached per configuration"
    other = predictor.superpoints(SuperpointConfig(voxel_size=0.05, min_size=0))
    assert other is not sp and other.num > sp.num
    # against the reference, from the device's normals
    g = R.Graph(xyz.cpu().numpy(), 0.05)
    n = sp.normals
    want = SP.superpoints(g.inv, g.nbr, n.count.cpu().numpy(), n.normal.cpu().numpy(), n.curvature.cpu().numpy(), cfg.cos_angle, cfg.max_curvature,
                          cfg.min_points, cfg.min_size, cfg.absorb_rounds)
    assert sp.num == want[3] and np.array_equal(sp.labels.cpu().numpy(), want[1])
    normal, curv = predictor.point_normals(cfg=cfg)
    inv = torch.from_numpy(g.inv).cuda()
    assert normal.shape == (6000, 3) and curv.shape == (6000,) and torch.equal(normal, n.normal[inv]) and torch.equal(curv, n.curvature[inv])
    facing, _ = predictor.point_normals(viewpoint=(-0.9, -0.9, -0.9), cfg=cfg)      # behind all three planes: their normals turn round
    assert torch.equal(facing.abs(), normal.abs()) and not torch.equal(facing, normal)

    # snap_masks of predict_mask_bits' rows == snap_bits on the same rows
    pts = xyz[torch.tensor([[5], [700]], device="cuda")]
    bits = predictor.predict_mask_bits(pts, torch.ones(2, 1, dtype=torch.int64, device="cuda"))[0]
    bits = bits.reshape(-1, bits.shape[-1]).contiguous()
    assert bits.shape[1] == ops.mask_words(6000)
    got = predictor.snap_masks(bits, cfg)
    want = snap_bits(sp, bits, 0.5)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    ref, rarea, _ = SP.snap(ops.mask_unpack(bits, 6000).cpu().numpy().astype(bool), sp.labels.cpu().numpy(), sp.size.cpu().numpy(), 32768)
    assert np.array_equal(_np_words(got[0]), SR.words(ref)) and np.array_equal(got[1].cpu().numpy(), rarea)
    with pytest.raises(ValueError):
        predictor.snap_masks(bits[:, :-1].contiguous(), cfg)
    # another cloud drops the cache
    xyz2, rgb2 = _room(3000, 12)
    predictor.set_pointcloud(xyz2, rgb2)
    sp2 = predictor.superpoints(cfg)
    assert sp2 is not sp and sp2.labels.shape == (3000,)


def test_generate_masks_is_unchanged_without_snap_and_rows_are_unions_of_superpoints_with_it(ops, predictor):
    from point_sam_amd.proposals import ProposalConfig, generate_proposals
    from point_sam_amd.regions import build_graph
    from point_sam_amd.superpoints import SuperpointConfig, build_superpoints
    xyz, rgb = _room(2048, 13)
    predictor.set_pointcloud(xyz, rgb)
    st = predictor._state
    ninf = float("-inf")
    probe = predictor.model.decode(st, xyz[None, :1], torch.ones(1, 1, dtype=torch.int64, device="cuda"), None, True)[0]
    base = dict(num_prompts=16, prompt_chunk=8, mask_threshold=float(probe.median()), pred_iou_thresh=ninf, stability_thresh=ninf, min_points=1,
                max_area_frac=1.0001)
    assert ProposalConfig().snap is None
    a = predictor.generate_masks(ProposalConfig(**base))[0]
    b = generate_proposals(predictor.model, st, ProposalConfig(**base, snap=None))[0]
    assert len(a) >= 1 and a.changed is None
    for name in ("bits", "candidate", "score", "area", "stability", "labels"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    # the rows a run with snap starts from are the rows of the run without: snap them with the reference and compare what is kept
    sc = SuperpointConfig(voxel_size=0.05, min_size=20)
    snapped = predictor.generate_masks(ProposalConfig(**base, snap=sc))[0]
    sp = build_superpoints(build_graph(st.coords[0].contiguous(), 0.05), st.coords[0].contiguous(), sc)
    label, size = sp.labels.cpu().numpy(), sp.size.cpu().numpy()
    assert len(snapped) >= 1 and snapped.changed is not None
    rows = ops.mask_unpack(snapped.bits.contiguous(), 2048).cpu().numpy().astype(bool)
    for k in range(len(rows)):
        inside = np.bincount(label[rows[k] & (label >= 0)], minlength=sp.num)
        assert ((inside == 0) | (inside == size)).all(), "every kept row is a union of superpoints"
        assert not rows[k][label < 0].any()
    assert np.array_equal(snapped.area.cpu().numpy(), rows.sum(1))
