"""Instance geometry on the GPU (csrc/geometry.hip: ops.mask_moments / ops.mask_extents, point_sam_amd/geometry.py, predictor.mask_geometry /
set_crop_to_mask) against the plain numpy reference of tests/geometry_reference.py.

Counts, boxes and extents are compared exactly (integer views of the fp32 bits).  The fp64 sums are compared against math.fsum of the exact terms
with the bound that holds for ANY order of IEEE additions: |gpu - fsum| <= n 2^-52 sum|term| (gamma_{n-1} sum|t| with gamma_m = m u / (1 - m u),
u = 2^-53, plus fsum's own half ulp u |S|; the factor 2 covers 1 / (1 - n u)).  It is derived, not tuned."""
import functools
import math

import numpy as np
import pytest
import torch

import geometry_reference as G

pytestmark = pytest.mark.gpu
f32 = np.float32

# The kernel's own constant (ops.INSTANCE_RANGE_WORDS = PSAM_INSTANCE_RANGE_WORDS): a wave owns 256 words = 16384 points of a row.
RANGE_POINTS = 256 * 64
N_ONE_RANGE = RANGE_POINTS            # the largest N at which a row is handled by a single wave range
N_SPLIT = RANGE_POINTS + 1            # the smallest N at which it is split over several (two; the second holds one point)
SIZES = (1, 63, 64, 65, 4097, N_ONE_RANGE, N_SPLIT)
ROWS = (1, 3, 65)
KINDS = ("empty", "full", "first", "last", "sparse", "dense", "every64", "oneword")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd import ops
    assert ops.INSTANCE_RANGE_WORDS * 64 == RANGE_POINTS
    return ops


def _row(kind, N, rng):
    m = np.zeros(N, dtype=bool)
    if kind == "full":
        m[:] = True
    elif kind == "first":
        m[0] = True
    elif kind == "last":
        m[N - 1] = True
    elif kind == "sparse":
        m = rng.random(N) < 0.01
    elif kind == "dense":
        m = rng.random(N) < 0.5
    elif kind == "every64":
        m[::64] = True                                   # one bit per word
    elif kind == "oneword":
        w = ((N + 63) // 64) // 2                         # one fully set word between empty ones
        m[w * 64:min(w * 64 + 64, N)] = True
    return m


@functools.lru_cache(maxsize=None)
def _case(N, K, kinds=KINDS):
    """Seeded inputs and their reference, computed once and shared (never modified).  Coordinates up to magnitude 4 (the model's accepted range),
    colours in [-1, 1]."""
    rng = np.random.default_rng(1000 * K + N)
    xyz = rng.uniform(-4, 4, (N, 3)).astype(f32)
    rgb = rng.uniform(-1, 1, (N, 3)).astype(f32)
    first = N % len(kinds)                                # fewer rows than kinds: another selection at every size
    names = [kinds[(first + k) % len(kinds)] for k in range(K)]
    mask = np.stack([_row(n, N, rng) for n in names])
    bits = G.words(mask)
    origin = (xyz[rng.integers(0, N, K)] + rng.normal(0, 0.1, (K, 3))).astype(f32)
    q, _ = np.linalg.qr(rng.normal(0, 1, (K, 3, 3)))
    frames = {"identity": None, "orthonormal": q.astype(f32), "skew": rng.uniform(-1.5, 1.5, (K, 3, 3)).astype(f32)}
    for a in (xyz, rgb, mask, bits, origin):
        a.setflags(write=False)
    return dict(N=N, K=K, kinds=kinds, xyz=xyz, rgb=rgb, mask=mask, bits=bits, names=names, origin=origin, frames=frames)


@functools.lru_cache(maxsize=None)
def _ref_cached(N, K, kinds):
    c = _case(N, K, kinds)
    ref = G.mask_moments(c["xyz"], c["bits"], c["rgb"])
    assert np.array_equal(ref[0], c["mask"].sum(1))
    return ref


def _ref(c):
    """(count, fsum sums, lo, hi, fsum of |term|) of a case: computed once, shared."""
    return _ref_cached(c["N"], c["K"], c["kinds"])


def _dirty(c, fill=1e30, extra=97):
    """The case on the device with a hostile surrounding: every bit at a position >= N set, xyz / rgb views of the first N rows of a larger buffer
    whose other rows hold 1e30.  A read past N shows up as a wrong value."""
    N = c["N"]
    bits = c["bits"].copy()
    if N % 64:
        bits[:, -1] |= np.int64(-1) << np.int64(N % 64)
    big_xyz, big_rgb = torch.full((N + extra, 3), fill, dtype=torch.float32, device="cuda"), torch.full((N + extra, 3), fill, dtype=torch.float32, device="cuda")
    big_xyz[:N], big_rgb[:N] = _dev(c["xyz"]), _dev(c["rgb"])
    return big_xyz[:N], big_rgb[:N], torch.from_numpy(bits).cuda()


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()           # a copy: the cases are read-only


def _clean(c):
    return _dev(c["xyz"]), _dev(c["rgb"]), _dev(c["bits"])


def _i32(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, dtype=f32).view(np.int32)


def _i64(a):
    return np.ascontiguousarray(a.cpu().numpy(), dtype=np.float64).view(np.int64)


def _check_moments(got, c, label=""):
    count, sums, lo, hi = got
    want_count, want_sums, want_lo, want_hi, abs_sums = _ref(c)
    assert count.dtype == torch.int32 and sums.dtype == torch.float64 and lo.dtype == torch.float32 and tuple(sums.shape) == (c["K"], 12)
    assert np.array_equal(count.cpu().numpy(), want_count), label
    assert np.array_equal(_i32(lo), _i32(want_lo)) and np.array_equal(_i32(hi), _i32(want_hi)), label
    err = np.abs(sums.cpu().numpy() - want_sums)
    bound = want_count[:, None].astype(np.float64) * 2.0 ** -52 * abs_sums
    worst = float((err / np.where(bound > 0, bound, 1)).max())
    print(f"{label} N={c['N']} K={c['K']}: max |gpu - fsum| / bound = {worst:.3g}")
    assert (err <= bound).all(), (label, np.argwhere(err > bound)[:5], worst)


@pytest.mark.parametrize("K", ROWS)
@pytest.mark.parametrize("N", SIZES)
def test_moments_count_box_and_sums(ops, N, K):
    c = _case(N, K)
    xyz, rgb, bits = _dirty(c)
    got = ops.mask_moments(xyz, bits, rgb)
    _check_moments(got, c, "dirty tail")
    cx, cr, cb = _clean(c)
    clean = ops.mask_moments(cx, cb, cr)
    for a, b in zip(got, clean):                           # the tail bits and the surrounding buffer change nothing, bit for bit
        assert torch.equal(a, b)
    empty = np.nonzero(_ref(c)[0] == 0)[0]
    sums = got[1].cpu().numpy()
    assert (sums[empty] == 0).all() and not np.signbit(sums[empty]).any()
    assert np.isposinf(got[2].cpu().numpy()[empty]).all() and np.isneginf(got[3].cpu().numpy()[empty]).all()


@pytest.mark.parametrize("frame", ("identity", "orthonormal", "skew"))
@pytest.mark.parametrize("K", ROWS)
@pytest.mark.parametrize("N", SIZES)
def test_extents_are_the_float32_emulation(ops, N, K, frame):
    c = _case(N, K)
    axes = c["frames"][frame]
    want = G.mask_extents(c["xyz"], c["bits"], c["origin"], axes)
    xyz, _, bits = _dirty(c)
    origin = _dev(c["origin"])
    got = ops.mask_extents(xyz, bits, origin, None if axes is None else _dev(axes))
    for g, w, name in zip(got, want, ("lo", "hi", "r2max")):
        assert g.dtype == torch.float32 and np.array_equal(_i32(g), _i32(w)), (name, frame)
    cx, _, cbits = _clean(c)
    for g, h in zip(got, ops.mask_extents(cx, cbits, origin, None if axes is None else _dev(axes))):
        assert torch.equal(g, h)
    empty = c["mask"].sum(1) == 0
    assert np.isposinf(want[0][empty]).all() and np.isneginf(want[1][empty]).all() and np.isneginf(want[2][empty]).all()


def test_the_box_orders_negative_zero_below_positive_zero(ops):
    xyz = torch.tensor([[0.0, -0.0, 0.0], [-0.0, 0.0, 0.0], [0.0, -0.0, -0.0]], device="cuda")
    bits = torch.tensor([[7]], dtype=torch.int64, device="cuda")
    _, _, lo, hi = ops.mask_moments(xyz, bits)
    assert np.signbit(lo.cpu().numpy()).tolist() == [[True, True, True]] and np.signbit(hi.cpu().numpy()).tolist() == [[False, False, False]]
    want = G.mask_moments(xyz.cpu().numpy(), bits.cpu().numpy())
    assert np.array_equal(_i32(lo), _i32(want[2])) and np.array_equal(_i32(hi), _i32(want[3]))


def test_one_larger_cloud(ops):
    """N = 2^20, K = 8: 64 wave ranges per row."""
    c = _case(1 << 20, 8, ("empty", "first", "last", "sparse", "dense", "every64", "oneword", "sparse"))
    xyz, rgb, bits = _dirty(c)
    _check_moments(ops.mask_moments(xyz, bits, rgb), c, "2^20")
    axes = c["frames"]["skew"]
    want = G.mask_extents(c["xyz"], c["bits"], c["origin"], axes)
    got = ops.mask_extents(xyz, bits, _dev(c["origin"]), _dev(axes))
    for g, w in zip(got, want):
        assert np.array_equal(_i32(g), _i32(w))


@pytest.mark.parametrize("N", (4097, N_SPLIT, 5 * RANGE_POINTS + 77))
def test_sums_are_bitwise_reproducible_and_independent_of_the_other_rows(ops, N):
    c = _case(N, 65)
    xyz, rgb, bits = _clean(c)
    first = ops.mask_moments(xyz, bits, rgb)
    second = ops.mask_moments(xyz, bits, rgb)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert np.array_equal(_i64(first[1]), _i64(second[1]))
    for kind in ("sparse", "dense", "full"):               # a sparse and a dense row, each computed alone
        k = c["names"].index(kind)
        alone = ops.mask_moments(xyz, bits[k:k + 1].contiguous(), rgb)
        assert np.array_equal(_i64(alone[1][0]), _i64(first[1][k])), kind
        assert int(alone[0][0]) == int(first[0][k]) and torch.equal(alone[2][0], first[2][k]) and torch.equal(alone[3][0], first[3][k])
    plain = ops.mask_moments(xyz, bits)                    # rgb=None: the colour columns are exactly zero, the others unchanged
    assert (plain[1][:, 9:] == 0).all() and not np.signbit(plain[1][:, 9:].cpu().numpy()).any()
    assert np.array_equal(_i64(plain[1][:, :9]), _i64(first[1][:, :9]))
    assert torch.equal(plain[0], first[0]) and torch.equal(plain[2], first[2]) and torch.equal(plain[3], first[3])


# ------------------------------------------------------------------------------------------------ geometry.mask_geometry end to end
HALF = np.array([0.5, 0.25, 0.125])                       # sides 1 : 0.5 : 0.25
SIDE = 16


@functools.lru_cache(maxsize=None)
def _cuboid():
    """A 16 x 16 x 16 lattice cuboid, corners included, rotated by a fixed rotation and shifted, stored in fp32 among 3 x as many distractors."""
    rng = np.random.default_rng(7)
    ang = (0.7, -0.4, 1.1)
    cz, sz, cy, sy, cx, sx = math.cos(ang[0]), math.sin(ang[0]), math.cos(ang[1]), math.sin(ang[1]), math.cos(ang[2]), math.sin(ang[2])
    rot = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])).T
    shift = np.array([0.3, -0.2, 0.25])
    t = np.linspace(-1, 1, SIDE)
    u = np.stack(np.meshgrid(t * HALF[0], t * HALF[1], t * HALF[2], indexing="ij"), -1).reshape(-1, 3)      # local coordinates; rows of rot are the axes
    obj = (shift + u @ rot).astype(f32)
    n = len(obj)
    xyz = rng.uniform(-1, 1, (4 * n, 3)).astype(f32)
    where = np.sort(rng.permutation(4 * n)[:n])
    xyz[where] = obj
    mask = np.zeros((1, 4 * n), dtype=bool)
    mask[0, where] = True
    rgb = rng.uniform(-1, 1, (4 * n, 3)).astype(f32)
    return xyz, rgb, mask, rot, shift, float(np.linalg.norm(HALF))


def _reference_axes(xyz, bits):
    """The host maths of geometry.py on the reference's correctly rounded moments."""
    from point_sam_amd.geometry import centroid_covariance, principal_axes
    count, sums, _, _, abs_sums = G.mask_moments(xyz, bits)
    c, cov, _ = centroid_covariance(count.astype(np.int64), sums)
    return count, sums, abs_sums, c, cov, principal_axes(cov)


def test_mask_geometry_of_a_rotated_cuboid(ops):
    from point_sam_amd.geometry import mask_geometry
    xyz, rgb, mask, rot, shift, reach = _cuboid()
    bits = G.words(mask)
    dx, db = torch.from_numpy(xyz).cuda(), torch.from_numpy(bits).cuda()
    geo = mask_geometry(dx, db, torch.from_numpy(rgb).cuda())
    idx = np.nonzero(mask[0])[0]
    n = len(idx)
    assert int(geo.count[0]) == n == SIDE ** 3 and bool(geo.valid[0])
    axes = geo.axes[0].numpy()
    assert geo.axes.dtype == torch.float32 and geo.centroid.dtype == torch.float64 and geo.obb_half.dtype == torch.float64

    # every member's projection lies within [lo, hi] of the returned frame: exactly, the kernel's operations emulated in float32
    origin = geo.centroid.float()
    lo, hi, r2max = (t.cpu().numpy()[0] for t in ops.mask_extents(dx, db, origin.cuda(), geo.axes.cuda()))
    p, r2 = G.project(xyz[idx], origin.numpy()[0], axes)
    assert (p >= lo).all() and (p <= hi).all() and (p.min(0) == lo).all() and (p.max(0) == hi).all() and r2.max() == r2max
    assert np.array_equal(geo.obb_half[0].numpy(), (hi.astype(np.float64) - lo) / 2) and float(geo.radius[0]) == float(np.sqrt(f32(r2max)))
    mid = (hi.astype(np.float64) + lo) / 2
    assert np.allclose(geo.obb_center[0].numpy(), origin.numpy()[0].astype(np.float64) + mid @ axes.astype(np.float64), rtol=0, atol=1e-15)

    # the axes against the reference's own (the same host maths on fsum moments).  The two covariances differ by the sums' error only:
    # |dS| <= n 2^-52 sum|t| per sum and C_ij = S_ij / n - c_i c_j, so |dC_ij| <= 2^-52 (sum|t_ij| + |c_i| sum|x_j| + |c_j| sum|x_i|), plus the host's
    # own fp64 roundings (a handful of operations on numbers below 2: 16 u); Davis-Kahan: sin(angle) <= 2 ||dC|| / gap.  The returned axes are fp32:
    # rounding moves each of the three components by at most 2^-25.  Axis 2 is the cross product of the other two and inherits both errors.
    count, sums, abs_sums, c, cov, ref_axes = _reference_axes(xyz, bits)
    u = 2.0 ** -53
    pair = {(0, 0): 3, (0, 1): 4, (0, 2): 5, (1, 1): 6, (1, 2): 7, (2, 2): 8}
    dC = np.zeros((3, 3))
    for (i, j), col in pair.items():
        dC[i, j] = dC[j, i] = 2 * u * (abs_sums[0, col] + abs(c[0, i]) * abs_sums[0, j] + abs(c[0, j]) * abs_sums[0, i]) + 16 * u
    lam = np.sort(np.linalg.eigvalsh(cov[0]))[::-1]
    gaps = np.array([lam[0] - lam[1], min(lam[0] - lam[1], lam[1] - lam[2]), lam[1] - lam[2]])
    eps = 2 * np.linalg.norm(dC) / gaps + math.sqrt(3) * 2.0 ** -25
    eps[2] = eps[0] + eps[1]
    dots = np.abs((axes.astype(np.float64) * ref_axes[0]).sum(1))
    print("axes: 1 - |dot| =", 1 - dots, "eps =", eps)
    assert (dots >= 1 - eps).all()
    assert abs(np.linalg.det(axes.astype(np.float64)) - 1) < 1e-6
    assert np.abs(geo.centroid[0].numpy() - c[0]).max() <= 2 * u * n * 4 and np.abs(geo.covariance[0].numpy() - cov[0]).max() <= dC.max()

    # obb_half against the generating half sides.  M = max |coordinate|.  Per projected coordinate, in units of 2^-24 M: the stored point is the
    # rotated one rounded to fp32 (each component off by <= 1, through a unit axis: sqrt 3); d = x - origin rounds once per component (sqrt 3);
    # three products and two sums round once each (5); the fp32 axes are off by 2^-25 per component against |d| <= M (< 1): 2 sqrt 3 + 6 < 9.5.
    # The frame itself is the stored points', not the generator's: it is tilted by `tilt`, which moves a half side by at most tilt * |u|max; that
    # is a property of the test data (measured on the reference's axes, not on the code under test) and is required to stay below one more unit.
    M = float(np.abs(xyz[idx]).max())
    unit = 2.0 ** -24 * M
    true_axes = rot * np.sign((rot * ref_axes[0]).sum(1))[:, None]
    tilt = np.linalg.norm(ref_axes[0] - true_axes, axis=1).max()
    assert tilt * reach <= unit, (tilt, unit)
    bound = 11 * unit
    half = geo.obb_half[0].numpy()
    print("obb_half - generating half sides:", half - HALF, "bound", bound)
    assert (np.abs(half - HALF) <= bound).all()

    # the axis-aligned box holds the oriented box's eight corners (they are lattice points) to within the same bound
    corners = np.array([geo.obb_center[0].numpy() + (((2 * np.array(s) - 1) * half) @ axes.astype(np.float64)) for s in np.ndindex(2, 2, 2)])
    alo, ahi = geo.aabb_lo[0].numpy().astype(np.float64), geo.aabb_hi[0].numpy().astype(np.float64)
    assert np.array_equal(_i32(geo.aabb_lo[0]), _i32(xyz[idx].min(0))) and np.array_equal(_i32(geo.aabb_hi[0]), _i32(xyz[idx].max(0)))
    assert (corners >= alo - bound).all() and (corners <= ahi + bound).all()
    assert np.abs(geo.mean_rgb[0].numpy() - rgb[idx].astype(np.float64).mean(0)).max() < 1e-12

    flat = mask_geometry(dx, db, None, oriented=False)
    assert flat.mean_rgb is None and np.array_equal(flat.axes[0].numpy(), np.eye(3, dtype=f32))
    assert np.array_equal(flat.obb_half[0].numpy(), (ahi - alo) / 2) and np.array_equal(flat.obb_center[0].numpy(), (ahi + alo) / 2)
    assert float(flat.radius[0]) == float(geo.radius[0])


# ------------------------------------------------------------------------------------------------ the predictor
M_SCAN, SCENE_POINTS = 6000, 1500


@pytest.fixture(scope="module")
def scan(ops):
    from oracle import pointsam_oracle as O
    from point_sam_amd.config import get_config
    from point_sam_amd.model import PointCloudSAM
    from point_sam_amd.weights import random_state_dict
    cfg = get_config("tiny")
    model = PointCloudSAM(cfg, random_state_dict(cfg, 3), "cuda", precision="f16x3")
    xyz, rgb, _, _ = O.synthetic_batch(1, M_SCAN, seed=8)
    return model, xyz[0].cuda().contiguous(), rgb[0].cuda().contiguous()


def _proposal_config(pred, xyz):
    from point_sam_amd.proposals import ProposalConfig
    logits, _, _ = pred.predict_masks(xyz[None, :1], torch.ones(1, 1, dtype=torch.int64, device="cuda"), None, True)
    return ProposalConfig(num_prompts=16, prompt_chunk=16, mask_threshold=float(logits.median()), pred_iou_thresh=float("-inf"), stability_thresh=0.0,
                          min_points=1, max_area_frac=1.0001)


def _same_geometry(a, b):
    for name in ("count", "centroid", "aabb_lo", "aabb_hi", "covariance", "mean_rgb", "axes", "obb_center", "obb_half", "radius", "valid"):
        x, y = getattr(a, name), getattr(b, name)
        assert torch.equal(x, y), name


def test_predictor_mask_geometry_on_a_scene(ops, scan):
    from point_sam_amd.geometry import mask_geometry
    from point_sam_amd.predictor import PointSAMPredictor
    model, xyz, rgb = scan
    pred = PointSAMPredictor(model)
    with pytest.raises(RuntimeError):
        pred.mask_geometry(torch.zeros(1, ops.mask_words(M_SCAN), dtype=torch.int64, device="cuda"))
    pred.set_scene(xyz, rgb, max_points=SCENE_POINTS)
    assert pred.scene.num_working < M_SCAN and not pred.scene.identity      # the working cloud is a true subset
    prop = pred.generate_masks(_proposal_config(pred, xyz))[0]
    assert len(prop) >= 1 and prop.n_points == M_SCAN
    geo = pred.mask_geometry(prop)
    assert torch.equal(geo.count, prop.area.cpu()) and bool(geo.valid.all())
    assert bool((geo.centroid >= geo.aabb_lo.double()).all()) and bool((geo.centroid <= geo.aabb_hi.double()).all())
    _same_geometry(geo, mask_geometry(xyz, prop.bits.contiguous(), rgb))
    _same_geometry(pred.mask_geometry(prop.bits), geo)
    with pytest.raises(ValueError, match=str(ops.mask_words(pred.scene.num_working))):      # working-width rows are the caller's to expand
        pred.mask_geometry(torch.zeros(2, ops.mask_words(pred.scene.num_working), dtype=torch.int64, device="cuda"))


def test_set_crop_to_mask_zooms_into_the_mask_and_back(ops, scan):
    from point_sam_amd.predictor import PointSAMPredictor
    model, xyz, rgb = scan
    pred = PointSAMPredictor(model)
    with pytest.raises(RuntimeError):
        pred.set_crop_to_mask(torch.zeros(ops.mask_words(M_SCAN), dtype=torch.int64, device="cuda"))
    pred.set_scene(xyz, rgb, max_points=SCENE_POINTS)
    click, one = xyz[None, 40:41], torch.ones(1, 1, dtype=torch.int64, device="cuda")
    before = pred.predict_masks(click, one, None, True)
    # a compact object: the points within 0.3 of the click
    member = ((xyz - xyz[40]) ** 2).sum(1) < 0.09
    row = torch.from_numpy(G.words(member.cpu().numpy()[None])).cuda()[0]
    with pytest.raises(ValueError, match="empty"):
        pred.set_crop_to_mask(torch.zeros_like(row))
    assert pred.crop is None
    center, radius = pred.set_crop_to_mask(row)
    assert pred.crop is not None and pred.crop.center == center and pred.crop.radius == radius
    geo = pred.mask_geometry(row[None], oriented=False)
    assert np.allclose(center, geo.centroid[0].numpy(), atol=1e-6) and abs(radius - 1.1 * float(geo.radius[0])) <= 1e-6
    inside = pred.crop.inv >= 0
    assert bool(inside[member].all()) and pred.crop.num_members >= int(member.sum())
    pred.set_crop_to_mask(row, margin=0.0)                 # the farthest member is still inside with no margin
    assert bool((pred.crop.inv >= 0)[member].all())
    pred.clear_crop()
    assert pred.crop is None
    after = pred.predict_masks(click, one, None, True)
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])
    with pytest.raises(ValueError, match="words"):
        pred.set_crop_to_mask(row[:-1])


def test_predictor_mask_geometry_on_a_batch_of_clouds(ops, scan):
    from point_sam_amd.geometry import mask_geometry
    from point_sam_amd.predictor import PointSAMPredictor
    model, xyz, rgb = scan
    n = 1024
    bx, br = torch.stack([xyz[:n], xyz[n:2 * n]]).contiguous(), torch.stack([rgb[:n], rgb[n:2 * n]]).contiguous()
    pred = PointSAMPredictor(model)
    pred.set_pointcloud(bx, br)
    rng = np.random.default_rng(2)
    bits = torch.from_numpy(G.words(rng.random((3, n)) < 0.2)).cuda()
    second = pred.mask_geometry(bits, cloud=1)
    _same_geometry(second, mask_geometry(bx[1], bits, br[1]))
    _same_geometry(pred.mask_geometry(bits), mask_geometry(bx[0], bits, br[0]))
    assert not torch.equal(second.centroid, pred.mask_geometry(bits).centroid)
    with pytest.raises(ValueError, match="words"):
        pred.mask_geometry(torch.zeros(1, ops.mask_words(n) + 1, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="cloud"):
        pred.mask_geometry(bits, cloud=2)
