"""One point-to-plane ICP step and its loop on the GPU (csrc/align_plane.hip, ops.align_plane_step, align.icp(normals=...), predictor.snapshot(normals=True)
/ align(plane=...)) against the plain numpy reference tests/align_plane_reference.py.  `nearest` and the three counts are always exact.  The other
sums are exact where every term is a short dyadic number (lattice coordinates, axis normals, a lattice translation: no addition rounds in any order)
and otherwise within M * 2^-53 * sum |term| of the exactly rounded sum: the first-order bound of M rounded additions -- tests/test_gpu_align.py's --
while a term of the device's sum passes through at most 6 + ceil(ceil(M / 64) / 32) + 32 of them.  The terms themselves are the reference's bit for
bit: the same fp64 operations in the same order, nothing contracted."""
import ctypes

import numpy as np
import pytest
import torch

import align_plane_reference as P
import align_reference as A
import transfer_reference as T
from point_sam_amd.config import get_config
from point_sam_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu
f32 = np.float32
U = 2.0 ** -53
COUNTS = [0, 30, 31]
SHIFT = np.array([[1, 0, 0, 3 / 64], [0, 1, 0, -1 / 64], [0, 0, 1, 2 / 64]], dtype=f32)      # a lattice translation: the posed coordinates stay dyadic


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd import ops
    return ops


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _pack(take, garbage=True):
    """[M] bool -> [ceil(M / 64)] int64 words in mask_pack's layout; the bits past M are SET (the entry must ignore them)."""
    M = len(take)
    pad = np.ones(-(-M // 64) * 64, dtype=bool) if garbage else np.zeros(-(-M // 64) * 64, dtype=bool)
    pad[:M] = take
    return (pad.reshape(-1, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(1, dtype=np.uint64).view(np.int64)


def _device_step(ops, index, nrm, qry, pose=None, radius=None, take=None, nearest=True):
    out = ops.align_plane_step(index, _dev(qry), nrm, pose, radius, None if take is None else _dev(_pack(take)), return_nearest=nearest)
    sums, near = out if nearest else (out, None)
    assert sums.dtype == torch.float64 and sums.shape == (32,) and sums.is_cuda
    if nearest:
        assert near.dtype == torch.int32 and near.shape == (len(qry),)
    return (None if near is None else near.cpu().numpy()), sums.cpu().numpy()


def _check_step(ops, src, nrm, r, qry, pose=None, radius=None, take=None, exact=False):
    """The device's step equals the reference's -> (nearest, sums) of the reference."""
    src, nrm, qry = (np.ascontiguousarray(v, dtype=f32) for v in (src, nrm, qry))
    want_near, want, mass = P.step(src, nrm, r, qry, pose, radius, take)
    near, got = _device_step(ops, ops.transfer_index(_dev(src), r), _dev(nrm), qry, pose, radius, take)
    bad = np.nonzero(near != want_near)[0]
    assert len(bad) == 0, (len(bad), bad[:5], near[bad[:5]], want_near[bad[:5]])
    assert not np.isnan(got).any(), got
    assert np.array_equal(got[COUNTS], want[COUNTS]) and got[0] + got[30] == (want_near >= 0).sum(), (got[COUNTS], want[COUNTS])
    err = np.abs(got - want)
    bound = np.zeros(32) if exact else len(qry) * U * mass
    print(f"M = {len(qry)}: used {int(got[0])}, unused {int(got[30])}, with a cell {int(got[31])}, max |error| / bound = "
          f"{'exact' if exact else float(np.max(err[1:30] / np.maximum(bound[1:30], 1e-300)))}")
    assert (err <= bound).all(), (np.nonzero(err > bound)[0], got, want, bound)
    return want_near, want


# ------------------------------------------------------------------------------------------------ the step
@pytest.mark.parametrize("pose,radius", [(None, None), (None, 0.125), (SHIFT, None)])
def test_lattice_case_is_exact(ops, pose, radius):
    """901 sources and 1543 queries on the 1/64 and 1/128 grids, r = 0.25, axis normals (a quarter of them zero), the identity or a lattice translation:
    every term is a short dyadic number, so all 32 words equal the reference's in any order of addition."""
    src, qry, r = T.lattice_case()
    near, sums = _check_step(ops, src, P.axis_normals(len(src), 5, zeros=0.25), r, qry, pose, radius, exact=True)
    assert sums[0] > 150 and sums[30] > 40 and sums[31] > sums[0] + sums[30] and (near < 0).sum() > 300
    if pose is None:
        assert np.array_equal(near, A.step(src, r, qry, None, radius)[0]) and sums[0] + sums[30] == (611 if radius is None else 373)      # align_step's pairs


@pytest.mark.parametrize("posed", [False, True])
def test_uniform_cloud_at_a_search_radius_below_the_indexs(ops, posed):
    src, qry = T.uniform_case()
    nrm = np.random.default_rng(12).normal(size=src.shape).astype(f32)                  # taken as given: not unit
    near, sums = _check_step(ops, src, nrm, 0.11, qry, T.POSE if posed else None, 0.07)
    assert (near >= 0).mean() > 0.3 and sums[0] == (near >= 0).sum() and sums[30] == 0 and sums[31] <= len(qry)
    if posed:
        _check_step(ops, src, nrm, 0.11, qry, T.POSE)                                    # and at the index's own


@pytest.mark.parametrize("N,M", [(1, 1), (5, 65), (5, 257), (901, 64 * 33 + 1), (901, 64 * 32 + 1)])
def test_one_pair_one_past_a_wave_one_past_a_block_and_a_ragged_last_segment(ops, N, M):
    """M = 64 * 33 + 1: 34 waves in segments of 2, the last segments empty; 64 * 32 + 1: 33 waves, the last segment holds one.  Rounded sums: the bound."""
    g = np.random.default_rng(100 + M)
    src = g.uniform(-0.5, 0.5, size=(N, 3)).astype(f32)
    qry = src[g.integers(0, N, size=M)] + g.normal(scale=0.05, size=(M, 3))            # where the queries land: beside a source
    pose = T.POSE if M > 1 else None
    if pose is not None:
        qry = (qry - pose[:, 3].astype(np.float64)) @ pose[:, :3].astype(np.float64)      # q = R^T (p - t): T.POSE is orthonormal
    qry = qry.astype(f32)
    nrm = g.normal(size=(N, 3)).astype(f32)
    near, sums = _check_step(ops, src, nrm, 0.25, qry, pose, 0.2)
    assert near.shape == (M,) and (sums[0] >= 1 if M == 1 else sums[0] > M // 8)
    # and exactly, on the lattice
    lsrc, lqry, r = T.lattice_case()
    lqry = np.concatenate([lsrc[:1], lqry, lqry + f32(0.5)], 0)[:M]
    _check_step(ops, lsrc[:N], P.axis_normals(N, 6), r, lqry, SHIFT if M > 1 else None, exact=True)


def test_zero_nan_and_infinite_normals_drop_out_and_are_counted(ops):
    src, qry = T.uniform_case()
    g = np.random.default_rng(13)
    nrm = g.normal(size=src.shape).astype(f32)
    nrm[g.uniform(size=len(src)) < 1 / 3] = 0                                            # what voxel_normals writes below min_points
    near = A.step(src, 0.11, qry, T.POSE, 0.07)[0]
    hit = np.unique(near[(near >= 0) & (np.abs(nrm[np.maximum(near, 0)]).sum(1) > 0)])
    nrm[hit[0]], nrm[hit[1]] = (np.nan, 0.5, 0.5), (0.5, -np.inf, 0.5)
    nrm[hit[2]], nrm[hit[3]] = (1e-30, 0, 0), (3e19, 1, 1)                                # nn underflows to 0, overflows to infinity, in fp32
    _, sums = _check_step(ops, src, nrm, 0.11, qry, T.POSE, 0.07)
    unused = ~P.used_normals(nrm)
    assert unused[hit[:4]].all() and sums[30] == unused[near[near >= 0]].sum() > 800 and sums[0] > 1500 and np.isfinite(sums).all()


def test_bits_select_an_irregular_subset(ops):
    """M = 1543 is no multiple of 64 and the bits past M are set: the result is the reference's restricted to the subset."""
    src, qry, r = T.lattice_case()
    nrm = P.axis_normals(len(src), 5, zeros=0.25)
    g = np.random.default_rng(8)
    take = g.uniform(size=len(qry)) < 0.37
    take[64:128] = False                                                               # a whole word, hence a whole wave, without a participant
    take[1536:] = [True, False, True, True, False, False, True]
    near, sums = _check_step(ops, src, nrm, r, qry, SHIFT, None, take, exact=True)
    assert (near[~take] == -1).all() and 0 < sums[0] < sums[0] + sums[30] < sums[31] <= take.sum()
    sub_near, sub, _ = P.step(src, nrm, r, qry[take], SHIFT)
    assert np.array_equal(sums, sub) and np.array_equal(near[take], sub_near)
    # posed, rounded sums: the bound; and all bits set is no bits at all
    usrc, uqry = T.uniform_case()
    unrm = g.normal(size=usrc.shape).astype(f32)
    utake = g.uniform(size=len(uqry)) < 0.5
    _check_step(ops, usrc, unrm, 0.11, uqry, T.POSE, 0.07, utake)
    index, dn = ops.transfer_index(_dev(usrc), 0.11), _dev(unrm)
    every = _device_step(ops, index, dn, uqry, T.POSE, take=np.ones(len(uqry), dtype=bool))
    none = _device_step(ops, index, dn, uqry, T.POSE)
    assert np.array_equal(every[0], none[0]) and np.array_equal(every[1].view(np.int64), none[1].view(np.int64))


def test_queries_without_a_cell_are_neither_paired_nor_counted(ops):
    src, qry, r = T.lattice_case()
    nrm = P.axis_normals(len(src), 5, zeros=0.25)
    odd = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e6, 0, 0], [-1e6, -1e6, 1e6], [np.nan, np.nan, np.nan]], dtype=f32)
    mixed = np.concatenate([odd[:3], qry[:700], odd[3:], qry[700:]], 0).astype(f32)
    near, sums = _check_step(ops, src, nrm, r, mixed, exact=True)
    plain_near, plain = P.step(src, nrm, r, qry)[:2]
    assert np.array_equal(sums, plain) and np.isfinite(sums).all()                     # the six add nothing, not even to sums[31]
    assert (near[:3] == -1).all() and (near[703:706] == -1).all() and np.array_equal(np.delete(near, [0, 1, 2, 703, 704, 705]), plain_near)


def test_queries_out_of_reach(ops):
    """Beyond the cell range: no query has a cell, all 32 words are zero.  In range but far from every source: 31 zeros and the count of queries with a cell."""
    src, qry, r = T.lattice_case()
    nrm = P.axis_normals(len(src), 5)
    index, dn = ops.transfer_index(_dev(src), r), _dev(nrm)
    near, sums = _device_step(ops, index, dn, (qry + f32(1e6)).astype(f32))
    assert (near == -1).all() and np.array_equal(sums, np.zeros(32)) and not np.signbit(sums).any()
    near, sums = _device_step(ops, index, dn, (qry + f32(100)).astype(f32))
    assert (near == -1).all() and np.array_equal(sums[:31], np.zeros(31)) and sums[31] == len(qry) and not np.signbit(sums).any()
    _check_step(ops, src, nrm, r, (qry + f32(100)).astype(f32), exact=True)


def test_duplicate_sources_at_a_tie_the_lower_index_wins_and_its_normal_is_used(ops):
    g = np.random.default_rng(3)
    src = (g.integers(0, 16, size=(300, 3)).astype(f32) / f32(64)).astype(f32)      # one cell of 0.25: a chain of 300, many exact duplicates
    src[0] = 0                                                                      # pins the origin: the cell is [0, 0.25)^3
    src[200:] = src[100:200]                                                        # every one of these twice
    nrm = P.axis_normals(300, 9)
    nrm[200:] = 0                                                                   # the later copy has no normal: were it the pair, the query would not be used
    qry = np.concatenate([(g.integers(-16, 32, size=(700, 3)).astype(f32) / f32(64)).astype(f32), src[200:] + np.array([1 / 256, 0, 0], dtype=f32)], 0)      # nearest to ONE position, held by two sources
    near, sums = _check_step(ops, src, nrm, 0.25, qry, exact=True)
    assert (near[700:] < 200).all() and (near[700:] >= 0).all()
    tied = np.array([len(np.nonzero((src == p).all(1))[0]) for p in src[near[700:]]])
    assert (tied >= 2).all() and np.array_equal(near[700:], [np.nonzero((src == p).all(1))[0][0] for p in src[near[700:]]])
    assert sums[30] == (np.abs(nrm[near[near >= 0]]).sum(1) == 0).sum()


def test_without_nearest_the_sums_are_the_same_words_and_two_calls_agree(ops):
    src, qry = T.uniform_case()
    dn = _dev(np.random.default_rng(14).normal(size=src.shape).astype(f32))
    a = ops.transfer_index(_dev(src), 0.11)
    b = ops.transfer_index(_dev(src), 0.11)                                            # another arrival order inside the chains
    runs = [_device_step(ops, ix, dn, qry, T.POSE, nearest=n)[1].view(np.int64) for ix, n in ((a, True), (a, True), (a, False), (b, False))]
    for other in runs[1:]:
        assert np.array_equal(runs[0], other)


def test_entry_refusals_leave_the_sums_untouched(ops):
    from point_sam_amd import _lib
    lib = _lib.load()
    src, qry, r = T.lattice_case()
    nrm = P.axis_normals(len(src), 5, zeros=0.25)
    index = ops.transfer_index(_dev(src), r)
    q, dn = _dev(qry), _dev(nrm)
    sums = torch.full((32,), -7.25, dtype=torch.float64, device="cuda")
    ws = torch.zeros(lib.psam_plane_workspace_bytes(len(qry)) // 8, dtype=torch.float64, device="cuda")
    org = (ctypes.c_float * 3)(*index.origin)
    stream = torch.cuda.current_stream().cuda_stream
    good = dict(src=index.src_xyz.data_ptr(), src_normals=dn.data_ptr(), N=len(src), index_ws=index.ws.data_ptr(), index_ws_bytes=index.ws.numel() * 8,
                origin=ctypes.addressof(org), inv_h=float(index.inv_h), r2=float(index.r2), qry=q.data_ptr(), M=len(qry), qry_bits=None, pose=None,
                nearest=None, sums=sums.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel() * 8)
    call = lambda **kw: lib.psam_plane_step(*{**good, **kw}.values(), stream)
    nan_pose = (ctypes.c_float * 12)(*([1.0] * 11 + [float("nan")]))
    for code, kw in ((-1, dict(r2=float("nan"))), (-1, dict(M=0)), (-1, dict(ws=None)), (-1, dict(src_normals=None)),
                     (-1, dict(pose=ctypes.addressof(nan_pose))), (-2, dict(qry=q.data_ptr() + 2)), (-2, dict(src_normals=dn.data_ptr() + 2)),
                     (-2, dict(sums=sums.data_ptr() + 4)), (-2, dict(index_ws=index.ws.data_ptr() + 8)), (-3, dict(ws_bytes=ws.numel() * 8 - 1)),
                     (-3, dict(ws_bytes=lib.psam_align_workspace_bytes(len(qry)))),
                     (-3, dict(index_ws_bytes=lib.psam_transfer_index_workspace_bytes(len(src)) - 1))):
        assert call(**kw) == code, (kw, lib.psam_last_error_string())
    torch.cuda.synchronize()
    assert bool((sums == -7.25).all())
    assert call() == 0
    want = P.step(src, nrm, r, qry)[1]
    assert np.array_equal(sums.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ the loop, on the fixture tests/test_align_plane_cpu.py verifies
# The reference loop's recorded errors against the truth, plus 1% plus 1e-6: the allowance for one fp32 pose word rounding the other way on the device.
ROTATION_MARGIN = P.REF_PLANE_ROTATION_ERROR * 1.01 + 1e-6
TRANSLATION_MARGIN = P.REF_PLANE_TRANSLATION_ERROR * 1.01 + 1e-6


def _config():
    from point_sam_amd.align import AlignConfig
    return AlignConfig(A.ICP_RADIUS, A.ICP_FINAL, A.ICP_SHRINK, A.ICP_ITERATIONS)


def _share(bits_a, bits_b, M):
    """Per row the share of the M points whose bit is the same in both."""
    x = (bits_a ^ bits_b).cpu().numpy().view(np.uint64)
    return 1 - np.array([sum(bin(int(w)).count("1") for w in row) for row in x]) / M


def _same_alignment(a, b):
    return (np.array_equal(a.pose.view(np.int64), b.pose.view(np.int64)) and (a.pairs, a.coverage, a.rms, a.iterations, a.converged, a.reason) ==
            (b.pairs, b.coverage, b.rms, b.iterations, b.converged, b.reason) and a.history == b.history)


def test_icp_on_the_device_follows_the_reference_loop(ops):
    """The same number of steps with the same pairs per step as the reference loop, converged by tolerance, as close to the TRUTH as the reference
    (REF_PLANE_* plus the margin above), and the carried masks agree with those under the true pose at the recorded share or better."""
    from point_sam_amd import align as X, transfer as S
    a, n, b = P.plane_case()
    src, nrm, qry = _dev(a), _dev(n), _dev(b)
    out = X.icp(ops.transfer_index(src, A.ICP_RADIUS), qry, _config(), normals=nrm)
    rot, tr = A.pose_error(out.pose)
    print(f"device point-to-plane ICP: {out.iterations} steps, pairs {[h[0] for h in out.history]}, coverage {out.coverage:.4f}, rms {out.rms:.4e}, "
          f"rotation error {rot:.4e} rad (margin {ROTATION_MARGIN:.4e}), translation error {tr:.4e} (margin {TRANSLATION_MARGIN:.4e}), {out.reason}")
    assert out.converged and out.reason == "tolerance" and out.iterations == len(out.history) == P.REF_PLANE_STEPS
    assert tuple(h[0] for h in out.history) == P.REF_PLANE_PAIRS and out.pairs == P.REF_PLANE_PAIRS[-1] and out.coverage == 1.0
    assert rot <= ROTATION_MARGIN and tr <= TRANSLATION_MARGIN
    assert out.history[0][2] == A.ICP_RADIUS and out.history[-1][2] == A.ICP_FINAL and 0 < out.rms < 2e-3
    assert _same_alignment(out, X.icp(ops.transfer_index(src, A.ICP_RADIUS), qry, _config(), normals=nrm, plane=X.PlaneConfig()))      # run to run
    rows = _dev(A.mask_rows(a))
    same = _share(*[S.transfer_bits(S.build_plan(src, qry, A.TRANSFER_RADIUS, pose), rows)[0] for pose in (A.TRUE_POSE, out.pose)], len(b))
    print(f"share of points with the same bit as under the true pose: {same.tolist()} (the reference loop's pose: {P.REF_PLANE_MASK_SHARE})")
    assert same.min() >= P.REF_PLANE_MASK_SHARE
    # without normals the loop is the point-to-point one: 20 words per step, a fixed point after many more steps
    plain = X.icp(ops.transfer_index(src, A.ICP_RADIUS), qry, _config())
    assert plain.converged and plain.reason == "fixed point" and plain.iterations >= 4 * out.iterations


# ------------------------------------------------------------------------------------------------ the predictor
@pytest.fixture(scope="module")
def scans(ops):
    """The fixture's cloud A as a scene with a snapshot of two objects WITH normals, then cloud B as the current scene; both are their own working clouds."""
    from point_sam_amd.model import PointCloudSAM
    from point_sam_amd.predictor import PointSAMPredictor
    cfg = get_config("tiny")
    pred = PointSAMPredictor(PointCloudSAM(cfg, random_state_dict(cfg, 3), "cuda", precision="f16x3"))
    a, b = A.icp_case()
    axyz, bxyz = _dev(a), _dev(b)
    pred.set_scene(axyz, torch.full_like(axyz, 0.5), max_points=8192)
    rows = _dev(A.mask_rows(a))
    snap, bare = pred.snapshot(rows, normals=True), pred.snapshot(rows)
    want = pred.point_normals()[0].index_select(0, pred.scene.keep_idx)
    assert torch.equal(snap.coords, axyz) and bare.normals is None and torch.equal(bare.coords, snap.coords) and torch.equal(bare.logits, snap.logits)
    pred.set_scene(bxyz, torch.full_like(bxyz, 0.5), max_points=8192)
    assert torch.equal(pred._state.coords[0], bxyz)
    return pred, snap, bare, bxyz, want


def test_snapshot_normals_are_the_point_normals_of_the_working_points(ops, scans):
    from point_sam_amd.superpoints import SuperpointConfig
    pred, snap, _, bxyz, want = scans
    n = snap.normals
    assert n.dtype == torch.float32 and n.shape == (6000, 3) and n.is_cuda and n.is_contiguous() and torch.equal(n.view(torch.int32), want.view(torch.int32))
    length = n.double().norm(dim=1)
    assert bool(((length - 1).abs() < 1e-6).logical_or(length == 0).all()) and int((length > 0).sum()) > 5000
    # against the analytic normals of the fixture: most voxel normals lie within 10 degrees of them, either sign
    cos = (n.double() * _dev(P.analytic_normals(A.icp_case()[0])).double()).sum(1).abs()[length > 0]
    assert float((cos > np.cos(np.radians(10.0))).double().mean()) > 0.8
    # the current cloud (B, its own working cloud) with a SuperpointConfig; a scan-width mask row keeps working
    cfg = SuperpointConfig(min_points=8, voxel_size=0.05)
    now = pred.snapshot(torch.zeros(1, len(bxyz), device="cuda"), normals=cfg)
    assert torch.equal(now.normals.view(torch.int32), pred.point_normals(cfg=cfg)[0].index_select(0, pred.scene.keep_idx).view(torch.int32))
    assert not torch.equal(now.normals, pred.snapshot(torch.zeros(1, len(bxyz), device="cuda"), normals=True).normals)
    with pytest.raises(TypeError, match="SuperpointConfig"):
        pred.snapshot(torch.zeros(1, len(bxyz), device="cuda"), normals="yes")


def test_snapshot_normals_of_a_downsampled_scene_and_of_a_plain_cloud(ops, scans):
    from point_sam_amd.predictor import PointSAMPredictor
    pred = PointSAMPredictor(scans[0].model)
    axyz = _dev(A.icp_case()[0])
    pred.set_scene(axyz, torch.full_like(axyz, 0.5), max_points=2048)                    # a working cloud smaller than the scan
    Nw = pred.scene.num_working
    assert 512 <= Nw <= 2048 and not pred.scene.identity
    snap = pred.snapshot(torch.zeros(1, len(axyz), device="cuda"), normals=True)
    assert snap.normals.shape == (Nw, 3) and torch.equal(snap.normals, pred.point_normals()[0][pred.scene.keep_idx]) and snap.coords.shape == (Nw, 3)
    pred.set_pointcloud(axyz[None, :2048], torch.full_like(axyz[None, :2048], 0.5))        # no scene: the cloud's own rows
    snap = pred.snapshot(torch.zeros(1, 2048, device="cuda"), normals=True)
    assert snap.normals.shape == (2048, 3) and torch.equal(snap.normals, pred.point_normals()[0])


def test_predictor_align_plane_equals_icp_composed_from_public_calls(ops, scans):
    from point_sam_amd import align as X
    pred, snap, bare, bxyz, _ = scans
    init = np.concatenate([A.rotation([0, 0, 1], 1.0), [[0.01], [0.0], [0.0]]], 1)
    take = torch.zeros(ops.mask_words(len(bxyz)), dtype=torch.int64, device="cuda")
    take[:40] = -1                                                                     # the first 2560 working points
    loose = X.PlaneConfig(1e-4, 1e-4, 1e-8)
    for plane, kw in ((True, dict()), (True, dict(init=init)), (loose, dict(mask=take))):
        got = pred.align(snap, _config(), plane=plane, **kw)
        want = X.icp(ops.transfer_index(snap.coords, A.ICP_RADIUS), pred._state.coords[0].contiguous(), _config(), kw.get("init"), kw.get("mask"),
                     normals=snap.normals, plane=None if plane is True else plane)
        assert _same_alignment(got, want), kw
        assert got.pose.shape == (3, 4) and got.pose.dtype == np.float64 and got.search is None
    full = pred.align(snap, _config(), plane=True)
    rot, tr = A.pose_error(full.pose)
    print(f"predictor.align(plane=True) on voxel normals: {full.iterations} steps, pairs {[h[0] for h in full.history]}, {full.reason}, rotation error "
          f"{rot:.4e} rad, translation error {tr:.4e}")
    # voxel normals are estimates: the answer is held against point-to-point's recorded errors, which it must still beat, in a quarter of its steps
    assert full.converged and full.reason == "tolerance" and full.iterations <= 10 and rot < A.REF_ROTATION_ERROR and tr < A.REF_TRANSLATION_ERROR
    # the pose passes straight to transfer_masks
    est, _, covered = pred.transfer_masks(snap, A.TRANSFER_RADIUS, full.pose)
    true, _, _ = pred.transfer_masks(snap, A.TRANSFER_RADIUS, A.TRUE_POSE)
    assert _share(est, true, len(bxyz)).min() >= A.REF_MASK_SHARE and int(covered) > 0.99 * len(bxyz)


def test_predictor_align_plane_needs_normals_and_without_plane_answers_as_before(ops, scans):
    from point_sam_amd import align as X
    pred, snap, bare, bxyz, _ = scans
    for plane in (True, X.PlaneConfig()):
        with pytest.raises(ValueError, match=r"snapshot\(\.\.\., normals=True\)"):
            pred.align(bare, _config(), plane=plane)
    with pytest.raises(TypeError, match="PlaneConfig"):
        pred.align(snap, _config(), plane={"condition": 1e-6})
    # plane=None: the point-to-point run of align.icp, whether or not the snapshot carries normals
    want = X.icp(ops.transfer_index(bare.coords, A.ICP_RADIUS), pred._state.coords[0].contiguous(), _config())
    assert want.converged and want.reason == "fixed point" and want.iterations > 20
    for s in (bare, snap):
        assert _same_alignment(pred.align(s, _config()), want) and _same_alignment(pred.align(s, _config(), plane=None), want)


def test_predictor_align_plane_with_search_returns_a_converged_pose(ops, scans):
    from point_sam_amd import align as X
    pred, snap, _, bxyz, _ = scans
    search = X.SearchConfig(rotations="yaw", yaw_steps=8, sample=512, keep=2)
    got = pred.align(snap, _config(), search=search, plane=True)
    want = X.search(ops.transfer_index(snap.coords, A.ICP_RADIUS), pred._state.coords[0].contiguous(), search, _config(), normals=snap.normals,
                    plane=X.PlaneConfig())
    assert _same_alignment(got, want) and got.search.poses == 8 and len(got.search.candidates) == 2
    rot, tr = A.pose_error(got.pose)
    print(f"search + point-to-plane: {got.iterations} steps, {got.pairs} pairs, {got.reason}, rotation error {rot:.4e} rad, translation error {tr:.4e}, "
          f"candidates {got.search.candidates}")
    assert got.converged and got.reason == "tolerance" and got.pairs > 6000 and rot < A.REF_ROTATION_ERROR and tr < A.REF_TRANSLATION_ERROR
