"""Scan map relocalisation on the GPU (csrc/track_score.hip, ops.track_score, ScanMap.track_score / relocalize / anchors,
predictor.map_relocalize) against the plain numpy reference tests/track_score_reference.py.  Counts are integers: every comparison of counts is
EXACT.  The C entry is called with `counts` and the workspace between guard words, and the map's block is compared bit for bit before and after: a
scoring only reads it.  Maps are built on the device with ScanMap.add from the same points the RefMap got."""
import ctypes

import numpy as np
import pytest
import torch

import align_reference as AR
import align_search_reference as ASR
import scanmap_reference as SM
import track_reference as TR
import track_score_reference as R
from point_sam_amd.config import get_config
from point_sam_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD_WORDS = 256
COUNT_GUARD, WS_GUARD = -77, 0x5A5A5A5A5A5A5A5A
POSES7 = R.seven_poses()
IDENTITY = POSES7[0]
H = TR.H


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd import ops
    return ops


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pack(take):
    n = len(take)
    pad = np.zeros(-(-n // 64) * 64, dtype=bool)
    pad[:n] = take
    return (pad.reshape(-1, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(1, dtype=np.uint64).view(np.int64)


def _device_map(h, max_voxels, adds):
    """-> (ScanMap on the device, RefMap): the adds in order, each under the identity; the ids of every add agree."""
    from point_sam_amd.scanmap import ScanMap
    m, ref = ScanMap(h, max_voxels), SM.RefMap(h, max_voxels)
    for pts in adds:
        pts = np.ascontiguousarray(pts, dtype=f32).reshape(-1, 3)
        got = m.add(_dev(pts), _dev(np.zeros_like(pts)))
        assert np.array_equal(got.ids.cpu().numpy(), ref.add(pts, np.zeros_like(pts))[0])
    assert m.num_voxels == ref.V
    return m, ref


_maps = {}


def _shared_map(case):
    key = (case["h"], case["max_voxels"]) + tuple(a.tobytes() for a in case["adds"])
    if key not in _maps:
        _maps[key] = _device_map(case["h"], case["max_voxels"], case["adds"])
    return _maps[key]


def _raw_score(m, qry, poses, r2, reach, V=None, skip=None, min_count=1, counts=None, ws=None, status=0):
    """psam_relocalize_score itself: `counts` and the workspace lie between guard words that stay intact, and the map's block is bit for bit what it
    was -> counts [P] int64.  counts / ws: buffers of an earlier call to use again."""
    from point_sam_amd import _lib, ops
    lib = _lib.load()
    q = _dev(np.ascontiguousarray(qry, dtype=f32))
    words = poses if isinstance(poses, torch.Tensor) else _dev(ops.transfer_poses(poses))
    M, P = len(qry), words.shape[0]
    V = m.num_voxels if V is None else V
    n_ws = lib.psam_relocalize_workspace_bytes(V) // 8
    assert n_ws == 2 * V
    if counts is None:
        counts = torch.full((P + 2 * GUARD_WORDS,), COUNT_GUARD, dtype=torch.int32, device="cuda")
    if ws is None:
        ws = torch.full((n_ws + 2 * GUARD_WORDS,), WS_GUARD, dtype=torch.int64, device="cuda")
    skipw = None if skip is None else _dev(_pack(np.asarray(skip, dtype=bool)[:V]))
    before = m._block.clone()
    st = lib.psam_relocalize_score(m._block.data_ptr(), m._block.numel() * 8, m.max_voxels, m.max_pairs, V, None if skipw is None else skipw.data_ptr(),
                                   min_count, reach, float(r2), q.data_ptr(), M, words.data_ptr(), P, counts[GUARD_WORDS:].data_ptr(),
                                   ws[GUARD_WORDS:].data_ptr(), n_ws * 8, torch.cuda.current_stream().cuda_stream)
    assert st == status, lib.psam_last_error_string()
    torch.cuda.synchronize()
    assert torch.equal(m._block, before), "the map block is only read"
    c, w = counts.cpu().numpy(), ws.cpu().numpy()
    assert (c[:GUARD_WORDS] == COUNT_GUARD).all() and (c[GUARD_WORDS + P:] == COUNT_GUARD).all(), "a guard word around counts was written"
    assert (w[:GUARD_WORDS] == WS_GUARD).all() and (w[GUARD_WORDS + n_ws:] == WS_GUARD).all(), "a guard word around the workspace was written"
    return c[GUARD_WORDS:GUARD_WORDS + P].astype(np.int64)


def _check(m, ref, qry, poses, radius, reach=None, r2=None, V=None, skip=None, min_count=1):
    """The device's counts equal the reference's, word for word -> the counts."""
    reach = TR.reach_of(radius, 1.0 / float(ref.inv_h)) if reach is None else reach
    r2 = TR.r2_of(radius) if r2 is None else r2
    want = R.score(ref, qry, poses, radius, reach, r2, V, skip, min_count)
    got = _raw_score(m, qry, poses, r2, reach, V, skip, min_count)
    assert np.array_equal(got, want), (np.nonzero(got != want)[0][:8], got[:8], want[:8])
    return got


# ------------------------------------------------------------------------------------------------ 1: the cases of the step
@pytest.mark.parametrize("case", TR.cases() + [TR.lattice_case()], ids=lambda c: c["name"])
def test_counts_equal_the_reference_on_every_case_of_the_step(ops, case):
    """The case's own pose and bits are not used: a scoring takes the seven poses and every query."""
    m, ref = _shared_map(case)
    radius = case.get("radius", case["h"])
    got = _check(m, ref, case["qry"], POSES7, radius, case.get("reach"), None, case.get("V"), case.get("skip"), case.get("min_count", 1))
    print(f"{case['name']}: M = {len(case['qry'])}, V = {ref.V}: counts {got.tolist()}")
    assert got[3] == 0, "a translation of 3e6 leaves the map"


# ------------------------------------------------------------------------------------------------ 2: shapes
@pytest.fixture(scope="module")
def rand(ops):
    case = TR.random_case(0)
    m, ref = _device_map(case["h"], case["max_voxels"], case["adds"])
    g = np.random.default_rng(3)
    qry = np.concatenate([TR.means(ref)[:1], case["qry"], g.uniform(-0.95, 0.95, size=(400, 3)).astype(f32)], 0)      # the first query sits on a voxel's mean
    return m, ref, qry, case["h"]


def _poses(P, seed=4):
    """P rigid poses: the seven named ones first (pose 3 sends every query away), then random rotations with small translations."""
    g = np.random.default_rng(seed)
    out = list(POSES7)
    while len(out) < P:
        out.append(np.concatenate([AR.rotation(g.normal(size=3), float(g.uniform(0, 360))), g.uniform(-0.1, 0.1, size=(3, 1))], 1))
    return np.stack(out[:P])


@pytest.mark.parametrize("M,P", [(1, 1), (63, 1), (64, 2), (65, 1), (257, 3), (1025, 2)])
def test_shapes_around_a_wave_and_a_workgroup(ops, rand, M, P):
    m, ref, qry, h = rand
    assert len(qry) >= 1025
    got = _check(m, ref, qry[:M], _poses(P), h)
    assert got[0] >= 1


@pytest.mark.parametrize("dP", [-1, 0, 1])
def test_pose_counts_around_a_chunk(ops, rand, dP):
    m, ref, qry, h = rand
    P = ops.TRACK_SCORE_POSES + dP
    got = _check(m, ref, qry[:130], _poses(P), h)
    hits = np.arange(P) != 3
    assert len(got) == P and (got[~hits] == 0).all() and (got[hits] > 0).all()


def test_several_chunks_the_last_one_short_and_a_pose_in_the_middle_that_scores_a_written_zero(ops, rand):
    m, ref, qry, h = rand
    P = 8 * ops.TRACK_SCORE_POSES + 1
    poses = _poses(P)
    poses[17] = POSES7[3]                                          # every query leaves [-1, 1]^3
    got = _check(m, ref, qry[:130], poses, h)
    assert (got[[3, 17]] == 0).all() and (np.delete(got, [3, 17]) > 0).all()


# ------------------------------------------------------------------------------------------------ 3: the corner cells of the cube
CELL = 8                                                           # the query's cell on every axis; h = 2^-3: cells 4 .. 12 lie inside [0, 16)


def _corner_setup(sign, reach):
    """The query sits 0.05 h inside the corner of its own cell that faces the cube's corner cell `sign`; the one pairable voxel sits 0.05 h inside
    that corner cell, (reach - 0.9) h away on every axis; r2 is 1.1 x that squared distance.  Fillers, all OUT of that radius: one voxel in each of
    the seven other corner cells of the cube, at the cell's far end (at least (reach + 0.9) h away on one axis and reach h on the others), and at
    reach 1 one in the far corner of the query's own cell (0.9 h away on every axis).  At reach 2 and 4 no point of the query's own cell can be
    out of radius while the corner voxel is in: the corner voxel is at least (reach - 1) h away on every axis, a point of the own cell at most h.
    -> (query [1, 3], corner voxel [1, 3], fillers [n, 3], r2)"""
    s = np.asarray(sign, dtype=np.float64)
    lo = (s < 0)
    q = (CELL + np.where(lo, 0.05, 0.95)) * H - 1.0
    corner = (CELL + s * reach + np.where(lo, 0.95, 0.05)) * H - 1.0
    fill = []
    for t in np.ndindex(2, 2, 2):
        t = np.asarray(t) * 2.0 - 1.0
        if not np.array_equal(t, s):
            fill.append((CELL + t * reach + np.where(t < 0, 0.05, 0.95)) * H - 1.0)
    if reach == 1:
        fill.append((CELL + np.where(lo, 0.95, 0.05)) * H - 1.0)
    r2 = f32(1.1 * 3.0 * ((reach - 0.9) * H) ** 2)
    return q[None].astype(f32), corner[None].astype(f32), np.array(fill, dtype=f32), r2


@pytest.mark.parametrize("reach", [1, 2, 4])
@pytest.mark.parametrize("sign", [(a, b, c) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)], ids=lambda s: "".join("+" if v > 0 else "-" for v in s))
def test_the_only_pairable_voxel_sits_in_a_corner_cell_of_the_cube(ops, sign, reach):
    q, corner, fill, r2 = _corner_setup(sign, reach)
    with_it, ref_with = _device_map(H, 64, [fill, corner])
    without, ref_without = _device_map(H, 64, [fill])
    cell = lambda p: np.floor((p.astype(np.float64) + 1.0) / H).astype(int)
    assert np.array_equal(cell(corner[0]) - cell(q[0]), np.asarray(sign) * reach) and ref_with.V == len(fill) + 1
    assert _check(with_it, ref_with, q, IDENTITY[None], None, reach, r2)[0] == 1
    assert _check(without, ref_without, q, IDENTITY[None], None, reach, r2)[0] == 0
    if reach > 1:                                                  # one cell short of the corner: the voxel is outside the cube
        assert _check(with_it, ref_with, q, IDENTITY[None], None, reach - 1, r2)[0] == 0


@pytest.mark.parametrize("reach", [1, 2, 4])
def test_the_only_pairable_voxel_sits_in_the_querys_own_cell(ops, reach):
    q, _, fill, _ = _corner_setup((1, 1, 1), reach)
    own = (q + f32(-0.05 * H)).astype(f32)                         # 0.05 h from the query on every axis, in its cell
    fill = fill[:7]                                                # the seven other corner cells; the own cell holds `own` alone
    r2 = f32((0.2 * H) ** 2)
    with_it, ref_with = _device_map(H, 64, [fill, own])
    without, ref_without = _device_map(H, 64, [fill])
    assert ref_with.locate(q)[0] == ref_with.V - 1 == 7
    assert _check(with_it, ref_with, q, IDENTITY[None], None, reach, r2)[0] == 1
    assert _check(without, ref_without, q, IDENTITY[None], None, reach, r2)[0] == 0


# ------------------------------------------------------------------------------------------------ 4: the first candidate, not the first voxel
def test_a_nearer_voxel_that_is_not_allowed_does_not_end_the_walk(ops):
    """Voxel 0 (two points, in the query's own cell, nearer), voxel 1 (three points, the next cell, farther), both within the radius."""
    base = (CELL + 0.5) * H - 1.0
    near = np.array([[base + 0.30 * H, base, base], [base + 0.32 * H, base, base]], dtype=f32)
    far = np.array([[base + 0.6 * H, base, base]] * 3, dtype=f32)
    q = np.array([[base, base, base]], dtype=f32)
    m, ref = _device_map(H, 64, [near, far])
    assert ref.V == 2 and list(ref.count) == [2, 3] and ref.locate(q)[0] == 0
    one = IDENTITY[None]
    for reach in (1, 2, 4):
        assert _check(m, ref, q, one, H, reach)[0] == 1
        assert _check(m, ref, q, one, H, reach, skip=[True, False])[0] == 1, "the nearer one skipped: the farther one is the candidate"
        assert _check(m, ref, q, one, H, reach, skip=[True, True])[0] == 0
        assert _check(m, ref, q, one, H, reach, skip=[False, True])[0] == 1
        assert _check(m, ref, q, one, H, reach, min_count=3)[0] == 1, "the nearer one too sparse"
        assert _check(m, ref, q, one, H, reach, min_count=4)[0] == 0
        assert _check(m, ref, q, one, H, reach, V=1)[0] == 1 and _check(m, ref, q, one, H, reach, V=1, skip=[True])[0] == 0
    skip = _dev(_pack(np.array([True, False])))
    assert m.track_score(_dev(q), one, H, skip).tolist() == [1] and m.track_score(_dev(q), one, H, skip, 4).tolist() == [0]


# ------------------------------------------------------------------------------------------------ 5: q == r2
def test_a_hit_at_q_equal_r2_counts_and_one_step_below_it_does_not(ops):
    """One voxel at (0, 0, 0) exactly, the query at (0.25, 0, 0): q = 0.0625 = fl32(0.25^2).  The bound one fp32 step lower goes through the C
    entry, which takes r2 itself."""
    m, ref = _device_map(H, 64, [np.zeros((1, 3), dtype=f32), np.full((1, 3), 0.9, dtype=f32)])
    assert np.array_equal(TR.means(ref)[0], np.zeros(3, dtype=f32))
    qry = np.array([[0.25, 0, 0], [0.5, 0.5, 0.5]], dtype=f32)
    assert m.track_score(_dev(qry), IDENTITY[None], 0.25).tolist() == [1]
    assert _check(m, ref, qry, IDENTITY[None], 0.25, 2, f32(0.0625))[0] == 1
    assert _check(m, ref, qry, IDENTITY[None], 0.25, 2, np.nextafter(f32(0.0625), f32(0)))[0] == 0


# ------------------------------------------------------------------------------------------------ 6: track_step's pairs, pose by pose
@pytest.fixture(scope="module")
def loop(ops):
    ref, a, b = TR.loop_case()
    m, _ = _device_map(TR.LOOP_H, TR.LOOP_MAX_VOXELS, [a])
    return m, ref, _dev(b), b


@pytest.mark.parametrize("radius", [TR.LOOP_RADIUS, TR.LOOP_FINAL])
def test_counts_equal_track_steps_pairs_pose_by_pose(ops, loop, radius):
    m, ref, qry, b = loop
    g = np.random.default_rng(12)
    poses = np.stack([np.concatenate([AR.rotation(g.normal(size=3), float(g.uniform(0, 3))) @ AR.TRUE_POSE[:, :3],
                                      (AR.TRUE_POSE[:, 3] + g.uniform(-0.05, 0.05, size=3))[:, None]], 1) for _ in range(40)])
    poses[0] = AR.TRUE_POSE
    skip_rows = g.uniform(size=ref.V) < 0.3
    for skip, min_count in ((None, 1), (skip_rows, 2)):
        words = None if skip is None else _dev(_pack(skip))
        got = m.track_score(qry, poses, radius, words, min_count).cpu().numpy()
        want = [int(m.track_step(qry, p, radius, None, words, min_count)[0]) for p in poses]
        assert got.tolist() == want and got[0] > 1000, (got, want)
    assert np.array_equal(m.track_score(qry, poses[:5], radius).cpu().numpy(), R.score(ref, b, poses[:5], radius))


# ------------------------------------------------------------------------------------------------ 7: queries and poses that are not finite
def test_queries_without_a_cell_disturb_no_count_and_a_pose_row_of_nan_scores_zero(ops, rand):
    m, ref, qry, h = rand
    odd = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e7, 0, 0], [-1e7, -1e7, 1e7], [np.nan, np.nan, np.nan]], dtype=f32)
    mixed = np.concatenate([odd[:3], qry[:700], odd[3:], qry[700:]], 0).astype(f32)
    poses = _poses(9)
    assert np.array_equal(_check(m, ref, mixed, poses, h), _check(m, ref, qry, poses, h))
    words = ops.transfer_poses(poses).copy()
    words[2, 5] = np.nan
    words[6, 11] = np.inf
    got = m.track_score(_dev(qry), _dev(words), h).cpu().numpy()
    want = _check(m, ref, qry, poses, h)
    assert got[2] == 0 and got[6] == 0 and np.array_equal(np.delete(got, [2, 6]), np.delete(want, [2, 6]))


# ------------------------------------------------------------------------------------------------ 8: refusals, and clearing
def test_refusals_leave_counts_untouched_and_an_accepted_call_overwrites_its_own_answer(ops, rand):
    from point_sam_amd import _lib
    lib = _lib.load()
    m, ref, qry, h = rand
    q, words = _dev(qry[:200]), _dev(ops.transfer_poses(_poses(6)))
    V = m.num_voxels
    counts = torch.full((6,), COUNT_GUARD, dtype=torch.int32, device="cuda")
    ws = torch.empty(2 * V, dtype=torch.int64, device="cuda")
    good = dict(map=m._block.data_ptr(), map_bytes=m._block.numel() * 8, mv=m.max_voxels, mp=m.max_pairs, V=V, skip=None, min_count=1, reach=1,
                r2=float(TR.r2_of(h)), qry=q.data_ptr(), M=200, poses=words.data_ptr(), P=6, counts=counts.data_ptr(), ws=ws.data_ptr(), ws_bytes=16 * V)

    def call(**change):
        a = dict(good, **change)
        st = lib.psam_relocalize_score(a["map"], a["map_bytes"], a["mv"], a["mp"], a["V"], a["skip"], a["min_count"], a["reach"], a["r2"], a["qry"], a["M"],
                                       a["poses"], a["P"], a["counts"], a["ws"], a["ws_bytes"], torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return st
    for change, code in ((dict(map=None), -1), (dict(qry=None), -1), (dict(poses=None), -1), (dict(ws=None), -1), (dict(M=0), -1), (dict(V=0), -1),
                         (dict(V=m.max_voxels + 1), -1), (dict(reach=0), -1), (dict(reach=5), -1), (dict(min_count=0), -1), (dict(r2=0.0), -1),
                         (dict(r2=float("nan")), -1), (dict(P=0), -1), (dict(P=(1 << 20) + 1), -1), (dict(map=good["map"] + 8), -2), (dict(ws=good["ws"] + 8), -2),
                         (dict(qry=good["qry"] + 2), -2), (dict(poses=good["poses"] + 1), -2), (dict(map_bytes=good["map_bytes"] // 2), -3),
                         (dict(ws_bytes=16 * V - 1), -3)):
        assert call(**change) == code and lib.psam_last_error_string().decode().startswith("psam_relocalize_score"), change
        assert (counts == COUNT_GUARD).all(), change
    assert call(counts=None) == -1 and call(counts=good["counts"] + 2) == -2
    assert call() == 0
    first = counts.clone()
    assert np.array_equal(first.cpu().numpy(), R.score(ref, qry[:200], _poses(6), h))
    assert call() == 0 and torch.equal(counts, first), "it clears, it does not add"


# ------------------------------------------------------------------------------------------------ 9, 10: the means table, run to run
def test_the_means_table_is_rebuilt_after_the_map_has_grown_and_skip_has_changed(ops):
    case = TR.random_case(2, n_map=600, n_qry=300)
    m, ref = _device_map(case["h"], case["max_voxels"], case["adds"][:1])
    poses, r2 = _poses(5), TR.r2_of(case["h"])
    counts = torch.full((5 + 2 * GUARD_WORDS,), COUNT_GUARD, dtype=torch.int32, device="cuda")
    grown = SM.RefMap(case["h"], case["max_voxels"])
    for pts in case["adds"]:
        grown.add(pts, np.zeros_like(pts))
    ws = torch.full((2 * grown.V + 2 * GUARD_WORDS,), WS_GUARD, dtype=torch.int64, device="cuda")
    ws[GUARD_WORDS + 2 * ref.V:] = WS_GUARD
    first = _raw_score(m, case["qry"], poses, r2, 1, counts=counts, ws=torch.cat([ws[:GUARD_WORDS + 2 * ref.V], ws[-GUARD_WORDS:]]))
    assert np.array_equal(first, R.score(ref, case["qry"], poses, case["h"]))
    pts = case["adds"][1]
    m.add(_dev(pts), _dev(np.zeros_like(pts)))
    assert m.num_voxels == grown.V > ref.V and max(grown.count) > 1, "new voxels, and old ones whose mean has moved"
    second = _raw_score(m, case["qry"], poses, r2, 1, counts=counts, ws=ws)
    assert np.array_equal(second, R.score(grown, case["qry"], poses, case["h"])) and not np.array_equal(first, second)
    skip = np.arange(grown.V) % 2 == 0
    third = _raw_score(m, case["qry"], poses, r2, 1, skip=skip, counts=counts, ws=ws)
    assert np.array_equal(third, R.score(grown, case["qry"], poses, case["h"], skip=skip)) and (third <= second).all() and third.sum() < second.sum()
    assert np.array_equal(_raw_score(m, case["qry"], poses, r2, 1, counts=counts, ws=ws), second), "and back"


def test_two_runs_give_identical_words(ops, rand):
    m, ref, qry, h = rand
    poses, q = _poses(41), _dev(qry)
    a, b = m.track_score(q, poses, 2 * h), m.track_score(q, poses, 2 * h)
    assert a.dtype == torch.int32 and a.shape == (41,) and a.is_cuda and torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), R.score(ref, qry, poses, 2 * h))
    four = np.stack([np.concatenate([p, [[0.0, 0.0, 0.0, 1.0]]], 0) for p in poses])      # 4 x 4 rows, a host tensor, the words on the device
    assert torch.equal(m.track_score(q, four, 2 * h), a) and torch.equal(m.track_score(q, torch.from_numpy(four), 2 * h), a)
    assert torch.equal(m.track_score(q, _dev(ops.transfer_poses(poses)), 2 * h), a)


def test_a_dead_map_and_an_empty_map_raise(ops):
    from point_sam_amd.scanmap import MapOverflow, ScanMap
    m = ScanMap(H, 64)
    q = torch.zeros(4, 3, device="cuda")
    with pytest.raises(ValueError, match="empty"):
        m.track_score(q, IDENTITY[None])
    with pytest.raises(ValueError, match="empty"):
        m.anchors()
    m._flags = 1
    with pytest.raises(MapOverflow):
        m.track_score(q, IDENTITY[None])


# ------------------------------------------------------------------------------------------------ anchors
def test_anchors_on_the_device_equal_the_reference(ops, loop):
    m, ref, _, _ = loop
    keys, means = np.asarray(ref.keys, dtype=np.int64), TR.means(ref)
    for cells, min_voxels, min_count in ((8, 8, 1), (4, 3, 1), (2, 1, 2), (16, 1, 1)):
        got = m.anchors(cells, None, min_count, min_voxels)
        want = R.anchors(keys, means, R.pairable(ref, None, min_count), cells, min_voxels)
        assert got.dtype == np.float64 and got.shape == want.shape and len(want) >= 1 and np.array_equal(got, want), (cells, min_voxels)
    occupied = np.arange(ref.V) % 3 != 0
    assert np.array_equal(m.anchors(4, _dev(occupied), 1, 2), R.anchors(keys, means, R.pairable(ref, occupied), 4, 2))
    assert np.array_equal(m.anchors(occupied=True), m.anchors()), "never carved: everything is occupied"


# ------------------------------------------------------------------------------------------------ 11: the search
ROTATION_MARGIN, TRANSLATION_MARGIN = 10 * R.REF_ROTATION_ERROR, 10 * R.REF_TRANSLATION_ERROR


@pytest.fixture(scope="module")
def fixture(ops):
    ref, a, b = R.search_case()
    m, _ = _device_map(R.SEARCH_H, R.SEARCH_MAX_VOXELS, [a])
    assert m.num_voxels == R.SEARCH_VOXELS and len(b) == R.SEARCH_QUERIES
    return m, ref, _dev(b), b


def _configs(**more):
    from point_sam_amd.align import AlignConfig, SearchConfig
    return AlignConfig(**ASR.ICP), SearchConfig(rotations="yaw", yaw_steps=ASR.YAW_STEPS, offsets=ASR.YAW_OFFSETS, offset_step=ASR.YAW_OFFSET_STEP,
                                                sample=ASR.SAMPLE, radius=ASR.SCORE_RADIUS, keep=ASR.KEEP, **more)


def _same_alignment(x, y):
    return (np.array_equal(x.pose, y.pose) and (x.pairs, x.coverage, x.iterations, x.converged, x.reason) == (y.pairs, y.coverage, y.iterations, y.converged, y.reason)
            and (x.rms == y.rms or (np.isnan(x.rms) and np.isnan(y.rms))) and x.history == y.history and
            (x.search is None) == (y.search is None) and (x.search is None or (x.search.poses, x.search.sample, x.search.chosen, repr(x.search.candidates)) ==
                                                          (y.search.poses, y.search.sample, y.search.chosen, repr(y.search.candidates))))


def test_the_grid_of_the_fixture_scores_as_the_reference(ops, fixture):
    m, ref, qry, b = fixture
    poses, picked = R.search_poses(ref, b)
    assert len(poses) == R.SEARCH_POSES
    got = m.track_score(_dev(b[picked]), poses, ASR.SCORE_RADIUS).cpu().numpy().astype(np.int64)
    order = ASR.ordered(got, ASR.KEEP)
    assert order == R.SEARCH_ORDER and [int(got[p]) for p in order] == R.SEARCH_COUNTS and int(np.median(got)) == R.SEARCH_MEDIAN
    some = np.concatenate([np.asarray(order), np.arange(0, R.SEARCH_POSES, 97)])
    assert np.array_equal(got[some], R.score(ref, b[picked], poses[some], ASR.SCORE_RADIUS))


def test_search_on_the_device_finds_the_pose_plain_tracking_does_not(ops, fixture):
    """The query and source centroids come from a device fp64 mean, the reference's from numpy's; the eight indices and counts are asserted as
    recorded all the same (no anchors are passed)."""
    m, ref, qry, b = fixture
    cfg, search = _configs()
    before = m._block.clone()
    out = m.relocalize(qry, cfg, search)
    rec = out.search
    rot, tr = AR.pose_error(out.pose, ASR.YAW_TRUTH)
    print(f"device search: {rec.poses} poses on {rec.sample} queries; candidates {[(c['pose_index'], c['count'], c['pairs']) for c in rec.candidates]}; "
          f"chosen {rec.chosen}: {out.pairs} pairs, rms {out.rms:.6f}, rotation error {rot:.4e} rad (margin {ROTATION_MARGIN:.4e}), translation error "
          f"{tr:.4e} (margin {TRANSLATION_MARGIN:.4e})")
    assert rec.poses == R.SEARCH_POSES and rec.sample == ASR.SAMPLE
    assert [c["pose_index"] for c in rec.candidates] == R.SEARCH_ORDER and [c["count"] for c in rec.candidates] == R.SEARCH_COUNTS
    assert out.pairs == R.SEARCH_QUERIES and rot <= ROTATION_MARGIN and tr <= TRANSLATION_MARGIN
    assert torch.equal(m._block, before)
    plain = m.track(qry, cfg)
    assert AR.pose_error(plain.pose, ASR.YAW_TRUTH)[0] > 1.0 and plain.search is None
    with pytest.raises(TypeError, match="search"):
        m.relocalize(qry, cfg, IDENTITY)                           # a pose is track()'s start: relocalize takes a SearchConfig in its place
    assert _same_alignment(out, m.relocalize(qry, cfg, search)), "run to run"
    anchored = m.relocalize(qry, cfg, _configs(anchors=R.search_centroid(ref)[None])[1])      # the reference's own centroid as the one anchor
    assert [c["pose_index"] for c in anchored.search.candidates] == R.SEARCH_ORDER and anchored.pairs == R.SEARCH_QUERIES


def test_search_with_normals_meets_the_same_margin(ops, fixture):
    m, ref, qry, b = fixture
    cfg, search = _configs()
    out = m.relocalize(qry, cfg, search, normals=True)
    rot, tr = AR.pose_error(out.pose, ASR.YAW_TRUTH)
    print(f"device search, point to plane: chosen {out.search.chosen}: {out.pairs} pairs, rotation error {rot:.4e} rad, translation error {tr:.4e}")
    assert [c["pose_index"] for c in out.search.candidates] == R.SEARCH_ORDER and [c["count"] for c in out.search.candidates] == R.SEARCH_COUNTS
    assert rot <= ROTATION_MARGIN and tr <= TRANSLATION_MARGIN


# ------------------------------------------------------------------------------------------------ 12: the predictor
def test_predictor_map_relocalize_is_relocalize_on_the_same_points(ops, fixture):
    from point_sam_amd.model import PointCloudSAM
    from point_sam_amd.predictor import PointSAMPredictor
    m, ref, qry, b = fixture
    cfg = get_config("tiny")
    pred = PointSAMPredictor(PointCloudSAM(cfg, random_state_dict(cfg, 3), "cuda", precision="f16x3"))
    pred.set_scene(qry, torch.zeros(len(b), 3, device="cuda"), max_points=1024)
    icp, search = _configs()
    out = pred.map_relocalize(m, icp, search)
    assert _same_alignment(out, m.relocalize(qry, icp, search)) and out.search is not None and out.pairs == R.SEARCH_QUERIES
    with pytest.raises(TypeError, match="search"):
        pred.map_relocalize(m, icp, IDENTITY)
