"""The score of a pose search on the GPU (csrc/align_score.hip, ops.align_score) and the search built on it (point_sam_amd/align.py: search,
predictor.align(search=), the /propagate route) against the plain numpy reference tests/align_search_reference.py.  Counts are integers: every comparison
of counts is EXACT."""
import ctypes

import numpy as np
import pytest
import torch

import align_reference as A
import align_search_reference as S
import transfer_reference as T
from point_sam_amd.config import get_config
from point_sam_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu
f32 = np.float32
IDENTITY = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
HALF_TURN = np.concatenate([np.diag([-1.0, -1.0, 1.0]), [[0.05], [-0.1], [0.0]]], 1)
FAR_AWAY = np.concatenate([np.eye(3), [[3e6], [0.0], [0.0]]], 1)            # beyond 2^21 cells of any radius used here


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _counts(ops, index, qry, poses, radius=None):
    out = ops.align_score(index, _dev(np.ascontiguousarray(qry, dtype=f32)), poses, radius)
    assert out.dtype == torch.int32 and out.shape == (len(poses),) and out.is_cuda
    return out.cpu().numpy().astype(np.int64)


def _check(ops, src, r, qry, poses, radius=None):
    """The device's counts equal the reference's, word for word -> the counts."""
    src, qry = np.ascontiguousarray(src, dtype=f32), np.ascontiguousarray(qry, dtype=f32)
    want = S.score(src, r, qry, poses, r if radius is None else radius)
    got = _counts(ops, ops.transfer_index(_dev(src), r), qry, poses, radius)
    assert np.array_equal(got, want), (np.nonzero(got != want)[0][:8], got[:8], want[:8])
    return got


@pytest.fixture(scope="module")
def small():
    g = np.random.default_rng(17)
    return g.uniform(-1, 1, size=(901, 3)).astype(f32), g.uniform(-1.1, 1.1, size=(1543, 3)).astype(f32)


def _poses(P, seed=4):
    """P rigid poses: the five named ones first, then random rotations with small translations."""
    g = np.random.default_rng(seed)
    out = [IDENTITY, A.TRUE_POSE, A.TRUE_POSE, HALF_TURN, FAR_AWAY]
    while len(out) < P:
        out.append(np.concatenate([A.rotation(g.normal(size=3), g.uniform(0, 360)), g.uniform(-0.2, 0.2, size=(3, 1))], 1))
    return np.stack(out[:P])


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("r", [0.11, 0.05])
def test_small_clouds_five_poses(ops, small, r):
    src, qry = small
    got = _check(ops, src, r, qry, _poses(5))
    assert got[1] == got[2] and got[4] == 0 and (got[:4] > 0).all() and len(set(got[[0, 1, 3]].tolist())) == 3
    four = np.stack([np.concatenate([p, [[0.0, 0.0, 0.0, 1.0]]], 0) for p in _poses(5)])      # 4 x 4 rows, and a tensor of host numbers
    index = ops.transfer_index(_dev(src), r)
    assert np.array_equal(_counts(ops, index, qry, four), got) and np.array_equal(_counts(ops, index, qry, torch.from_numpy(four)), got)
    words = _dev(ops.transfer_poses(_poses(5)))                                              # the twelve words on the device, taken as they are
    assert np.array_equal(_counts(ops, index, qry, words), got)


@pytest.mark.parametrize("M,P", [(1, 1), (63, 1), (64, 2), (65, 1), (257, 3), (1025, 2)])
def test_shapes_around_a_wave_and_a_workgroup(ops, small, M, P):
    src, qry = small
    qry = np.concatenate([src[3:4] + f32(0.01), qry], 0)                                      # the first query has a source in reach
    got = _check(ops, src, 0.11, qry[:M], _poses(P))
    assert got[0] >= 1


@pytest.mark.parametrize("dP", [-1, 0, 1])
def test_pose_counts_around_a_chunk(ops, small, dP):
    src, qry = small
    P = ops.ALIGN_SCORE_POSES + dP
    got = _check(ops, src, 0.11, qry[:130], _poses(P))
    hits = np.arange(P) != 4                                                                  # pose 4, where there is one, sends every query out of range
    assert len(got) == P and (got[~hits] == 0).all() and (got[hits] > 0).all()
    if P < 33:                                                                                # and several chunks, the last one short
        got = _check(ops, src, 0.11, qry[:130], _poses(33))
        assert (got[np.arange(33) != 4] > 0).all() and got[4] == 0


def test_a_single_source(ops, small):
    src, qry = small
    qry = np.concatenate([src[:1], src[:1] + f32(0.05), qry[:200]], 0)
    got = _check(ops, src[:1], 0.11, qry, _poses(5))
    assert got[0] >= 2


def test_a_hit_at_q_equal_r2_counts_and_one_step_below_it_does_not(ops):
    """The source at (0, 0, 0), the query at (0.25, 0, 0): q = 0.0625 = fl32(0.25^2) exactly.  The bound one fp32 step lower goes through the C entry, which
    takes r2 itself."""
    from point_sam_amd import _lib
    src = np.array([[0, 0, 0], [1, 1, 1]], dtype=f32)
    qry = np.array([[0.25, 0, 0], [0.5, 0.5, 0.5]], dtype=f32)
    assert _check(ops, src, 0.25, qry, IDENTITY[None])[0] == 1
    index = ops.transfer_index(_dev(src), 0.25)
    q, words = _dev(qry), _dev(ops.transfer_poses(IDENTITY[None]))
    counts = torch.full((1,), -9, dtype=torch.int32, device="cuda")
    org = (ctypes.c_float * 3)(*index.origin)
    for r2, want in ((f32(0.0625), 1), (np.nextafter(f32(0.0625), f32(0)), 0)):
        assert S.score(src, 0.25, qry, IDENTITY[None], None, r2)[0] == want
        st = _lib.load().psam_pose_score(index.src_xyz.data_ptr(), 2, index.ws.data_ptr(), index.ws.numel() * 8, ctypes.addressof(org), float(index.inv_h),
                                         float(r2), q.data_ptr(), 2, words.data_ptr(), 1, counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert st == 0 and int(counts[0]) == want, (r2, int(counts[0]))


def test_a_smaller_search_radius_on_a_coarser_index_and_a_larger_one_refused(ops, small):
    src, qry = small
    src = np.concatenate([src, (qry[:300] + f32(0.02)).astype(f32)], 0)                       # sources in reach of the smaller radius too
    got = _check(ops, src, 0.11, qry, _poses(5), 0.05)
    assert np.array_equal(got, S.score(src, 0.05, qry, _poses(5), 0.05)) and got[0] >= 250    # here the 27 cells of either index hold the radius-0.05 search
    wide = _check(ops, src, 0.11, qry, _poses(5))
    assert (wide >= got).all() and wide[0] > got[0]
    index = ops.transfer_index(_dev(src), 0.11)
    with pytest.raises(ValueError, match=r"align_score: radius .* exceeds the index's .*: the search covers the 27 cells around a query only"):
        ops.align_score(index, _dev(qry), _poses(5), 0.12)


def test_queries_without_a_cell_hit_nothing_and_disturb_no_count(ops, small):
    src, qry = small
    odd = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e7, 0, 0], [-1e7, -1e7, 1e7], [np.nan, np.nan, np.nan]], dtype=f32)
    mixed = np.concatenate([odd[:3], qry[:700], odd[3:], qry[700:]], 0).astype(f32)
    poses = _poses(7)
    assert np.array_equal(_check(ops, src, 0.11, mixed, poses), _check(ops, src, 0.11, qry, poses))
    assert np.array_equal(_check(ops, src, 0.11, odd, poses), np.zeros(7))


def test_one_long_chain_with_duplicates(ops):
    g = np.random.default_rng(3)
    src = (g.integers(0, 16, size=(300, 3)).astype(f32) / f32(64)).astype(f32)      # one cell of 0.25: a chain of 300, many exact duplicates
    src[0] = 0                                                                      # pins the origin: the cell is [0, 0.25)^3
    src[200:] = src[100:200]                                                        # every one of these twice
    assert len(T.index(src, 0.25, T.parameters(src, 0.25)[0])) == 1
    qry = np.concatenate([(g.integers(-16, 32, size=(700, 3)).astype(f32) / f32(64)).astype(f32), src[200:]], 0)
    poses = np.stack([IDENTITY, np.concatenate([np.eye(3), [[0.25], [0.0], [-0.125]]], 1), HALF_TURN, FAR_AWAY])
    for radius in (None, 1 / 32):                                                   # at 1/32 most queries walk the whole chain and find nothing
        got = _check(ops, src, 0.25, qry, poses, radius)
        assert got[0] >= 100 and got[3] == 0
    assert got[0] < 800


@pytest.mark.parametrize("where", [0, 3, 6])
def test_the_only_source_in_reach_sits_in_the_27th_cell_behind_a_chain(ops, where):
    """Cells of 0.25 from the origin (-0.25)^3.  The query, just below (0.25, 0.25, 0.25), is in cell (1, 1, 1); the one source within 1/64 of it, AT that
    corner, is in cell (2, 2, 2) -- o = 26, the last cell the walk visits -- among six more sources of that cell which are out of reach.  The chain's order
    is the build's own, so the source is placed first, in the middle and last in the array: whichever way a chain runs, one of the three has it at the
    chain's end.  A walk that gave up early, or skipped the last cell, would count 0."""
    g = np.random.default_rng(9)
    near = np.full((1, 3), 0.25, dtype=f32)
    rest = (0.25 + g.integers(8, 16, size=(6, 3)) / 64).astype(f32)                  # cell (2, 2, 2), at least 1/8 from the corner on every axis
    cell = np.concatenate([rest[:where], near, rest[where:]], 0)
    own = (g.integers(0, 8, size=(20, 3)) / 64).astype(f32)                          # the query's own cell: a chain to walk, nothing in reach
    own[0] = 0                                                                       # pins the origin
    src = np.concatenate([own[:10], cell, own[10:]], 0)
    table = T.index(src, 0.25, T.parameters(src, 0.25)[0])
    assert set(table) == {(1, 1, 1), (2, 2, 2)} and len(table[(2, 2, 2)]) == 7
    qry = np.full((1, 3), 0.25 - 2.0 ** -9, dtype=f32)
    assert _check(ops, src, 0.25, qry, IDENTITY[None], 1 / 64)[0] == 1
    assert _check(ops, np.delete(src, 10 + where, 0), 0.25, qry, IDENTITY[None], 1 / 64)[0] == 0      # without that source: nothing


def test_counts_equal_the_pairs_of_align_step_pose_by_pose(ops):
    a, b = A.icp_case()
    index = ops.transfer_index(_dev(a), A.ICP_RADIUS)
    qry = _dev(b)
    poses = _poses(40, seed=6)
    poses[5:] = [np.concatenate([A.rotation([0.3, -0.5, 0.8], 4.0 + 0.5 * k), (A.TRUE_POSE[:, 3] + 0.002 * k)[:, None]], 1) for k in range(35)]
    for radius in (None, A.ICP_FINAL):
        got = ops.align_score(index, qry, poses, radius).cpu().numpy()
        want = [int(ops.align_step(index, qry, p, radius)[0]) for p in poses]
        assert got.tolist() == want, (got, want)
    assert got[1] > 6000 and got[4] == 0 and len(set(want)) > 20


def test_entry_refusals_leave_the_counts_untouched_and_an_accepted_call_overwrites_them(ops, small):
    from point_sam_amd import _lib
    lib = _lib.load()
    src, qry = small
    poses = _poses(37)
    index = ops.transfer_index(_dev(src), 0.11)
    q, words = _dev(qry), _dev(ops.transfer_poses(poses))
    counts = torch.full((37,), -77, dtype=torch.int32, device="cuda")
    org = (ctypes.c_float * 3)(*index.origin)
    bad_org = (ctypes.c_float * 3)(0.0, float("inf"), 0.0)
    stream = torch.cuda.current_stream().cuda_stream
    good = dict(src=index.src_xyz.data_ptr(), N=len(src), index_ws=index.ws.data_ptr(), index_ws_bytes=index.ws.numel() * 8, origin=ctypes.addressof(org),
                inv_h=float(index.inv_h), r2=float(index.r2), qry=q.data_ptr(), M=len(qry), poses=words.data_ptr(), P=37, counts=counts.data_ptr())
    call = lambda **kw: lib.psam_pose_score(*{**good, **kw}.values(), stream)
    for code, kw in ((-1, dict(r2=float("nan"))), (-1, dict(inv_h=0.0)), (-1, dict(M=0)), (-1, dict(N=-1)), (-1, dict(P=0)), (-1, dict(P=(1 << 20) + 1)),
                     (-1, dict(poses=None)), (-1, dict(counts=None)), (-1, dict(origin=ctypes.addressof(bad_org))), (-2, dict(qry=q.data_ptr() + 2)),
                     (-2, dict(poses=words.data_ptr() + 1)), (-2, dict(counts=counts.data_ptr() + 2)), (-2, dict(index_ws=index.ws.data_ptr() + 8)),
                     (-3, dict(index_ws_bytes=lib.psam_transfer_index_workspace_bytes(len(src)) - 1))):
        assert call(**kw) == code, (kw, lib.psam_last_error_string())
        assert b"psam_pose_score" in lib.psam_last_error_string()
    torch.cuda.synchronize()
    assert bool((counts == -77).all())
    assert call() == 0
    first = counts.cpu().numpy().copy()
    want = S.score(src, 0.11, qry, poses, 0.11)
    assert np.array_equal(first, want) and first[4] == 0 and (first != -77).all()           # pose 4 hits nothing: its word is a written 0
    assert call() == 0                                                                      # onto its own previous answer: cleared, not added to
    assert np.array_equal(counts.cpu().numpy(), first)


# ------------------------------------------------------------------------------------------------ the search, on the fixture tests/test_align_search_cpu.py verifies
ROTATION_MARGIN = 10 * S.YAW_REF_ROTATION_ERROR            # ten times the reference ICP's recorded error from a good start: the margin
TRANSLATION_MARGIN = 10 * S.YAW_REF_TRANSLATION_ERROR      # tests/test_gpu_align.py gives the device ICP's fp64 sum order, for the same reason


def _configs(scale=1.0):
    from point_sam_amd.align import AlignConfig, SearchConfig
    icp = AlignConfig(S.ICP["radius"] / scale, S.ICP["final_radius"] / scale, S.ICP["shrink"], S.ICP["iterations"])
    return icp, SearchConfig(rotations="yaw", yaw_steps=S.YAW_STEPS, offsets=S.YAW_OFFSETS, offset_step=S.YAW_OFFSET_STEP / scale, sample=S.SAMPLE,
                             radius=S.SCORE_RADIUS / scale, keep=S.KEEP)


def _same_alignment(a, b):
    return (np.array_equal(a.pose.view(np.int64), b.pose.view(np.int64)) and (a.pairs, a.coverage, a.rms, a.iterations, a.converged, a.reason) ==
            (b.pairs, b.coverage, b.rms, b.iterations, b.converged, b.reason) and a.history == b.history)


def _same_record(a, b):
    return (a.poses, a.sample, a.chosen) == (b.poses, b.sample, b.chosen) and repr(a.candidates) == repr(b.candidates)


def test_search_on_the_device_scores_like_the_reference_and_finds_the_truth(ops):
    """Fixture (a): the first eight pose indices and their counts are the reference's (S.YAW_ORDER, S.YAW_COUNTS: recomputed on the CPU by
    tests/test_align_search_cpu.py), exactly.  The refinement runs the device's ICP, whose pose may differ from the reference's by an fp32 ulp on the
    way: the chosen pose is held against the TRUTH within the margins above."""
    from point_sam_amd import align as X
    a, b = S.yaw_case()
    icp, cfg = _configs()
    index = ops.transfer_index(_dev(a), icp.radius)
    out = X.search(index, _dev(b), cfg, icp)
    rec = out.search
    rot, tr = A.pose_error(out.pose, S.YAW_TRUTH)
    print(f"device search: {rec.poses} poses on {rec.sample} queries, refined {[(c['pose_index'], c['count'], c['pairs']) for c in rec.candidates]}, chosen "
          f"{rec.chosen}: {out.pairs} pairs, rms {out.rms:.6f}, rotation error {rot:.4e} rad (margin {ROTATION_MARGIN:.4e}), translation error {tr:.4e} "
          f"(margin {TRANSLATION_MARGIN:.4e})")
    assert (rec.poses, rec.sample) == (1944, 512)
    assert [c["pose_index"] for c in rec.candidates] == S.YAW_ORDER and [c["count"] for c in rec.candidates] == S.YAW_COUNTS
    assert out.pairs > 4300 and rot <= ROTATION_MARGIN and tr <= TRANSLATION_MARGIN
    assert min(c["pairs"] for c in rec.candidates) < out.pairs
    again = X.search(index, _dev(b), cfg, icp)                                               # run to run
    assert _same_alignment(out, again) and _same_record(rec, again.search)


# ------------------------------------------------------------------------------------------------ the predictor
@pytest.fixture(scope="module")
def scans(ops):
    """Fixture (a)'s sources as a scene with a snapshot of two objects, then its queries as the current scene; both are their own working clouds."""
    from point_sam_amd.model import PointCloudSAM
    from point_sam_amd.predictor import PointSAMPredictor
    cfg = get_config("tiny")
    pred = PointSAMPredictor(PointCloudSAM(cfg, random_state_dict(cfg, 3), "cuda", precision="f16x3"))
    a, b = S.yaw_case()
    axyz, bxyz = _dev(a), _dev(b)
    pred.set_scene(axyz, torch.full_like(axyz, 0.5), max_points=8192)
    snap = pred.snapshot(_dev(A.mask_rows(a)))
    assert torch.equal(snap.coords, axyz)
    pred.set_scene(bxyz, torch.full_like(bxyz, 0.5), max_points=8192)
    assert torch.equal(pred._state.coords[0], bxyz)
    return pred, snap, bxyz


def test_predictor_align_with_search_equals_the_search_composed_from_public_calls(ops, scans):
    from point_sam_amd import align as X
    pred, snap, bxyz = scans
    icp, cfg = _configs()
    take = torch.zeros(ops.mask_words(len(bxyz)), dtype=torch.int64, device="cuda")
    take[:50] = -1                                                                     # the first 3200 working points
    for kw in (dict(), dict(mask=take)):
        got = pred.align(snap, icp, search=cfg, **kw)
        want = X.search(ops.transfer_index(snap.coords, icp.radius), pred._state.coords[0].contiguous(), cfg, icp, kw.get("mask"))
        assert _same_alignment(got, want) and _same_record(got.search, want.search), kw
        assert got.pose.shape == (3, 4) and got.pose.dtype == np.float64 and len(got.search.candidates) == S.KEEP
    rot, tr = A.pose_error(got.pose, S.YAW_TRUTH)                                      # the masked run: the same truth from the first 3200 points
    assert got.search.sample == 512 and got.pairs <= 3200
    full = pred.align(snap, icp, search=cfg)
    rot, tr = A.pose_error(full.pose, S.YAW_TRUTH)
    assert rot <= ROTATION_MARGIN and tr <= TRANSLATION_MARGIN
    # search=None is the path of before: the ICP from the identity (which does not get there), and no record
    plain = pred.align(snap, icp)
    assert _same_alignment(plain, X.icp(ops.transfer_index(snap.coords, icp.radius), pred._state.coords[0].contiguous(), icp)) and plain.search is None
    assert _same_alignment(plain, pred.align(snap, icp, search=None)) and A.pose_error(plain.pose, S.YAW_TRUTH)[0] > 1.0
    # the refusals
    with pytest.raises(ValueError, match="init and search"):
        pred.align(snap, icp, init=IDENTITY, search=cfg)
    with pytest.raises(TypeError, match="SearchConfig"):
        pred.align(snap, icp, search={"keep": 8})
    with pytest.raises(ValueError, match="exceeds"):
        pred.align(snap, icp, search=X.SearchConfig(radius=2 * icp.radius))


# ------------------------------------------------------------------------------------------------ the demo
def _write_ply(path, pts):
    with open(path, "w") as f:
        f.write(f"ply\nformat ascii 1.0\nelement vertex {len(pts)}\nproperty float x\nproperty float y\nproperty float z\n"
                "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
        f.writelines(f"{p[0]!r} {p[1]!r} {p[2]!r} 128 128 128\n" for p in pts.tolist())


def test_propagate_route_with_search_returns_the_pose_and_the_record(ops, scans, tmp_path):
    """Fixture (a) through the demo, as tests/test_gpu_align.py sends its fixture: the sources (with two far points that keep the queries inside the unit
    ball of their normalisation) are loaded and clicked, the queries follow by /propagate with "align" and "search" and NO pose.  Lengths in the request
    are in normalised coordinates, so the fixture's are divided by the scale; the pose is held against the truth there.  A second session that is GIVEN
    the returned pose, without "align" or "search", answers with the fields of before, equal value for value."""
    import http.client
    import json
    import threading
    from point_sam_amd.demo_server import DemoSession, serve
    from point_sam_amd.predictor import PointSAMPredictor
    a, b = S.yaw_case()
    a = np.concatenate([a.astype(np.float64), [[1.3, 1.2, 1.1], [-1.4, -1.3, -1.2]]], 0)
    _write_ply(tmp_path / "a.ply", a)
    _write_ply(tmp_path / "b.ply", b.astype(np.float64))
    shift = a.mean(0)
    scale = np.linalg.norm(a - shift, axis=1).max()
    Rm, t = S.YAW_TRUTH[:, :3], S.YAW_TRUTH[:, 3]
    truth = np.concatenate([Rm, ((Rm @ shift + t - shift) / scale)[:, None]], 1)       # A_n = R B_n + (R c + t - c) / s
    model = scans[0].model

    def session(body):
        sess = DemoSession(PointSAMPredictor(model), models_dir=str(tmp_path), output_dir=str(tmp_path / "results"))
        srv = serve(sess, "127.0.0.1", 0)
        threading.Thread(target=srv.serve_forever, daemon=True).start()

        def req(method, path, data=None):
            c = http.client.HTTPConnection("127.0.0.1", srv.server_address[1], timeout=120)
            c.request(method, path, None if data is None else json.dumps(data), {"Content-Type": "application/json"})
            r = c.getresponse()
            return r.status, json.loads(r.read())
        try:
            st, cloud = req("GET", "/pointcloud/a.ply")
            assert st == 200 and len(cloud["xyz"]) == 3 * len(a)
            k = int(np.argmin(np.linalg.norm(a - np.array([0.15, 0.1, 0.15]), axis=1)))      # the top of the sphere
            st, seg = req("POST", "/segment", {"prompt_point": cloud["xyz"][3 * k:3 * k + 3], "prompt_label": 1})
            assert st == 200, seg
            return req("POST", "/propagate", dict({"pointcloud": "b.ply", "radius": A.TRANSFER_RADIUS}, **body))
        finally:
            srv.shutdown()

    icp, cfg = _configs(scale)
    fields = {"radius": icp.radius, "final_radius": icp.final_radius, "shrink": icp.shrink, "iterations": icp.iterations}
    search = {"rotations": "yaw", "yaw_steps": cfg.yaw_steps, "offsets": cfg.offsets, "offset_step": cfg.offset_step, "sample": cfg.sample,
              "radius": cfg.radius, "keep": cfg.keep}
    st, out = session({"align": fields, "search": search})
    assert st == 200, out
    pose = np.array(out["pose"])
    rot, tr = A.pose_error(pose, truth)
    print(f"/propagate with search: {out['align']}, rotation error {rot:.4e} rad, translation error {tr:.4e} (normalised; scale {scale:.4f})")
    assert pose.shape == (3, 4) and rot <= ROTATION_MARGIN and tr <= TRANSLATION_MARGIN / scale
    stats = out["align"]
    assert set(stats) == {"pairs", "coverage", "rms", "iterations", "converged", "search"} and stats["pairs"] > 4300
    rec = stats["search"]
    assert set(rec) == {"poses", "sample", "chosen", "candidates"} and (rec["poses"], rec["sample"]) == (1944, 512) and len(rec["candidates"]) == S.KEEP
    assert all(set(c) == {"pose_index", "count", "pairs", "rms", "converged"} for c in rec["candidates"])
    assert rec["candidates"][rec["chosen"]]["pairs"] == stats["pairs"] == max(c["pairs"] for c in rec["candidates"])
    assert [c["count"] for c in rec["candidates"]] == sorted((c["count"] for c in rec["candidates"]), reverse=True)
    st, bad = session({"search": search})                                              # "search" alone: this request's 400
    assert st == 400 and "error" in bad
    st, plain = session({"pose": out["pose"]})
    assert st == 200 and set(plain) == {"xyz", "rgb", "objects", "lost", "scores"} == set(out) - {"pose", "align"}
    assert all(plain[k] == out[k] for k in plain)
