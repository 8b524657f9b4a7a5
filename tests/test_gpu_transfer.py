"""Masks carried to the next scan on the GPU (csrc/transfer.hip, point_sam_amd/transfer.py, predictor.snapshot / transfer_masks / propagate) against the plain
numpy reference tests/transfer_reference.py.  Every comparison is exact: idx3 as int32, w3 and rows through a 32-bit integer view.  NaNs that a blend
computed (an infinite or NaN source logit) are compared as NaNs, as tests/test_gpu_scene_interp.py does: their payload is the adder's business."""
import numpy as np
import pytest
import torch

import interp_reference as I
import transfer_reference as T
from point_sam_amd.config import get_config
from point_sam_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd import ops
    return ops


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _device_plan(ops, src, r, qry, pose=None):
    index = ops.transfer_index(_dev(src), r)
    o, inv_h, r2 = T.parameters(src, r)
    assert index.origin == tuple(float(v) for v in o) and index.inv_h == inv_h and index.r2 == r2 and index.num_source == len(src)
    idx3, w3 = ops.transfer_plan(index, _dev(qry), pose)
    assert idx3.dtype == torch.int32 and w3.dtype == torch.float32 and idx3.shape == w3.shape == (len(qry), 3)
    return idx3.cpu().numpy(), w3.cpu().numpy()


def _check_plan(ops, src, r, qry, pose=None):
    """The device's plan equals the reference's bit for bit -> (idx3, w3)."""
    src, qry = np.ascontiguousarray(src, dtype=f32), np.ascontiguousarray(qry, dtype=f32)
    want_i, want_w = T.plan(src, r, qry, pose)
    got_i, got_w = _device_plan(ops, src, r, qry, pose)
    bad = np.nonzero((got_i != want_i).any(1) | (got_w.view(np.int32) != want_w.view(np.int32)).any(1))[0]
    assert len(bad) == 0, (len(bad), bad[:5], got_i[bad[:5]], want_i[bad[:5]], got_w[bad[:5]], want_w[bad[:5]])
    return want_i, want_w


def _same_words(got, want, idx3, N):
    got, want = np.ascontiguousarray(got, dtype=f32).copy(), np.ascontiguousarray(want, dtype=f32).copy()
    b = I.blended(idx3, N)[None] & np.ones(got.shape, dtype=bool)
    for a in (got, want):
        a.view(np.uint32)[b & np.isnan(a)] = 0x7FC00000
    return np.array_equal(got.view(np.int32), want.view(np.int32))


# ------------------------------------------------------------------------------------------------ the plan
def test_lattice_case_with_radius_edges_and_points_without_a_cell(ops):
    src, qry, r = T.lattice_case()
    rr = f32(r)
    on_edge = src[:50] + np.array([rr, 0, 0], dtype=f32)                            # q == r2: the source is a candidate
    past_edge = src[:50] + np.array([rr + f32(1 / 128), 0, 0], dtype=f32)           # that source is not
    odd = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e6, 0, 0], [-1e6, -1e6, 1e6]], dtype=f32)
    qry = np.concatenate([qry, on_edge, past_edge, odd], 0).astype(f32)
    idx3, w3 = _check_plan(ops, src, r, qry)
    cands = T.candidates_grid(src, r, qry)
    for k in range(50):
        assert k in cands[1543 + k][0] and k not in cands[1593 + k][0]
    assert (idx3[-5:] == -1).all() and (w3[-5:] == 0).all()
    n = np.array([len(c[0]) for c in cands])
    assert (n == 0).any() and (n == 1).any() and (n == 2).any() and (n >= 3).any()


@pytest.mark.parametrize("r", [0.05, 0.11])
@pytest.mark.parametrize("posed", [False, True])
def test_uniform_cases(ops, r, posed):
    src, qry = T.uniform_case()
    idx3, _ = _check_plan(ops, src, r, qry, T.POSE if posed else None)
    assert (idx3[:, 0] >= 0).mean() > 0.3


def test_a_four_by_four_pose_is_the_same_plan(ops):
    src, qry = T.uniform_case()
    P4 = np.concatenate([T.POSE.astype(np.float64), [[0, 0, 0, 1]]], 0)
    a = _device_plan(ops, src, 0.05, qry[:2000], T.POSE)
    b = _device_plan(ops, src, 0.05, qry[:2000], P4.tolist())
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


@pytest.mark.parametrize("N,M", [(1, 1543), (901, 1), (901, 257), (901, 1025)])
def test_single_source_single_query_and_one_past_a_block(ops, N, M):
    src, qry, r = T.lattice_case()
    src = src[:N]
    if N == 1:
        qry = np.concatenate([src, src + f32(0.125), qry], 0)[:M]                   # an exact hit and a lone candidate among them
    idx3, _ = _check_plan(ops, src, r, qry[:M])
    assert idx3.shape == (M, 3) and (N > 1 or (idx3[0].tolist() == [0, -1, -1] and idx3[1].tolist() == [0, -1, -1]))


def test_one_long_chain_with_duplicates(ops):
    g = np.random.default_rng(3)
    src = (g.integers(0, 16, size=(300, 3)).astype(f32) / f32(64)).astype(f32)      # one cell of 0.25: a chain of 300, many exact duplicates
    src[0] = 0                                                                      # pins the origin: the cell is [0, 0.25)^3
    assert len(T.index(src, 0.25, T.parameters(src, 0.25)[0])) == 1
    qry = (g.integers(-16, 32, size=(700, 3)).astype(f32) / f32(64)).astype(f32)
    _check_plan(ops, src, 0.25, qry)


def test_many_occupied_cells_probe_past_collisions(ops):
    g = np.random.default_rng(5)
    src = g.uniform(-1, 1, size=(40000, 3)).astype(f32)
    qry = np.concatenate([src[g.integers(0, 40000, size=2500)] + g.normal(0, 0.004, size=(2500, 3)).astype(f32), g.uniform(-1, 1, size=(2500, 3)).astype(f32)], 0)
    assert len(T.index(src, 0.01, T.parameters(src, 0.01)[0])) > 30000              # tens of thousands of keys in a table of 2^17 slots
    idx3, _ = _check_plan(ops, src, 0.01, qry.astype(f32))
    assert 0.2 < (idx3[:, 0] >= 0).mean() < 0.9


def test_two_builds_give_identical_bits(ops):
    """The order inside a chain is the arrival order and may differ between two builds; no output may."""
    src, qry = T.uniform_case()
    a = _device_plan(ops, src, 0.11, qry, T.POSE)
    b = _device_plan(ops, src, 0.11, qry, T.POSE)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


# ------------------------------------------------------------------------------------------------ apply
def test_transfer_rows_and_bits_equal_the_reference_apply(ops):
    from point_sam_amd import transfer as X
    src, qry = T.uniform_case()
    index = ops.transfer_index(_dev(src), 0.05)
    plan = X.TransferPlan(*ops.transfer_plan(index, _dev(qry)), index.num_source)
    idx3, w3 = plan.idx3.cpu().numpy(), plan.w3.cpu().numpy()
    g = np.random.default_rng(9)
    rows = g.normal(size=(5, len(src))).astype(f32)
    rows[1, ::7] = np.inf; rows[2, ::11] = np.nan; rows[3, ::5] = -np.inf
    cov = X.covered(plan).cpu().numpy()
    assert np.array_equal(cov, idx3[:, 0] >= 0) and 0.3 < cov.mean() < 0.8
    for fill in (None, -7.5, float("-inf")):
        got = X.transfer_rows(plan, _dev(rows), fill).cpu().numpy()
        assert got.shape == (5, len(qry))
        assert _same_words(got, I.apply_rows(rows, idx3, w3, 0.0 if fill is None else fill), idx3, len(src))
    for thr in (0.0, 0.4):
        bits, area = X.transfer_bits(plan, _dev(rows), thr)
        want_bits, want_area = I.apply_bits(rows, idx3, w3, thr)
        assert np.array_equal(bits.cpu().numpy().view(np.uint64), want_bits) and np.array_equal(area.cpu().numpy(), want_area)


def test_a_permutation_of_the_sources_is_a_copy(ops):
    from point_sam_amd import transfer as X
    g = np.random.default_rng(13)
    src = np.unique(g.uniform(-1, 1, size=(3000, 3)).astype(f32), axis=0)
    perm = g.permutation(len(src))
    plan = X.build_plan(_dev(src), _dev(src[perm]), 0.07)
    idx3, w3 = plan.idx3.cpu().numpy(), plan.w3.cpu().numpy()
    assert np.array_equal(idx3[:, 0], perm.astype(np.int32)) and (idx3[:, 1:] == -1).all()
    assert np.array_equal(w3, np.tile(np.array([1, 0, 0], dtype=f32), (len(src), 1)))
    logits = g.normal(size=(3, len(src))).astype(f32)
    logits[0, 5] = np.nan; logits[1, 6] = np.inf
    got = X.transfer_rows(plan, _dev(logits)).cpu().numpy()
    assert np.array_equal(got.view(np.int32), logits[:, perm].view(np.int32))


# ------------------------------------------------------------------------------------------------ the predictor
CENTRES = np.array([[0.45, 0.0, 0.0], [-0.45, 0.0, 0.1], [0.0, 0.55, 0.0], [0.0, -0.55, -0.1]], dtype=np.float64)
SPHERE, REACH, RADIUS = 0.2, 0.3, 0.06


def _surfaces(n, seed, spheres):
    """n points on the spheres `spheres` of CENTRES, in scan A's frame."""
    g = np.random.default_rng(seed)
    d = g.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return CENTRES[np.asarray(spheres)[g.integers(0, len(spheres), size=n)]] + SPHERE * d


@pytest.fixture(scope="module")
def scans(ops):
    """Scan A: 20 000 points on four spheres.  Scan B: another sample of the first three (the fourth is gone: nothing of B within RADIUS of it), given
    in a frame from which T.POSE leads back to A's.  K = 3 logit rows over A: REACH - distance to the centres of spheres 0, 1 and 3."""
    from point_sam_amd.model import PointCloudSAM
    from point_sam_amd.predictor import PointSAMPredictor
    cfg = get_config("tiny")
    model = PointCloudSAM(cfg, random_state_dict(cfg, 3), "cuda", precision="f16x3")
    a = _surfaces(20000, 1, [0, 1, 2, 3])
    b_in_a = _surfaces(15000, 2, [0, 1, 2])
    Rm, t = T.POSE[:, :3].astype(np.float64), T.POSE[:, 3].astype(np.float64)
    b = (b_in_a - t) @ Rm                                                           # q = R^T (p - t)
    assert np.abs(b).max() < 1 and np.abs(a).max() < 1
    axyz, bxyz = _dev(a, torch.float32), _dev(b, torch.float32)
    argb, brgb = torch.full_like(axyz, 0.5), torch.full_like(bxyz, 0.5)
    logits = np.stack([REACH - np.linalg.norm(a - CENTRES[k], axis=1) for k in (0, 1, 3)]).astype(f32)
    pred = PointSAMPredictor(model)
    pred.set_scene(axyz, argb, max_points=4096)
    assert not pred.scene.identity and pred.scene.num_working <= 4096
    snap = pred.snapshot(_dev(logits))
    assert snap.num_masks == 3 and snap.coords.shape == (pred.scene.num_working, 3)
    assert torch.equal(snap.coords, pred._state.coords[0]) and torch.equal(snap.logits, _dev(logits).index_select(1, pred.scene.keep_idx))
    assert torch.equal(pred.snapshot(snap.logits).logits, snap.logits)              # working width passes unchanged
    pred.set_scene(bxyz, brgb, max_points=4096)
    return pred, snap, bxyz, brgb, (axyz, argb)


def test_transfer_masks_equal_the_reference_at_scan_width(ops, scans):
    pred, snap, bxyz, _, _ = scans
    src, rows = snap.coords.cpu().numpy(), snap.logits.cpu().numpy()
    idx3, w3 = T.plan(src, RADIUS, bxyz.cpu().numpy(), T.POSE)
    for thr in (0.0, 0.05):
        bits, area, covered = pred.transfer_masks(snap, RADIUS, T.POSE, thr)
        want_bits, want_area = I.apply_bits(rows, idx3, w3, thr)
        assert bits.shape == (3, (len(bxyz) + 63) // 64)
        assert np.array_equal(bits.cpu().numpy().view(np.uint64), want_bits) and np.array_equal(area.cpu().numpy(), want_area)
        assert int(covered) == int((idx3[:, 0] >= 0).sum())
    assert int(covered) > 0.8 * len(bxyz) and want_area[0] > 1000 and want_area[1] > 1000 and want_area[2] == 0


def _composed(ops, pred, snap, clicks):
    """propagate's steps from public calls, for every snapshot row with a non-empty carried mask -> (kept rows, logits at scan width, scores, clicks, labels)."""
    model, st, sc = pred.model, pred._state, pred.scene
    index = ops.transfer_index(snap.coords, RADIUS)
    idx3, w3 = ops.transfer_plan(index, st.coords[0].contiguous(), T.POSE)
    prior = ops.scene_interp_rows(snap.logits, idx3, w3, 0.0)
    prior = torch.where((idx3[:, 0] >= 0)[None], prior, snap.logits.amin(1, keepdim=True)).contiguous()
    gt = prior > 0
    keep = torch.nonzero(gt.any(1))[:, 0]
    truth, pm, prev = gt[keep][None], prior[keep].contiguous(), None
    pc = torch.empty(len(keep), 0, 3, device="cuda")
    pl = torch.empty(len(keep), 0, dtype=torch.bool, device="cuda")
    for _ in range(clicks):
        nc, nl = model.sample_prompts(st.coords, truth, prev)
        pc, pl = torch.cat([pc, nc], 1), torch.cat([pl, nl], 1)
        masks, iou = model.decode(st, pc, pl, pm, multimask_output=False)
        pm = prev = masks[:, 0].contiguous()
    return keep, ops.scene_expand_rows(prev, sc.inv), iou[:, 0], pc, pl, gt.sum(1)


@pytest.mark.parametrize("clicks", [1, 2])
def test_propagate_equals_its_steps_composed_from_public_calls(ops, scans, clicks):
    pred, snap, bxyz, _, _ = scans
    out = pred.propagate(snap, RADIUS, T.POSE, clicks=clicks)
    keep, logits, scores, pc, pl, area = _composed(ops, pred, snap, clicks)
    assert keep.tolist() == [0, 1] and out.lost.tolist() == [False, False, True]
    assert out.logits.shape == (3, len(bxyz)) and out.logits.dtype == torch.float32
    assert torch.equal(out.logits[:2].view(torch.int32), logits.view(torch.int32))
    assert bool(torch.isinf(out.logits[2]).all()) and bool((out.logits[2] < 0).all())
    assert torch.equal(out.scores[:2].view(torch.int32), scores.float().view(torch.int32)) and bool(torch.isnan(out.scores[2]))
    assert torch.equal(out.prior_area, area) and out.prior_area[2] == 0
    assert out.click_points.shape == (3, clicks, 3) and torch.equal(out.click_points[:2], pc) and torch.equal(out.click_labels[:2], pl)
    assert bool(torch.isnan(out.click_points[2]).all()) and not bool(out.click_labels[2].any())
    assert bool(out.click_labels[:, 0][:2].all())                                   # click 0 is a point of the carried mask
    assert 0.8 < out.covered <= 1.0
    # the lost object takes no part: the others' outputs are those of a run without it
    from point_sam_amd.transfer import Snapshot
    two = pred.propagate(Snapshot(snap.coords, snap.logits[:2].contiguous(), 2), RADIUS, T.POSE, clicks=clicks)
    assert two.lost.tolist() == [False, False]
    assert torch.equal(two.logits.view(torch.int32), out.logits[:2].view(torch.int32)) and torch.equal(two.scores.view(torch.int32), out.scores[:2].view(torch.int32))


def test_a_constant_fill_replaces_the_minimum(ops, scans):
    """At a radius below the working clouds' spacing many points have no source: their prior is the fill."""
    pred, snap, _, _, _ = scans
    low = pred.propagate(snap, 0.012, T.POSE, fill=-50.0)
    assert low.lost.tolist() == [False, False, True] and 0.02 < low.covered < 0.9
    high = pred.propagate(snap, 0.012, T.POSE, fill=1.0)                            # every uncovered point joins every carried mask
    assert high.lost.tolist() == [False, False, False] and bool((high.prior_area > low.prior_area).all())


def test_snapshot_and_propagate_refuse_a_crop(ops, scans):
    pred, snap, bxyz, brgb, _ = scans
    pred.set_crop((0.0, 0.0, 0.0), 0.9, max_points=2048)
    try:
        for call in (lambda: pred.snapshot(snap.logits), lambda: pred.propagate(snap, RADIUS), lambda: pred.transfer_masks(snap, RADIUS)):
            with pytest.raises(RuntimeError, match="crop"):
                call()
    finally:
        pred.clear_crop()
    assert pred.propagate(snap, RADIUS, T.POSE).lost.tolist() == [False, False, True]
