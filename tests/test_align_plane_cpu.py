"""Point-to-plane ICP, the part that needs no GPU: the numpy reference (tests/align_plane_reference.py) against its own definition and its recorded
constants, solve_plane against the reference solve, PlaneConfig, the four-field Snapshot, the host loop of align.icp(normals=...) driven by the
reference step, the C entry points' declarations and refusals, every refusal of ops.align_plane_step raised before the library is touched, and the
demo's "plane" body rules."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

import align_plane_reference as P
import align_reference as A
import interp_reference as I
import transfer_reference as T
from point_sam_amd import _lib
from point_sam_amd import align as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANE_ENTRY_POINTS = ("psam_plane_workspace_bytes", "psam_plane_step")
POINT_TO_POINT_STEPS = 40      # tests/align_reference.py: the reference point-to-point ICP's fixed point on the same case
f32 = np.float32
IDENTITY = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("radius", [None, 0.125])
def test_reference_step_equals_its_definition_on_the_lattice(radius):
    """Vectorised pairs = the definition's, and with axis normals on the lattice every term is a short dyadic number: the sums are exact in ANY order."""
    src, qry, r = T.lattice_case()
    nrm = P.axis_normals(len(src), 5, zeros=0.25)
    near, sums, mass = P.step(src, nrm, r, qry, None, radius)
    want, wsums, _ = P.step(src, nrm, r, qry, None, radius, definition=True)
    assert np.array_equal(near, want) and np.array_equal(sums, wsums)
    assert np.array_equal(near, A.step(src, r, qry, None, radius)[0])                    # the pairs are point-to-point's
    paired = near >= 0
    used = paired.copy()
    used[paired] = np.abs(nrm[near[paired]]).sum(1) > 0
    assert sums[0] == used.sum() > 200 and sums[30] == (paired & ~used).sum() > 50 and sums[0] + sums[30] == paired.sum() and sums[31] == 1173
    p, s, n = qry[used].astype(np.float64), src[near[used]].astype(np.float64), nrm[near[used]].astype(np.float64)
    res = ((p - s) * n).sum(1)
    Jm = np.concatenate([np.cross(p, n), n], 1)
    assert sums[2] == (res * res).sum() and np.array_equal(sums[3:9], (Jm * res[:, None]).sum(0))
    full = Jm.T @ Jm
    assert np.array_equal(sums[9:30], full[np.triu_indices(6)]) and np.array_equal(mass[[0, 30, 31]], sums[[0, 30, 31]])


def test_reference_drops_zero_nan_and_infinite_normals_and_ignores_their_sign():
    src, qry = T.uniform_case()
    g = np.random.default_rng(6)
    nrm = g.normal(size=src.shape).astype(f32)
    near, sums, _ = P.step(src, nrm, 0.11, qry, T.POSE, 0.07)
    flipped = P.step(src, (nrm * np.where(g.uniform(size=(len(src), 1)) < 0.5, -1, 1)).astype(f32), 0.11, qry, T.POSE, 0.07)[1]
    assert np.array_equal(sums, flipped) and sums[30] == 0 and sums[0] == (near >= 0).sum() > 1000      # every term is even in n
    odd = nrm.copy()
    hit = np.unique(near[near >= 0])
    odd[hit[0]], odd[hit[1]], odd[hit[2]] = (0, 0, 0), (np.nan, 1, 0), (0, np.inf, 0)
    odd[hit[3]] = (1e-30, 0, 0)                                                          # nn underflows to 0 in fp32: not used
    odd[hit[4]] = (3e19, 0, 0)                                                           # nn overflows: not used
    dropped = np.isin(near, hit[:5])
    _, osums, _ = P.step(src, odd, 0.11, qry, T.POSE, 0.07)
    assert np.isfinite(osums).all() and osums[30] == dropped.sum() >= 5 and osums[0] == sums[0] - dropped.sum() and osums[31] == sums[31]
    assert np.array_equal(P.used_normals(odd[hit[:6]]), [False] * 5 + [True])


@pytest.fixture(scope="module")
def reference_icp():
    a, n, b = P.plane_case()
    return a, n, b, P.icp(a, n, b, A.ICP_RADIUS, A.ICP_FINAL, A.ICP_SHRINK, A.ICP_ITERATIONS)


def test_reference_icp_converges_by_tolerance_in_a_quarter_of_the_steps(reference_icp):
    """The numbers align_plane_reference.py records (REF_PLANE_*), recomputed; and the claim itself: at most a quarter of point-to-point's 40 steps,
    closer to the truth than point-to-point's recorded answer in both rotation and translation."""
    a, n, b, out = reference_icp
    assert np.array_equal(np.abs(n[:, :3]).max(1) == 1, np.abs(n).sum(1) == 1) and (np.abs(n).sum(1) == 1).sum() > 4000      # planes: axis normals
    rot, tr = A.pose_error(out["pose"])
    print(f"reference point-to-plane ICP: {out['iterations']} steps, pairs {[h[0] for h in out['history']]}, rms {out['rms']:.4e}, rotation error "
          f"{rot:.4e} rad, translation error {tr:.4e}, updates {out['updates']}")
    assert out["converged"] and out["reason"] == "tolerance" and out["iterations"] == len(out["history"]) == P.REF_PLANE_STEPS
    assert out["iterations"] <= POINT_TO_POINT_STEPS // 4
    assert rot < A.REF_ROTATION_ERROR and tr < A.REF_TRANSLATION_ERROR
    assert abs(rot / P.REF_PLANE_ROTATION_ERROR - 1) < 0.01 and abs(tr / P.REF_PLANE_TRANSLATION_ERROR - 1) < 0.01
    assert tuple(h[0] for h in out["history"]) == P.REF_PLANE_PAIRS and out["pairs"] == 6100 and out["coverage"] == 1.0
    assert out["history"][0][2] == A.ICP_RADIUS and out["history"][-1][2] == A.ICP_FINAL
    last, before = out["updates"][-1], out["updates"][-2]
    assert max(last) < 1e-7 and max(before) > 1e-5          # the tolerances of 1e-6 sit between the last update that moved the pose and the jitter


def test_reference_icp_pose_carries_the_masks_like_the_true_pose(reference_icp):
    a, _, b, out = reference_icp
    rows = A.mask_rows(a)
    bits = [I.apply_bits(rows, *T.plan(a, A.TRANSFER_RADIUS, b, pose.astype(f32)), 0.0)[0] for pose in (A.TRUE_POSE, out["pose"])]
    same = 1 - np.array([sum(bin(int(w)).count("1") for w in row) for row in bits[0] ^ bits[1]]) / len(b)
    print(f"share of points with the same bit as under the true pose: {same.tolist()}")
    assert same.min() == P.REF_PLANE_MASK_SHARE >= A.REF_MASK_SHARE


# ------------------------------------------------------------------------------------------------ solve_plane
def _exact_sums(p, s, n):
    """The 32 sums of the correspondences p -> s with normals n, every query paired and used."""
    p, s, n = (np.asarray(v, dtype=np.float64) for v in (p, s, n))
    res = ((p - s) * n).sum(1)
    Jm = np.concatenate([np.cross(p, n), n], 1)
    return np.concatenate([[len(p), ((p - s) ** 2).sum(), (res * res).sum()], (Jm * res[:, None]).sum(0), (Jm.T @ Jm)[np.triu_indices(6)], [0, len(p)]])


def _box_cloud(g, n):
    """Points on three orthogonal planes and a sphere, with their normals: no motion is free."""
    pts = g.uniform(-1, 1, size=(n, 3))
    nrm = np.zeros((n, 3))
    for k in range(3):
        pts[k::4, k] = -1.0
        nrm[k::4, k] = 1.0
    d = g.normal(size=(len(pts[3::4]), 3))
    nrm[3::4] = d / np.linalg.norm(d, axis=1, keepdims=True)
    pts[3::4] = 0.3 * nrm[3::4] + [0.2, -0.1, 0.3]
    return pts, nrm


def test_solve_plane_equals_the_reference_solve_and_recovers_a_small_motion():
    g = np.random.default_rng(1)
    s, n = _box_cloud(g, 800)
    Rm, t = A.rotation([1.0, 2.0, -0.5], 0.02), np.array([3e-4, -2e-4, 1e-4])             # 0.02 degrees
    x = (s - t) @ Rm                                                                      # s = R x + t
    start = np.concatenate([A.rotation([0.0, 0.0, 1.0], 0.5), [[0.001], [0.0], [0.0]]], 1)
    for pose in (IDENTITY, start):
        p = x @ pose[:, :3].T + pose[:, 3]
        m = _exact_sums(p, s, n)
        new, rms, rot, tr = X.solve_plane(m, pose)
        want, wrms, wrot, wtr = P.solve(m, pose)
        assert new.shape == (3, 4) and new.dtype == np.float64
        assert np.abs(new - want).max() < 1e-12 and abs(rms - wrms) < 1e-12 and abs(rot - wrot) < 1e-12 and abs(tr - wtr) < 1e-12
        assert abs(np.linalg.det(new[:, :3]) - 1) < 1e-12 and np.abs(new[:, :3] @ new[:, :3].T - np.eye(3)).max() < 1e-12
        err = A.pose_error(new, np.concatenate([Rm, t[:, None]], 1))
        # one Gauss-Newton step from at most 9.7e-3 away (0.5 degrees and 1e-3): what the linearisation leaves is of the order of its square, 1e-4
        assert err[0] < 1e-4 and err[1] < 1e-4 and rms < 1e-4 and rot > 1e-4
    # the sign of the normals does not change the answer
    flip = np.where(g.uniform(size=(len(n), 1)) < 0.5, -1.0, 1.0)
    a, b = X.solve_plane(_exact_sums(x, s, n), IDENTITY), X.solve_plane(_exact_sums(x, s, n * flip), IDENTITY)
    assert np.abs(a[0] - b[0]).max() < 1e-13 and abs(a[1] - b[1]) < 1e-13
    # a zero update leaves the pose alone: R is its own projection
    still = X.solve_plane(_exact_sums(s, s, n), start)
    assert np.abs(still[0] - start).max() < 1e-12 and still[1:] == (0.0, 0.0, 0.0)


def test_solve_plane_refuses_a_single_plane_few_pairs_and_bad_sums():
    g = np.random.default_rng(2)
    flat = np.concatenate([g.uniform(-1, 1, size=(300, 2)), np.full((300, 1), 0.25)], 1)
    up = np.tile([0.0, 0.0, 1.0], (300, 1))
    m = _exact_sums(flat + [0.0, 0.0, 0.01], flat, up)
    lam = np.linalg.eigvalsh(np.array([[m[9 + P.TRIU.index((min(a, b), max(a, b)))] for b in range(6)] for a in range(6)]))
    assert (np.abs(lam[:3]) < 1e-10 * lam[-1]).all() and lam[3] > 1e-3 * lam[-1]            # three motions free: sliding in x and y, turning about z
    with pytest.raises(ValueError, match="degenerate"):
        X.solve_plane(m, IDENTITY)
    with pytest.raises(ValueError, match="degenerate"):
        P.solve(m, IDENTITY)
    s, n = _box_cloud(g, 800)
    with pytest.raises(ValueError, match="degenerate: fewer than 6"):
        X.solve_plane(_exact_sums(s[:5], s[:5], n[:5]), IDENTITY)
    with pytest.raises(ValueError, match="degenerate"):
        X.solve_plane(np.zeros(32), IDENTITY)
    with pytest.raises(ValueError, match="degenerate"):
        X.solve_plane(_exact_sums(s, s, n), IDENTITY, condition=0.5)
    X.solve_plane(_exact_sums(s, s, n), IDENTITY)
    for bad in (np.zeros(20), np.full(32, np.nan)):
        with pytest.raises(ValueError, match="32 finite"):
            X.solve_plane(bad, IDENTITY)
    for pose in (np.eye(4), np.full((3, 4), np.inf)):
        with pytest.raises(ValueError, match="pose"):
            X.solve_plane(_exact_sums(s, s, n), pose)


# ------------------------------------------------------------------------------------------------ PlaneConfig, Snapshot
def test_plane_config_refuses_bad_values_and_unknown_fields():
    cfg = X.PlaneConfig()
    assert dataclasses.asdict(cfg) == dict(tol_rotation=1e-6, tol_translation=1e-6, condition=1e-10)
    assert (P.TOL_ROTATION, P.TOL_TRANSLATION, P.CONDITION) == (cfg.tol_rotation, cfg.tol_translation, cfg.condition)
    with pytest.raises(dataclasses.FrozenInstanceError):
        cfg.condition = 0.1
    for bad in (dict(tol_rotation=0), dict(tol_rotation=-1e-3), dict(tol_translation=float("nan")), dict(tol_translation=float("inf")),
                dict(tol_rotation="small"), dict(tol_translation=True), dict(condition=0), dict(condition=1.0), dict(condition=2), dict(condition=None)):
        with pytest.raises(ValueError):
            X.PlaneConfig(**bad)
    assert X.PlaneConfig.from_overrides({}) == cfg and X.PlaneConfig.from_overrides({"tol_rotation": 1e-4, "condition": 1e-6}) == X.PlaneConfig(1e-4, 1e-6, 1e-6)
    for bad in ({"tol_rotatoin": 1e-4}, {"radius": 0.1}, [1e-6], None, 3, {"condition": 0}):
        with pytest.raises(ValueError):
            X.PlaneConfig.from_overrides(bad)
    assert "tuned" in X.PlaneConfig.__doc__ and "ulp" in X.PlaneConfig.__doc__
    # AlignConfig is the one it was
    assert [f.name for f in dataclasses.fields(X.AlignConfig)] == ["radius", "final_radius", "shrink", "iterations", "min_pairs", "tol_rotation", "tol_translation"]


def test_snapshot_has_an_optional_fourth_field_and_its_shape_is_checked():
    from point_sam_amd import transfer as S
    snap = S.Snapshot(torch.zeros(5, 3), torch.zeros(2, 5), 2)
    assert snap.normals is None and S.check_snapshot(snap, "t") is snap
    assert [f.name for f in dataclasses.fields(S.Snapshot)] == ["coords", "logits", "num_masks", "normals"]
    full = S.Snapshot(torch.zeros(5, 3), torch.zeros(2, 5), 2, torch.zeros(5, 3))
    assert S.check_snapshot(full, "t") is full
    for bad in (torch.zeros(4, 3), torch.zeros(5, 4), torch.zeros(5, 3, dtype=torch.float64), torch.zeros(15), [[0.0] * 3] * 5):
        with pytest.raises(ValueError, match="normals"):
            S.check_snapshot(S.Snapshot(torch.zeros(5, 3), torch.zeros(2, 5), 2, bad), "t")


def test_predictor_align_plane_needs_the_snapshots_normals():
    from point_sam_amd import transfer as S
    from point_sam_amd.predictor import PointSAMPredictor
    pred = PointSAMPredictor(None)
    cfg = X.AlignConfig(0.1)
    bare = S.Snapshot(torch.zeros(5, 3), torch.zeros(2, 5), 2)
    for plane in (True, X.PlaneConfig()):
        with pytest.raises(ValueError, match=r"snapshot\(\.\.\., normals=True\)"):
            pred.align(bare, cfg, plane=plane)
    full = S.Snapshot(torch.zeros(5, 3), torch.zeros(2, 5), 2, torch.zeros(5, 3))
    for plane in ({"condition": 1e-6}, 1e-6, False):
        with pytest.raises(TypeError, match="PlaneConfig"):
            pred.align(full, cfg, plane=plane)
    with pytest.raises(RuntimeError, match="set_scene"):      # good arguments get as far as the cloud
        pred.align(full, cfg, plane=True)
    with pytest.raises(RuntimeError, match="set_scene"):
        pred.align(full, cfg, search=X.SearchConfig(), plane=X.PlaneConfig())


# ------------------------------------------------------------------------------------------------ the host loop
def _reference_step(src, r_index, want_normals, log=None):
    def step(index, xyz, normals, pose, radius, bits):
        assert index == "index" and bits is None and normals is want_normals
        m = P.step(src, normals, r_index, xyz, np.asarray(pose, dtype=np.float64).astype(f32), radius)[1]
        if log is not None:
            log.append(m)
        return m
    return step


def test_icp_host_loop_equals_the_reference_loop(reference_icp):
    """align.icp(normals=...) with the reference's step in place of ops.align_plane_step: the same schedule, the same stop, the same pose."""
    a, n, b, ref = reference_icp
    cfg = X.AlignConfig(A.ICP_RADIUS, A.ICP_FINAL, A.ICP_SHRINK, A.ICP_ITERATIONS)
    log = []
    out = X.icp("index", b, cfg, step=_reference_step(a, A.ICP_RADIUS, n, log), normals=n)
    assert out.converged and out.reason == "tolerance" and out.iterations == ref["iterations"] == len(out.history) == len(log)
    assert np.abs(out.pose - ref["pose"]).max() < 1e-12 and out.pairs == ref["pairs"] and out.coverage == ref["coverage"] and abs(out.rms - ref["rms"]) < 1e-12
    assert [h[0] for h in out.history] == [h[0] for h in ref["history"]] and [h[2] for h in out.history] == [h[2] for h in ref["history"]]
    assert all(len(h) == 3 for h in out.history) and out.search is None
    same = X.icp("index", b, cfg, step=_reference_step(a, A.ICP_RADIUS, n), normals=n, plane=X.PlaneConfig())      # None means the defaults
    assert np.array_equal(same.pose, out.pose) and same.history == out.history
    # looser tolerances end a step earlier, tighter ones than the jitter never by tolerance
    fast = dataclasses.replace(cfg, shrink=0.8)                                           # the final radius from step 2 on: the tolerances decide
    usual = X.icp("index", b, fast, step=_reference_step(a, A.ICP_RADIUS, n), normals=n)
    loose = X.icp("index", b, fast, step=_reference_step(a, A.ICP_RADIUS, n), normals=n, plane=X.PlaneConfig(1e-4, 1e-4))
    assert usual.converged and loose.converged and usual.reason == loose.reason == "tolerance" and 3 <= loose.iterations < usual.iterations
    assert loose.history == usual.history[:loose.iterations]
    tight = X.icp("index", b, dataclasses.replace(cfg, iterations=8), step=_reference_step(a, A.ICP_RADIUS, n), normals=n, plane=X.PlaneConfig(1e-12, 1e-12))
    assert tight.reason in ("iterations", "fixed point") and tight.iterations > ref["iterations"]
    # out of iterations: unconverged, the pose of the last step
    short = X.icp("index", b, dataclasses.replace(cfg, iterations=3), step=_reference_step(a, A.ICP_RADIUS, n), normals=n)
    assert not short.converged and short.reason == "iterations" and short.iterations == 3 and len(short.history) == 3
    # coverage is word [0] over word [31], and AlignConfig's own tolerances play no part
    m = log[-1].copy()
    m[0], m[30] = m[0] - 100, 100
    one = X.icp("index", b, X.AlignConfig(A.ICP_FINAL, iterations=1, tol_rotation=1.0, tol_translation=1.0), init=ref["pose"],
                step=lambda *a: m, normals=n, plane=X.PlaneConfig(1e-12, 1e-12))
    assert one.pairs == 6000 and one.coverage == 6000 / 6100 and not one.converged and one.reason == "iterations"


def test_icp_host_loop_stops_on_few_used_pairs_and_a_single_plane():
    a, n, b = P.plane_case()
    cfg = X.AlignConfig(A.ICP_RADIUS)
    # every query has a pair, but only 15 sources carry a normal: word [0] is what min_pairs looks at
    few = np.zeros_like(n)
    near = A.step(a, A.ICP_RADIUS, b, IDENTITY.astype(f32))[0]
    keep = np.unique(near[near >= 0])[:3]
    few[keep] = n[keep]
    used = int(np.isin(near, keep).sum())
    assert 3 <= used < 16
    out = X.icp("index", b, cfg, step=_reference_step(a, A.ICP_RADIUS, few), normals=few)
    assert not out.converged and out.reason == f"pairs: {used} < min_pairs 16" and out.iterations == 1 and out.pairs == 0
    assert np.array_equal(out.pose, IDENTITY) and out.history == [(used, pytest.approx(float("nan"), nan_ok=True), A.ICP_RADIUS)]
    # the floor alone: a single plane
    floor = np.where((n[:, 2:3] == 1), n, 0).astype(f32)
    out = X.icp("index", b, cfg, step=_reference_step(a, A.ICP_RADIUS, floor), normals=floor)
    assert not out.converged and "degenerate" in out.reason and out.iterations == 1 and np.array_equal(out.pose, IDENTITY)


def _host_loop_cases():
    """(name, a run of align.icp on a stand-in step) for every way the host loop ends, point to point and point to plane, on the fixtures of
    align_reference.py and align_plane_reference.py."""
    a, n, b = P.plane_case()
    cfg = X.AlignConfig(A.ICP_RADIUS, A.ICP_FINAL, A.ICP_SHRINK, A.ICP_ITERATIONS)

    def point(r_index):
        return lambda index, xyz, pose, radius, bits: A.step(a, r_index, xyz, np.asarray(pose, dtype=np.float64).astype(f32), radius)[1]
    done = X.icp("index", b, cfg, step=point(A.ICP_RADIUS))
    yield "point", done
    yield "point, out of iterations", X.icp("index", b, dataclasses.replace(cfg, iterations=3), step=point(A.ICP_RADIUS))
    # started at the fixed point with tolerances set: the words repeat AND the update is small
    yield "point, fixed and small", X.icp("index", b, X.AlignConfig(A.ICP_FINAL, tol_rotation=1e-4, tol_translation=1e-4), init=done.pose,
                                          step=point(A.ICP_FINAL))
    # one step short of the fixed point, generous tolerances: small alone
    yield "point, small", X.icp("index", b, X.AlignConfig(A.ICP_FINAL, tol_rotation=1e-2, tol_translation=1e-2), init=A.TRUE_POSE, step=point(A.ICP_FINAL))
    yield "point, few pairs", X.icp("index", (b + f32(5.0)).astype(f32), X.AlignConfig(A.ICP_RADIUS), step=point(A.ICP_RADIUS))
    line = np.outer(np.linspace(-0.5, 0.5, 40), [1.0, 0.5, 0.25]).astype(f32)
    yield "point, collinear", X.icp("index", line, X.AlignConfig(0.1), step=lambda index, xyz, pose, radius, bits: A.step(line, 0.1, xyz, None, radius)[1])

    log = []
    plane = _reference_step(a, A.ICP_RADIUS, n, log)
    done = X.icp("index", b, cfg, step=plane, normals=n)
    yield "plane", done
    yield "plane, out of iterations", X.icp("index", b, dataclasses.replace(cfg, iterations=3), step=plane, normals=n)
    yield "plane, tight", X.icp("index", b, dataclasses.replace(cfg, iterations=8), step=plane, normals=n, plane=X.PlaneConfig(1e-12, 1e-12))
    # sums whose gradient [3..8] is zero: the update is exactly zero, so the words repeat AND the update is small
    still = log[len(done.history) - 1].copy()
    still[3:9] = 0.0
    yield "plane, fixed and small", X.icp("index", b, X.AlignConfig(A.ICP_FINAL), init=IDENTITY, step=lambda *args: still, normals=n)
    few = np.zeros_like(n)
    near = A.step(a, A.ICP_RADIUS, b, IDENTITY.astype(f32))[0]
    keep = np.unique(near[near >= 0])[:3]
    few[keep] = n[keep]
    yield "plane, few used pairs", X.icp("index", b, X.AlignConfig(A.ICP_RADIUS), step=_reference_step(a, A.ICP_RADIUS, few), normals=few)
    floor = np.where((n[:, 2:3] == 1), n, 0).astype(f32)
    yield "plane, one plane", X.icp("index", b, X.AlignConfig(A.ICP_RADIUS), step=_reference_step(a, A.ICP_RADIUS, floor), normals=floor)


def _alignment_record(out):
    """An Alignment as JSON holds it: every float in float.hex, so that nothing is lost and a NaN has a spelling."""
    h = lambda v: float(v).hex()
    return dict(pose=[h(v) for v in np.asarray(out.pose).reshape(-1)], pairs=out.pairs, coverage=h(out.coverage), rms=h(out.rms), iterations=out.iterations,
                converged=out.converged, reason=out.reason, history=[[p, h(rms), h(radius)] for p, rms, radius in out.history], search=out.search)


def test_icp_runs_one_loop_with_the_results_of_the_two_it_replaced():
    """align.icp ran two copies of its loop, one per kind of step, until they became one.  tests/golden/align_icp_loops.json holds what the two copies
    returned for _host_loop_cases() -- every field of the Alignment, history, reason and iterations included, every float as float.hex -- recorded
    with the last commit that had both.  The one loop must return the same, field for field.  In particular the reason when the fp32 words repeat AND
    the update is small stays "fixed point" for point to point and "tolerance" for point to plane."""
    import json
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "align_icp_loops.json")))
    got = {name: _alignment_record(out) for name, out in _host_loop_cases()}
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
    assert got["point, fixed and small"]["reason"] == "fixed point" and got["plane, fixed and small"]["reason"] == "tolerance"
    assert {r["reason"].split(":")[0] for r in want.values()} == {"fixed point", "tolerance", "iterations", "pairs", "degenerate"}


def test_plane_without_normals_and_other_bad_arguments_are_refused():
    b = np.zeros((10, 3), dtype=f32)
    cfg = X.AlignConfig(0.1)
    with pytest.raises(ValueError, match="needs normals"):
        X.icp("index", b, cfg, plane=X.PlaneConfig())
    with pytest.raises(ValueError, match="needs normals"):
        X.search("index", b, X.SearchConfig(), cfg, plane=X.PlaneConfig())
    with pytest.raises(TypeError, match="PlaneConfig"):
        X.icp("index", b, cfg, normals=b, plane={"condition": 1e-6})
    with pytest.raises(TypeError, match="AlignConfig"):
        X.icp("index", b, {"radius": 0.1}, normals=b)
    with pytest.raises(ValueError, match="pose"):
        X.icp("index", b, cfg, init=np.eye(3), normals=b)


def test_search_passes_normals_and_plane_to_its_refinements():
    a, n, b = P.plane_case()
    seen = []

    def step(index, xyz, normals, pose, radius, bits):
        seen.append(normals)
        return P.step(a, normals, A.ICP_RADIUS, xyz, np.asarray(pose, dtype=np.float64).astype(f32), radius)[1]
    index = type("Index", (), {"src_xyz": a})()
    cfg = X.AlignConfig(A.ICP_RADIUS, A.ICP_FINAL, A.ICP_SHRINK, A.ICP_ITERATIONS)
    out = X.search(index, b, X.SearchConfig(yaw_steps=1, keep=1, sample=64), cfg, score=lambda ix, q, poses, r: np.zeros(len(poses), dtype=np.int32),
                   step=step, normals=n, plane=X.PlaneConfig(1e-4, 1e-4))
    assert seen and all(s is n for s in seen) and out.search.poses == 1 and out.reason in ("tolerance", "iterations") and len(out.history[0]) == 3


# ------------------------------------------------------------------------------------------------ the C entry points
def test_plane_entry_points_are_declared_bound_and_exported():
    from point_sam_amd import ops
    from point_sam_amd.build import SOURCES, build_library
    build_library()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pointsam_hip.h")).read()
    declared = set(re.findall(r"\b(psam_plane_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(PLANE_ENTRY_POINTS) == {n for n in _lib.SIGNATURES if n.startswith("psam_plane_")}
    for n in PLANE_ENTRY_POINTS:
        assert hasattr(lib, n), n
    assert re.search(r"#define PSAM_PLANE_SUMS 32\b", hdr) and re.search(r"#define PSAM_ALIGN_SUMS 20\b", hdr)
    assert hdr.index("pose between two clouds") < hdr.index("#define PSAM_PLANE_SUMS") < hdr.index("PSAM_ALIGN_SCORE_POSES")
    assert ops.PLANE_SUMS == 32 == P.SUMS and ops.ALIGN_SUMS == 20
    assert _lib.SIGNATURES["psam_plane_step"][1] == _lib.SIGNATURES["psam_align_step"][1][:1] + [_lib.ptr] + _lib.SIGNATURES["psam_align_step"][1][1:]
    assert dict(SOURCES)["align_plane.hip"] == dict(SOURCES)["align.hip"] == ["-ffp-contract=off", "-fno-slp-vectorize"]
    csrc = os.path.join(ROOT, "point_sam_amd", "csrc")
    src = open(os.path.join(csrc, "align_plane.hip")).read()
    assert "atomic" not in src.replace("no atomics", "") and "order of every fp64 addition is a function of M" in src
    # one copy of the posed coordinate, the cell, the candidate walk and the second kernel: both steps take them from the shared headers
    for name, header in (("bool transfer_cell(", "transfer_index.h"), ("void transfer_candidates(", "transfer_index.h"), ("void pose_apply(", "rigid_pose.h"),
                         ("void align_combine_kernel(", "align_combine.h"), ("int64_t align_waves(", "align_combine.h"), ("bool align_zero_row(", "align_combine.h"),
                         ("void align_store_row(", "align_combine.h"), ("int32_t align_step_entry(", "align_combine.h")):
        assert name in open(os.path.join(csrc, header)).read(), name
        for f in ("align.hip", "align_plane.hip"):
            text = open(os.path.join(csrc, f)).read()
            assert name not in text and f'#include "{header}"' in text, (f, name)


def test_plane_entry_points_reject_bad_arguments_on_the_host():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 15) & ~15               # a non-null, aligned pointer; never dereferenced by the device: every call below is refused
    org = (ctypes.c_float * 3)(-1.0, -1.0, -1.0)
    bad_org = (ctypes.c_float * 3)(-1.0, float("nan"), -1.0)
    bad_pose = (ctypes.c_float * 12)(*([0.0] * 11 + [float("inf")]))

    def refused(status, code, text):      # the whole text, as the entry worded it before its checks moved into the shared headers
        assert status == code, (status, lib.psam_last_error_string())
        assert lib.psam_last_error_string() == b"psam_plane_step: " + text, lib.psam_last_error_string()
    aligned = b"index_ws must be 16-byte aligned, sums, ws and qry_bits 8-byte aligned, src, src_normals, qry and nearest 4-byte aligned"
    small = b"workspace too small (psam_plane_workspace_bytes)"

    size = lib.psam_plane_workspace_bytes
    assert size(1) == size(64) == 256 and size(65) == 512 and size(6007) == 94 * 256 and size(1 << 28) == (1 << 22) * 256
    assert size(0) == 0 and size(-1) == 0 and size((1 << 28) + 1) == 0
    N, M, big = 1000, 100, 1 << 20
    good = dict(src=p, src_normals=p, N=N, index_ws=p, index_ws_bytes=big, origin=ctypes.addressof(org), inv_h=4.0, r2=0.0625, qry=p, M=M, qry_bits=None,
                pose=None, nearest=None, sums=p, ws=p, ws_bytes=big)
    call = lambda **kw: lib.psam_plane_step(*{**good, **kw}.values(), None)
    for name in ("src", "src_normals", "index_ws", "origin", "qry", "sums", "ws"):
        refused(call(**{name: None}), -1, b"null pointer")
    for name, word in (("N", b"need 0 < N <= 2^28"), ("M", b"need 0 < M <= 2^28")):
        for bad in (0, -5, (1 << 28) + 1):
            refused(call(**{name: bad}), -1, word)
    for name in ("inv_h", "r2"):
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            refused(call(**{name: bad}), -1, name.encode() + b" must be finite and positive")
    refused(call(origin=ctypes.addressof(bad_org)), -1, b"origin must be finite")
    refused(call(pose=ctypes.addressof(bad_pose)), -1, b"pose must be finite")
    refused(call(index_ws=p + 8), -2, aligned)
    for name in ("sums", "ws", "qry_bits"):
        refused(call(**{name: p + 4}), -2, aligned)
    for name in ("src", "src_normals", "qry", "nearest"):
        refused(call(**{name: p + 2}), -2, aligned)
    refused(call(index_ws_bytes=lib.psam_transfer_index_workspace_bytes(N) - 1), -3, b"index workspace too small (psam_transfer_index_workspace_bytes)")
    refused(call(ws_bytes=size(M) - 1), -3, small)
    refused(call(ws_bytes=lib.psam_align_workspace_bytes(M)), -3, small)      # the point-to-point size does not do
    # the order of psam_align_step: a null pointer before a range, a range before an alignment, an alignment before a size
    refused(call(src_normals=None, N=0), -1, b"null pointer")
    refused(call(N=0, qry=p + 2), -1, b"need 0 < N <= 2^28")
    refused(call(src_normals=p + 2, ws_bytes=0), -2, aligned)


# ------------------------------------------------------------------------------------------------ ops
def test_align_plane_step_refuses_bad_arguments_before_the_library_is_touched(monkeypatch):
    from point_sam_amd import ops

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_library)
    index = ops.TransferIndex(torch.zeros(8, dtype=torch.int64), torch.zeros(10, 3), f32(0.25), f32(4), f32(0.0625), (-1.0, -1.0, -1.0))
    xyz, nrm = torch.zeros(100, 3), torch.zeros(10, 3)
    with pytest.raises(TypeError, match="TransferIndex"):
        ops.align_plane_step("index", xyz, nrm)
    with pytest.raises(TypeError):
        ops.align_plane_step(index, xyz.double(), nrm)
    with pytest.raises(ValueError):
        ops.align_plane_step(index, torch.zeros(100, 2), nrm)
    for bad in (torch.zeros(9, 3), torch.zeros(10, 4), torch.zeros(30), torch.zeros(100, 3), torch.zeros(1, 10, 3)):
        with pytest.raises(ValueError, match="normals"):
            ops.align_plane_step(index, xyz, bad)
    for bad in (nrm.double(), nrm.half(), np.zeros((10, 3), dtype=f32), None):
        with pytest.raises(TypeError, match="normals"):
            ops.align_plane_step(index, xyz, bad)
    with pytest.raises(ValueError, match="normals are on"):
        ops.align_plane_step(index, xyz, nrm.to("meta"))
    for radius in (0.26, 1.0):
        with pytest.raises(ValueError, match="exceeds"):
            ops.align_plane_step(index, xyz, nrm, radius=radius)
    for radius in (0, -0.1, float("nan"), "r", True):
        with pytest.raises(ValueError, match="radius"):
            ops.align_plane_step(index, xyz, nrm, radius=radius)
    for pose in (np.eye(3), np.diag([1.0, 1, 1, 2]), np.full((3, 4), np.nan), "pose"):
        with pytest.raises(ValueError, match="pose"):
            ops.align_plane_step(index, xyz, nrm, pose)
    for bits in (torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int64), [0, 0]):
        with pytest.raises(ValueError, match="bits"):
            ops.align_plane_step(index, xyz, nrm, bits=bits)
    # good arguments on the CPU get as far as the device check, still without the library
    with pytest.raises(_lib.PointSamHipError, match="GPU"):
        ops.align_plane_step(index, xyz, nrm, np.eye(4), 0.25, torch.zeros(2, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------ the demo route
class FakePlaneAligner:
    """tests/test_align_cpu.py's stand-in predictor with the `normals` and `plane` arguments: it answers with a fixed Alignment and logs what it was given."""
    POSE = np.array([[1.0, 0.0, 0.0, 0.125], [0.0, 1.0, 0.0, -0.25], [0.0, 0.0, 1.0, 0.5]])

    def __init__(self):
        self.log = []

    def set_pointcloud(self, xyz, rgb):
        self.xyz = xyz

    def predict_masks(self, pts, labels, prompt_mask, multimask):
        logit = 0.5 - (self.xyz[0] - pts[0][-1]).norm(dim=-1)
        return logit[None, None], torch.tensor([[0.9]]), logit[None, None]

    def snapshot(self, logits, **kw):
        self.log.append(("snapshot", kw))
        return ("snap", logits.clone())

    def align(self, snap, cfg, init=None, mask=None, **kw):
        self.log.append(("align", cfg, init, mask, kw))
        out = X.Alignment(self.POSE.copy(), 41, 0.82, 0.0125, 5, True, "tolerance", [(41, 0.0125, cfg.radius)] * 5)
        if "search" in kw:
            out.search = X.SearchRecord(72, 50, [dict(pose_index=3, count=38, pairs=41, rms=0.0125, converged=True)], 0)
        return out

    def propagate(self, snap, radius, pose=None):
        from point_sam_amd.transfer import Propagated
        self.log.append(("propagate", radius, pose))
        K = snap[1].shape[0]
        return Propagated(snap[1].clone(), torch.full((K,), 0.75), torch.zeros(K, dtype=torch.bool), torch.ones(K, dtype=torch.int64), 1.0,
                          torch.zeros(K, 1, 3), torch.ones(K, 1, dtype=torch.bool))


def test_propagate_route_with_plane(tmp_path):
    import http.client
    import json
    import threading
    from point_sam_amd.demo_server import DemoSession, serve
    pts = np.random.RandomState(0).rand(50, 3) * 4 + 1
    for name, cloud in (("scan0.ply", pts), ("scan1.ply", pts[::-1] + 0.25)):
        with open(tmp_path / name, "w") as f:
            f.write(f"ply\nformat ascii 1.0\nelement vertex {len(cloud)}\nproperty float x\nproperty float y\nproperty float z\n"
                    "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
            f.writelines(f"{p[0]} {p[1]} {p[2]} 255 0 128\n" for p in cloud)
    pred = FakePlaneAligner()
    sess = DemoSession(pred, models_dir=str(tmp_path), output_dir=str(tmp_path / "results"), device="cpu")
    srv = serve(sess, "127.0.0.1", 0)
    threading.Thread(target=srv.serve_forever, daemon=True).start()

    def req(method, path, body=None):
        c = http.client.HTTPConnection("127.0.0.1", srv.server_address[1], timeout=10)
        c.request(method, path, None if body is None else json.dumps(body), {"Content-Type": "application/json"})
        r = c.getresponse()
        return r.status, json.loads(r.read())

    def first_scan_with_a_mask():
        sess.masks.clear()
        _, out = req("GET", "/pointcloud/scan0.ply")
        assert req("POST", "/segment", {"prompt_point": out["xyz"][9:12], "prompt_label": 1})[0] == 200
        pred.log.clear()

    try:
        body = {"pointcloud": "scan1.ply", "radius": 0.1}
        align = {"radius": 0.2, "final_radius": 0.05, "shrink": 0.5}
        given = [[1, 0, 0, 0.01], [0, 1, 0, 0], [0, 0, 1, 0]]
        # "plane" without "align", or with a bad field: this request's 400, before anything is loaded or snapshot
        first_scan_with_a_mask()
        for bad in (dict(body, plane={}), dict(body, pose=given, plane={}), dict(body, align=align, plane={"tol_rotation": 0}),
                    dict(body, align=align, plane={"radius": 0.1}), dict(body, align=align, plane=1e-6), dict(body, align=align, plane=None),
                    dict(body, align=align, plane={"condition": 1.5})):
            st, out = req("POST", "/propagate", bad)
            assert st == 400 and "error" in out and sess.obj_path == "scan0.ply" and pred.log == [], bad
        # with both: the snapshot is taken with normals and predictor.align gets the PlaneConfig; the response has the fields of "align" alone
        st, out = req("POST", "/propagate", dict(body, align=align, pose=given, plane={"tol_rotation": 1e-5}))
        assert st == 200, out
        assert pred.log[0] == ("snapshot", {"normals": True})
        assert pred.log[1] == ("align", X.AlignConfig(0.2, 0.05, 0.5), given, None, {"plane": X.PlaneConfig(tol_rotation=1e-5)})
        assert pred.log[2] == ("propagate", 0.1, FakePlaneAligner.POSE.tolist()) and len(pred.log) == 3
        assert out["pose"] == FakePlaneAligner.POSE.tolist()
        assert out["align"] == {"pairs": 41, "coverage": 0.82, "rms": 0.0125, "iterations": 5, "converged": True}
        # an empty "plane" is the defaults; beside "search" both reach the predictor
        first_scan_with_a_mask()
        st, both = req("POST", "/propagate", dict(body, align=align, search={"keep": 2}, plane={}))
        assert st == 200, both
        kind, cfg, init, mask, kw = pred.log[1]
        assert pred.log[0] == ("snapshot", {"normals": True}) and kind == "align" and init is None and set(kw) == {"search", "plane"}
        assert kw["plane"] == X.PlaneConfig() and kw["search"].keep == 2 and both["align"]["search"]["poses"] == 72
        # without "plane": the calls and the answer of before -- no `normals` reaches snapshot, no `plane` reaches align
        first_scan_with_a_mask()
        st, plain = req("POST", "/propagate", dict(body, align=align, pose=given))
        assert st == 200 and pred.log[0] == ("snapshot", {}) and pred.log[1] == ("align", X.AlignConfig(0.2, 0.05, 0.5), given, None, {})
        assert plain == out
    finally:
        srv.shutdown()
