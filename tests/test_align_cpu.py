"""The pose between two scans, the part that needs no GPU: solve_rigid, AlignConfig, the numpy reference (tests/align_reference.py) against its own
definition, the reference ICP on the fixture the GPU tests share, the host loop of align.icp driven by the reference step, the C entry points'
declarations and refusals, and every ValueError of ops.align_step raised before the library is touched."""
import ctypes
import dataclasses
import math
import os
import re

import numpy as np
import pytest
import torch

import align_reference as A
import interp_reference as I
import transfer_reference as T
from point_sam_amd import _lib
from point_sam_amd import align as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIGN_ENTRY_POINTS = ("psam_align_workspace_bytes", "psam_align_step")
f32 = np.float32


def _sums(x, s):
    """The 20 sums of exact correspondences x -> s (q = 0, every query paired)."""
    x, s = np.asarray(x, dtype=np.float64), np.asarray(s, dtype=np.float64)
    return np.concatenate([[len(x), 0.0], x.sum(0), s.sum(0), (x[:, :, None] * s[:, None, :]).sum(0).reshape(-1), [(x * x).sum(), (s * s).sum(), len(x)]])


# ------------------------------------------------------------------------------------------------ solve_rigid
def test_solve_rigid_recovers_a_known_motion():
    g = np.random.default_rng(1)
    x = g.normal(size=(500, 3))
    Rm, t = A.rotation([1.0, 2.0, -0.5], 37.0), np.array([0.3, -1.2, 0.7])
    pose, rms = X.solve_rigid(_sums(x, x @ Rm.T + t))
    assert pose.shape == (3, 4) and pose.dtype == np.float64
    assert np.abs(pose[:, :3] - Rm).max() < 1e-12 and np.abs(pose[:, 3] - t).max() < 1e-12
    assert rms < 1e-6                                      # the residual is a difference of sums of ~500: 1e-13 absolute, its root 1e-7
    # with noise the rms is the root mean square distance after the solve
    s = x @ Rm.T + t + g.normal(scale=0.01, size=x.shape)
    pose, rms = X.solve_rigid(_sums(x, s))
    want = math.sqrt(((x @ pose[:, :3].T + pose[:, 3] - s) ** 2).sum() / len(x))
    assert abs(rms - want) < 1e-9 and 0.015 < rms < 0.02
    # and the reference's independent solve agrees
    R2, t2, rms2 = A.solve(_sums(x, s))
    assert np.abs(pose[:, :3] - R2).max() < 1e-12 and np.abs(pose[:, 3] - t2).max() < 1e-12 and abs(rms - rms2) < 1e-9


def test_solve_rigid_returns_a_proper_rotation_on_planar_data():
    """Points of a plane (to 1e-6: the third singular value is tiny but its vectors are determined) mirrored through a plane across theirs: the
    uncorrected SVD answer V U^T is that reflection (det -1); the corrected one is the proper rotation that does the same to the points' plane (half a
    turn about the line the two planes share)."""
    g = np.random.default_rng(2)
    x = np.concatenate([g.normal(size=(200, 2)), g.normal(scale=1e-6, size=(200, 1))], 1)
    s = x * np.array([1.0, -1.0, 1.0])
    m = _sums(x, s)
    H = m[8:17].reshape(3, 3) - np.outer(m[2:5], m[5:8]) / m[0]
    U, _, Vt = np.linalg.svd(H)
    assert np.linalg.det(Vt.T @ U.T) < 0                   # the case the correction exists for
    pose, rms = X.solve_rigid(m)
    Rm = pose[:, :3]
    assert abs(np.linalg.det(Rm) - 1.0) < 1e-12 and np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-12
    assert np.abs(x @ Rm.T + pose[:, 3] - s).max() < 1e-5 and rms < 1e-5      # off by the 2e-6 the half turn does to the out-of-plane noise


def test_solve_rigid_refuses_collinear_points_and_fewer_than_three():
    line = np.outer(np.arange(10.0), [1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="degenerate"):
        X.solve_rigid(_sums(line, line + 1.0))
    with pytest.raises(ValueError, match="degenerate"):
        X.solve_rigid(_sums(np.eye(3)[:2], np.eye(3)[:2]))
    with pytest.raises(ValueError, match="degenerate"):
        X.solve_rigid(np.zeros(20))
    with pytest.raises(ValueError):
        X.solve_rigid(np.zeros(19))
    with pytest.raises(ValueError):
        X.solve_rigid(np.full(20, np.nan))
    X.solve_rigid(_sums(np.eye(3), np.eye(3)))             # three points that span a plane are enough


# ------------------------------------------------------------------------------------------------ AlignConfig
def test_align_config_refuses_bad_values_and_unknown_fields():
    cfg = X.AlignConfig(0.1)
    assert dataclasses.asdict(cfg) == dict(radius=0.1, final_radius=None, shrink=1.0, iterations=30, min_pairs=16, tol_rotation=0.0, tol_translation=0.0)
    with pytest.raises(dataclasses.FrozenInstanceError):
        cfg.radius = 0.2
    for bad in (dict(radius=0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")), dict(radius="r"), dict(radius=True),
                dict(radius=1e-30), dict(radius=0.1, final_radius=0.2), dict(radius=0.1, final_radius=0), dict(radius=0.1, final_radius="x"),
                dict(radius=0.1, shrink=0), dict(radius=0.1, shrink=1.5), dict(radius=0.1, shrink=None), dict(radius=0.1, iterations=0),
                dict(radius=0.1, iterations=2.5), dict(radius=0.1, iterations=True), dict(radius=0.1, min_pairs=2), dict(radius=0.1, min_pairs=1.0),
                dict(radius=0.1, tol_rotation=-1e-3), dict(radius=0.1, tol_translation=float("nan")), dict(radius=0.1, tol_rotation="small")):
        with pytest.raises(ValueError):
            X.AlignConfig(**bad)
    assert X.AlignConfig.from_overrides({"radius": 0.2, "shrink": 0.5, "final_radius": 0.05}) == X.AlignConfig(0.2, 0.05, 0.5)
    for bad in ({"shrink": 0.5}, {"radius": 0.2, "raduis": 1}, [0.2], None, {"radius": 0.2, "iterations": 0}):
        with pytest.raises(ValueError):
            X.AlignConfig.from_overrides(bad)
    assert "tuned" in X.AlignConfig.__doc__


def test_align_config_radius_schedule():
    cfg = X.AlignConfig(0.2, final_radius=0.05, shrink=0.5)
    assert [cfg.step_radius(k) for k in range(5)] == [0.2, 0.1, 0.05, 0.05, 0.05]
    assert [X.AlignConfig(0.2).step_radius(k) for k in (0, 7)] == [0.2, 0.2]
    assert [X.AlignConfig(0.2, shrink=0.5).step_radius(k) for k in (0, 3)] == [0.2, 0.2]      # without a final radius there is nothing to shrink to
    cfg = X.AlignConfig(A.ICP_RADIUS, A.ICP_FINAL, A.ICP_SHRINK)
    for k in range(12):
        assert cfg.step_radius(k) == A.radius_of_step(A.ICP_RADIUS, A.ICP_FINAL, A.ICP_SHRINK, k) == max(A.ICP_FINAL, A.ICP_RADIUS * A.ICP_SHRINK ** k)


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("radius", [None, 0.125])
def test_reference_step_equals_its_definition_on_the_lattice(radius):
    """The vectorised search equals the first entry of the (q, j)-sorted candidates, and on the lattice every sum is exact whatever the order."""
    src, qry, r = T.lattice_case()
    near, sums, mass = A.step(src, r, qry, None, radius)
    want, wsums, _ = A.step(src, r, qry, None, radius, definition=True)
    assert np.array_equal(near, want) and np.array_equal(sums, wsums)
    cands = T.candidates_grid(src, r, qry)
    r2 = A.r2_of(r if radius is None else radius)
    first = np.array([next((j for j, q in zip(js, qs) if q <= r2), -1) for js, qs in cands])
    assert np.array_equal(near, first)
    assert sums[0] == (near >= 0).sum() > 300 and sums[19] == 1173 and (near < 0).sum() > 300
    i = np.nonzero(near >= 0)[0]
    x, s = qry[i].astype(np.float64), src[near[i]].astype(np.float64)
    assert np.array_equal(sums[8:17], (x[:, :, None] * s[:, None, :]).sum(0).reshape(-1)) and sums[17] == (x * x).sum()      # exact in ANY order
    assert np.array_equal(mass[[0, 19]], sums[[0, 19]])


def test_reference_step_equals_its_definition_posed_and_on_a_subset():
    src, qry = T.uniform_case()
    take = np.random.default_rng(4).uniform(size=len(qry)) < 0.4
    near, sums, _ = A.step(src, 0.11, qry, T.POSE, 0.05, take)
    want, wsums, _ = A.step(src, 0.11, qry, T.POSE, 0.05, take, definition=True)
    assert np.array_equal(near, want) and np.array_equal(sums, wsums)
    assert (near[~take] == -1).all() and 0 < sums[0] < sums[19] <= take.sum()


@pytest.fixture(scope="module")
def reference_icp():
    a, b = A.icp_case()
    return a, b, A.icp(a, b, A.ICP_RADIUS, A.ICP_FINAL, A.ICP_SHRINK, A.ICP_ITERATIONS)


def test_reference_icp_converges_on_the_fixture(reference_icp):
    """The numbers align_reference.py records (REF_*), recomputed: the GPU tests' margins are ten times these errors."""
    a, b, out = reference_icp
    assert a.shape == (6000, 3) and b.shape == (6100, 3) and np.abs(a).max() < 1 and np.abs(b).max() < 1
    Rm = A.TRUE_POSE[:, :3]
    assert abs(math.degrees(math.acos((np.trace(Rm) - 1) / 2)) - 4.0) < 1e-9 and abs(np.linalg.norm(A.TRUE_POSE[:, 3]) - 0.03) < 1e-12
    start = A.pose_error(np.concatenate([np.eye(3), np.zeros((3, 1))], 1))
    assert out["converged"] and out["iterations"] < A.ICP_ITERATIONS, out["history"]
    assert out["history"][-1][2] == A.ICP_FINAL and out["history"][0][2] == A.ICP_RADIUS
    rot, tr = A.pose_error(out["pose"])
    print(f"reference ICP: {out['iterations']} steps, {out['pairs']} pairs, rms {out['rms']:.6f}, rotation error {rot:.4e} rad, translation error {tr:.4e}")
    assert rot < start[0] / 40 and tr < start[1] / 40                                 # from 4 degrees and 0.03
    assert abs(rot / A.REF_ROTATION_ERROR - 1) < 0.01 and abs(tr / A.REF_TRANSLATION_ERROR - 1) < 0.01
    assert out["pairs"] == 6100 and out["coverage"] == 1.0 and abs(out["rms"] - 0.01068) < 1e-5


def test_reference_icp_pose_carries_the_masks_like_the_true_pose(reference_icp):
    a, b, out = reference_icp
    rows = A.mask_rows(a)
    bits = [I.apply_bits(rows, *T.plan(a, A.TRANSFER_RADIUS, b, pose.astype(f32)), 0.0)[0] for pose in (A.TRUE_POSE, out["pose"])]
    same = 1 - np.array([sum(bin(int(w)).count("1") for w in row) for row in bits[0] ^ bits[1]]) / len(b)
    print(f"share of points with the same bit as under the true pose: {same.tolist()}")
    assert same.min() >= A.REF_MASK_SHARE and same.min() > 0.999


# ------------------------------------------------------------------------------------------------ the host loop
def _reference_step(src, r_index):
    def step(index, xyz, pose, radius, bits):
        assert index == "index" and bits is None
        return A.step(src, r_index, xyz, np.asarray(pose, dtype=np.float64).astype(f32), radius)[1]
    return step


def test_icp_host_loop_equals_the_reference_loop(reference_icp):
    """align.icp with the reference's step in place of ops.align_step: the same schedule, the same stops, the same pose as the independent loop."""
    a, b, ref = reference_icp
    cfg = X.AlignConfig(A.ICP_RADIUS, A.ICP_FINAL, A.ICP_SHRINK, A.ICP_ITERATIONS)
    out = X.icp("index", b, cfg, step=_reference_step(a, A.ICP_RADIUS))
    assert out.converged and out.reason == "fixed point" and out.iterations == ref["iterations"] == len(out.history)
    assert np.abs(out.pose - ref["pose"]).max() < 1e-12 and out.pairs == ref["pairs"] and out.coverage == ref["coverage"] and abs(out.rms - ref["rms"]) < 1e-9
    assert [h[0] for h in out.history] == [h[0] for h in ref["history"]] and [h[2] for h in out.history] == [h[2] for h in ref["history"]]
    # out of iterations: unconverged, the pose of the last step
    short = X.icp("index", b, dataclasses.replace(cfg, iterations=3), step=_reference_step(a, A.ICP_RADIUS))
    assert not short.converged and short.reason == "iterations" and short.iterations == 3 and len(short.history) == 3
    # started at the answer with tolerances set: one step at the final radius meets them
    tol = X.icp("index", b, X.AlignConfig(A.ICP_FINAL, tol_rotation=1e-4, tol_translation=1e-4), init=ref["pose"], step=_reference_step(a, A.ICP_FINAL))
    assert tol.converged and tol.iterations <= 2 and tol.reason in ("tolerance", "fixed point")


def test_icp_host_loop_stops_on_few_pairs_and_degenerate_pairs():
    a, b = A.icp_case()
    far = (b + f32(5.0)).astype(f32)
    cfg = X.AlignConfig(A.ICP_RADIUS)
    init = np.concatenate([np.eye(3), [[0.0], [0.0], [0.5]]], 1)
    out = X.icp("index", far, cfg, init=init, step=_reference_step(a, A.ICP_RADIUS))
    assert not out.converged and "min_pairs" in out.reason and out.iterations == 1 and out.pairs == 0
    assert np.array_equal(out.pose, init) and out.history == [(0, pytest.approx(float("nan"), nan_ok=True), A.ICP_RADIUS)]
    line = np.outer(np.linspace(-0.5, 0.5, 40), [1.0, 0.5, 0.25]).astype(f32)
    out = X.icp("index", line, X.AlignConfig(0.1), step=_reference_step(line, 0.1))
    assert not out.converged and "degenerate" in out.reason and out.iterations == 1 and np.array_equal(out.pose[:, :3], np.eye(3))
    with pytest.raises(TypeError):
        X.icp("index", b, {"radius": 0.1})
    with pytest.raises(ValueError, match="pose"):
        X.icp("index", b, cfg, init=np.eye(3))


# ------------------------------------------------------------------------------------------------ the C entry points
def test_align_entry_points_are_declared_bound_and_exported():
    from point_sam_amd.build import SOURCES, build_library
    build_library()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pointsam_hip.h")).read()
    declared = set(re.findall(r"\b(psam_align_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(ALIGN_ENTRY_POINTS) == {n for n in _lib.SIGNATURES if n.startswith("psam_align_")}
    for n in ALIGN_ENTRY_POINTS:
        assert hasattr(lib, n), n
    assert "pose between two clouds" in hdr and re.search(r"#define PSAM_ALIGN_SUMS 20\b", hdr)
    assert dict(SOURCES)["align.hip"] == dict(SOURCES)["transfer.hip"] == ["-ffp-contract=off", "-fno-slp-vectorize"]
    csrc = os.path.join(ROOT, "point_sam_amd", "csrc")
    src = open(os.path.join(csrc, "align.hip")).read()
    assert "atomic" not in src.replace("no atomics", "") and "order of every fp64 addition is a function of M" in src
    # one copy of the index's layout, of the cell and of the candidate walk: both translation units take them from the shared header
    shared = open(os.path.join(csrc, "transfer_index.h")).read()
    for name in ("struct TransferWs", "TransferWs transfer_layout(", "bool transfer_cell(", "void transfer_candidates("):
        assert name in shared, name
        for f in ("transfer.hip", "align.hip"):
            text = open(os.path.join(csrc, f)).read()
            assert name not in text and '#include "transfer_index.h"' in text, (f, name)


def test_align_entry_points_reject_bad_arguments_on_the_host():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 15) & ~15               # a non-null, aligned pointer; never dereferenced by the device: every call below is refused
    org = (ctypes.c_float * 3)(-1.0, -1.0, -1.0)
    bad_org = (ctypes.c_float * 3)(-1.0, float("nan"), -1.0)
    bad_pose = (ctypes.c_float * 12)(*([0.0] * 11 + [float("inf")]))

    def refused(status, code, text):      # the whole text, as the entry worded it before its checks moved into the shared headers
        assert status == code, (status, lib.psam_last_error_string())
        assert lib.psam_last_error_string() == b"psam_align_step: " + text, lib.psam_last_error_string()
    aligned = b"index_ws must be 16-byte aligned, sums, ws and qry_bits 8-byte aligned, src, qry and nearest 4-byte aligned"

    size = lib.psam_align_workspace_bytes
    assert size(1) == size(64) == 160 and size(65) == 320 and size(6007) == 94 * 160 and size(1 << 28) == (1 << 22) * 160
    assert size(0) == 0 and size(-1) == 0 and size((1 << 28) + 1) == 0
    N, M, big = 1000, 100, 1 << 20
    good = dict(src=p, N=N, index_ws=p, index_ws_bytes=big, origin=ctypes.addressof(org), inv_h=4.0, r2=0.0625, qry=p, M=M, qry_bits=None, pose=None,
                nearest=None, sums=p, ws=p, ws_bytes=big)
    call = lambda **kw: lib.psam_align_step(*{**good, **kw}.values(), None)
    for name in ("src", "index_ws", "origin", "qry", "sums", "ws"):
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
    for name in ("src", "qry", "nearest"):
        refused(call(**{name: p + 2}), -2, aligned)
    refused(call(index_ws_bytes=lib.psam_transfer_index_workspace_bytes(N) - 1), -3, b"index workspace too small (psam_transfer_index_workspace_bytes)")
    refused(call(ws_bytes=size(M) - 1), -3, b"workspace too small (psam_align_workspace_bytes)")


# ------------------------------------------------------------------------------------------------ ops
def test_align_step_refuses_bad_arguments_before_the_library_is_touched(monkeypatch):
    from point_sam_amd import ops

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_library)
    index = ops.TransferIndex(torch.zeros(8, dtype=torch.int64), torch.zeros(10, 3), f32(0.25), f32(4), f32(0.0625), (-1.0, -1.0, -1.0))
    xyz = torch.zeros(100, 3)
    with pytest.raises(TypeError, match="TransferIndex"):
        ops.align_step("index", xyz)
    with pytest.raises(TypeError):
        ops.align_step(index, xyz.double())
    with pytest.raises(ValueError):
        ops.align_step(index, torch.zeros(100, 2))
    for radius in (0.26, 1.0):
        with pytest.raises(ValueError, match="exceeds"):
            ops.align_step(index, xyz, radius=radius)
    for radius in (0, -0.1, float("nan"), "r", True):
        with pytest.raises(ValueError, match="radius"):
            ops.align_step(index, xyz, radius=radius)
    for pose in (np.eye(3), np.diag([1.0, 1, 1, 2]), np.full((3, 4), np.nan), "pose"):
        with pytest.raises(ValueError, match="pose"):
            ops.align_step(index, xyz, pose)
    for bits in (torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int64), [0, 0]):
        with pytest.raises(ValueError, match="bits"):
            ops.align_step(index, xyz, bits=bits)
    # good arguments on the CPU get as far as the device check, still without the library
    with pytest.raises(_lib.PointSamHipError, match="GPU"):
        ops.align_step(index, xyz, np.eye(4), 0.25, torch.zeros(2, dtype=torch.int64))


class _State:
    def __init__(self, n, batch=1):
        self.coords = torch.zeros(batch, n, 3)


def test_predictor_align_refuses_what_transfer_masks_refuses():
    from point_sam_amd import transfer as S
    from point_sam_amd.predictor import PointSAMPredictor
    pred = PointSAMPredictor(None)
    snap = S.Snapshot(torch.zeros(5, 3), torch.zeros(2, 5), 2)
    cfg = X.AlignConfig(0.1)
    with pytest.raises(TypeError, match="Snapshot"):
        pred.align("snap", cfg)
    with pytest.raises(TypeError, match="AlignConfig"):
        pred.align(snap, {"radius": 0.1})
    with pytest.raises(RuntimeError, match="set_scene"):
        pred.align(snap, cfg)
    pred._state = _State(5)
    pred.crop = object()
    with pytest.raises(RuntimeError, match="crop"):
        pred.align(snap, cfg)


# ------------------------------------------------------------------------------------------------ the demo route
class FakeAligner:
    """tests/test_transfer_cpu.py's stand-in predictor plus align: it answers with a fixed Alignment and logs what it was given."""
    POSE = np.array([[1.0, 0.0, 0.0, 0.125], [0.0, 1.0, 0.0, -0.25], [0.0, 0.0, 1.0, 0.5]])

    def __init__(self):
        self.log = []

    def set_pointcloud(self, xyz, rgb):
        self.xyz = xyz

    def predict_masks(self, pts, labels, prompt_mask, multimask):
        logit = 0.5 - (self.xyz[0] - pts[0][-1]).norm(dim=-1)
        return logit[None, None], torch.tensor([[0.9]]), logit[None, None]

    def snapshot(self, logits):
        return ("snap", logits.clone())

    def align(self, snap, cfg, init=None, mask=None):
        self.log.append(("align", snap[0], cfg, init, mask))
        return X.Alignment(self.POSE.copy(), 41, 0.82, 0.0125, 7, True, "fixed point", [(41, 0.0125, cfg.radius)] * 7)

    def propagate(self, snap, radius, pose=None):
        from point_sam_amd.transfer import Propagated
        self.log.append(("propagate", radius, pose))
        K = snap[1].shape[0]
        return Propagated(snap[1].clone(), torch.full((K,), 0.75), torch.zeros(K, dtype=torch.bool), torch.ones(K, dtype=torch.int64), 1.0,
                          torch.zeros(K, 1, 3), torch.ones(K, 1, dtype=torch.bool))


def test_propagate_route_with_and_without_align(tmp_path):
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
    pred = FakeAligner()
    sess = DemoSession(pred, models_dir=str(tmp_path), output_dir=str(tmp_path / "results"), device="cpu")
    srv = serve(sess, "127.0.0.1", 0)
    threading.Thread(target=srv.serve_forever, daemon=True).start()

    def req(method, path, body=None):
        c = http.client.HTTPConnection("127.0.0.1", srv.server_address[1], timeout=10)
        c.request(method, path, None if body is None else json.dumps(body), {"Content-Type": "application/json"})
        r = c.getresponse()
        return r.status, json.loads(r.read())

    def first_scan_with_a_mask():
        sess.masks.clear()                                 # a /propagate keeps its objects: every round starts from the one mask
        _, out = req("GET", "/pointcloud/scan0.ply")
        assert req("POST", "/segment", {"prompt_point": out["xyz"][9:12], "prompt_label": 1})[0] == 200

    try:
        body = {"pointcloud": "scan1.ply", "radius": 0.1}
        given = [[1, 0, 0, 0.01], [0, 1, 0, 0], [0, 0, 1, 0]]
        # without "align": the fields and the calls of before
        first_scan_with_a_mask()
        st, plain = req("POST", "/propagate", dict(body, pose=given))
        assert st == 200 and set(plain) == {"xyz", "rgb", "objects", "lost", "scores"}
        assert [c[0] for c in pred.log] == ["propagate"] and pred.log[-1] == ("propagate", 0.1, given)
        # a bad align field is this request's 400 and leaves the previous state, before anything is loaded
        first_scan_with_a_mask()
        for bad in ({"radius": -1}, {"shrink": 0.5}, {"radius": 0.1, "speed": 3}, 0.1, {"radius": 0.1, "iterations": 0}):
            st, out = req("POST", "/propagate", dict(body, align=bad))
            assert st == 400 and "error" in out and sess.obj_path == "scan0.ply" and len(pred.log) == 1, bad
        # with "align": the given pose (or the identity) is refined first, the refined one is used and returned with the statistics
        for pose in (given, None):
            first_scan_with_a_mask()
            pred.log.clear()
            request = dict(body, align={"radius": 0.2, "final_radius": 0.05, "shrink": 0.5})
            st, out = req("POST", "/propagate", request if pose is None else dict(request, pose=pose))
            assert st == 200, out
            kind, snap, cfg, init, mask = pred.log[0]
            assert kind == "align" and snap == "snap" and cfg == X.AlignConfig(0.2, 0.05, 0.5) and init == pose and mask is None
            assert pred.log[1] == ("propagate", 0.1, FakeAligner.POSE.tolist()) and len(pred.log) == 2
            assert out["pose"] == FakeAligner.POSE.tolist()
            assert out["align"] == {"pairs": 41, "coverage": 0.82, "rms": 0.0125, "iterations": 7, "converged": True}
            assert {k: out[k] for k in plain} == plain and set(out) == set(plain) | {"pose", "align"}      # the other fields are those of a request without
    finally:
        srv.shutdown()
