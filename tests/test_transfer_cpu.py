"""Masks carried to the next scan, the part that needs no GPU: the numpy reference against a brute-force radius search on the inputs the GPU tests use, the
C entry points' declarations and refusals, every ValueError of ops.transfer_index / transfer_plan / transfer.py / the predictor raised before any device
work, and the demo's /propagate route against a stand-in predictor."""
import ctypes
import http.client
import json
import os
import re
import threading

import numpy as np
import pytest
import torch

import transfer_reference as T
from point_sam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRANSFER_ENTRY_POINTS = ("psam_transfer_index_workspace_bytes", "psam_transfer_index_build", "psam_transfer_plan")


def _same(a, b):
    return all(np.array_equal(x[0], y[0]) and np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32)) for x, y in zip(a, b))


def _counts(cands):
    return np.array([len(c[0]) for c in cands])


# ------------------------------------------------------------------------------------------------ the reference and its inputs
def test_lattice_case_grid_equals_brute_force():
    """A condition on the input, not a tolerance: on the lattice the 27-cell candidates ARE the radius search, indices and q alike; and the input
    is not degenerate: empty queries, full triples, exact hits and distance ties all occur."""
    src, qry, r = T.lattice_case()
    assert src.shape == (901, 3) and qry.shape == (1543, 3)
    assert len(np.unique(src, axis=0)) < len(src)                                   # exact duplicates
    grid, brute = T.candidates_grid(src, r, qry), T.candidates_brute(src, r, qry)
    assert _same(grid, brute)
    n = _counts(grid)
    assert 0.4 < (n == 0).mean() < 0.75 and (n >= 3).mean() > 0.25
    assert np.mean([len(q) > 0 and q[0] == 0 for _, q in grid]) > 0.08              # exact hits: the 200 copied queries
    assert sum(len(q) > 1 and q[0] == q[1] for _, q in grid) >= 100                 # q0 == q1: the order falls to the index


@pytest.mark.parametrize("r", [0.05, 0.11])
def test_uniform_case_grid_equals_brute_force(r):
    src, qry = T.uniform_case()
    assert src.shape == (20000, 3) and qry.shape == (6007, 3)
    grid = T.candidates_grid(src, r, qry)
    assert _same(grid, T.candidates_brute(src, r, qry))
    n = _counts(grid)
    if r == 0.05:
        for k in range(3):
            assert (n == k).mean() >= 0.05, k                                       # each of 0, 1, 2, 3 candidates in >= 5 % of the queries
        assert (n >= 3).mean() >= 0.05
    else:
        assert (n >= 3).mean() >= 0.75


def test_reference_plan_rules():
    src = np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0], [0, 0, 0.5], [5, 5, 5]], dtype=np.float32)
    qry = np.array([[0, 0, 0], [0.25, 0, 0], [5, 5, 5.5], [9, 9, 9], [np.nan, 0, 0]], dtype=np.float32)
    idx3, w3 = T.plan(src, 1.0, qry)
    assert idx3[0].tolist() == [0, -1, -1] and w3[0].tolist() == [1, 0, 0]          # exact hit: a copy
    assert idx3[1].tolist()[:2] == [0, 1] and idx3[1, 2] == 2 and abs(w3[1].sum() - 1) < 1e-6 and w3[1, 0] == w3[1, 1]      # (q, j): the tie to the lower index
    assert idx3[2].tolist() == [4, -1, -1] and w3[2].tolist() == [1, 0, 0]          # a lone candidate: a copy
    assert idx3[3].tolist() == [-1, -1, -1] and w3[3].tolist() == [0, 0, 0] and idx3[4].tolist() == [-1, -1, -1]


# ------------------------------------------------------------------------------------------------ the C entry points
def test_transfer_entry_points_are_declared_bound_and_exported():
    from point_sam_amd.build import SOURCES, build_library
    build_library()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pointsam_hip.h")).read()
    declared = set(re.findall(r"\b(psam_transfer_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(TRANSFER_ENTRY_POINTS) == {n for n in _lib.SIGNATURES if n.startswith("psam_transfer_")}
    for n in TRANSFER_ENTRY_POINTS:
        assert hasattr(lib, n), n
    flags = dict(SOURCES)["transfer.hip"]
    assert "-ffp-contract=off" in flags
    assert "27-cell set IS the definition" in hdr
    src = open(os.path.join(ROOT, "point_sam_amd", "csrc", "transfer.hip")).read()
    assert "27-cell set IS the definition" in src and '#include "voxel_table.h"' in src and '#include "interp_select.h"' in src
    # one copy of the selection: scene_interp.hip and transfer.hip share interp_select.h
    for f in ("scene_interp.hip", "transfer.hip"):
        assert "void interp_insert(" not in open(os.path.join(ROOT, "point_sam_amd", "csrc", f)).read(), f


def test_transfer_entry_points_reject_bad_arguments_on_the_host():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 15) & ~15               # a non-null, aligned pointer; never dereferenced by the device: every call below is refused
    org = (ctypes.c_float * 3)(-1.0, -1.0, -1.0)
    bad_org = (ctypes.c_float * 3)(-1.0, float("nan"), -1.0)
    o, bo = ctypes.addressof(org), ctypes.addressof(bad_org)
    pose = (ctypes.c_float * 12)(*([0.0] * 11 + [float("inf")]))

    entry = [b"psam_transfer_index_build: "]

    def refused(status, code, text):      # the whole text, as the entry worded it before its checks moved into the shared header
        assert status == code, (status, lib.psam_last_error_string())
        assert lib.psam_last_error_string() == entry[0] + text, lib.psam_last_error_string()
    small = b"workspace too small (psam_transfer_index_workspace_bytes)"

    size = lib.psam_transfer_index_workspace_bytes
    assert size(131072) == (1 << 18) * 12 + 131072 * 4                               # 2^18 slots of a key and a head, one link per source
    assert size(1000) == 2048 * 12 + 4000 and size(1) == 64 * 12 + 16
    assert size(0) == 0 and size(-1) == 0 and size((1 << 28) + 1) == 0
    N, big = 1000, 1 << 20
    build = lambda *a: lib.psam_transfer_index_build(*a, None)
    refused(build(None, N, o, 4.0, p, big), -1, b"null pointer")
    refused(build(p, N, None, 4.0, p, big), -1, b"null pointer")
    refused(build(p, N, o, 4.0, None, big), -1, b"null pointer")
    refused(build(p, 0, o, 4.0, p, big), -1, b"need 0 < N <= 2^28")
    refused(build(p, (1 << 28) + 1, o, 4.0, p, big), -1, b"need 0 < N <= 2^28")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        refused(build(p, N, o, bad, p, big), -1, b"inv_h must be finite and positive")
    refused(build(p, N, bo, 4.0, p, big), -1, b"origin must be finite")
    refused(build(p, N, o, 4.0, p, size(N) - 1), -3, small)
    refused(build(p, N, o, 4.0, p + 8, big), -2, b"workspace must be 16-byte aligned, src 4-byte aligned")
    refused(build(p + 2, N, o, 4.0, p, big), -2, b"workspace must be 16-byte aligned, src 4-byte aligned")

    plan = lambda *a: lib.psam_transfer_plan(*a, None)
    entry[0] = b"psam_transfer_plan: "
    good = dict(src=p, N=N, ws=p, ws_bytes=big, origin=o, inv_h=4.0, r2=0.0625, qry=p, M=10, pose=None, eps=1e-8, idx3=p, w3=p)
    call = lambda **kw: plan(*{**good, **kw}.values())
    for name in ("src", "ws", "origin", "qry", "idx3", "w3"):
        refused(call(**{name: None}), -1, b"null pointer")
    for name, word in (("N", b"need 0 < N <= 2^28"), ("M", b"need 0 < M <= 2^28")):
        for bad in (0, -5, (1 << 28) + 1):
            refused(call(**{name: bad}), -1, word)
    for name in ("inv_h", "r2", "eps"):
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            refused(call(**{name: bad}), -1, name.encode() + b" must be finite and positive")
    refused(call(origin=bo), -1, b"origin must be finite")
    refused(call(pose=ctypes.addressof(pose)), -1, b"pose must be finite")
    refused(call(ws_bytes=size(N) - 1), -3, small)
    refused(call(ws=p + 8), -2, b"workspace must be 16-byte aligned")
    for name in ("src", "qry", "idx3", "w3"):
        refused(call(**{name: p + 2}), -2, b"src, qry, idx3 and w3 must be 4-byte aligned")


# ------------------------------------------------------------------------------------------------ the Python host
def test_radius_and_pose_arguments():
    from point_sam_amd import ops
    r, inv_h, r2 = ops.transfer_radius(0.1)
    assert (r, inv_h, r2) == (np.float32(0.1), np.float32(1) / np.float32(0.1), np.float32(np.float32(0.1) * np.float32(0.1)))
    assert all(isinstance(v, np.float32) for v in (r, inv_h, r2))
    for bad in (0, -1.0, float("inf"), float("nan"), 1e-30, 1e30, 1e-46, True, "1", None):      # 1e-30: the square underflows; 1e30: it overflows
        with pytest.raises(ValueError):
            ops.transfer_radius(bad)
    assert ops.transfer_pose(None) is None
    P3 = np.array(T.POSE, dtype=np.float64)
    P4 = np.concatenate([P3, [[0, 0, 0, 1]]], 0)
    a, b = ops.transfer_pose(P3), ops.transfer_pose(P4)
    assert a.dtype == np.float32 and a.shape == (12,) and np.array_equal(a, b) and np.array_equal(a, T.POSE.reshape(12))
    assert np.array_equal(ops.transfer_pose(P4.tolist()), a) and np.array_equal(ops.transfer_pose(torch.from_numpy(P3)), a)
    bad4 = P4.copy(); bad4[3, 3] = 2
    bad_nan = P3.copy(); bad_nan[1, 2] = np.nan
    bad_big = P3.copy(); bad_big[0, 3] = 1e300                                      # finite in fp64, infinite in fp32
    for bad in (bad4, bad_nan, bad_big, np.eye(3), np.zeros(12), "pose", [[1, 2], [3]]):
        with pytest.raises(ValueError):
            ops.transfer_pose(bad)


def test_transfer_index_and_plan_refuse_bad_arguments_before_any_device_work():
    from point_sam_amd import ops
    src = torch.rand(100, 3)
    for bad in (0.0, float("nan"), 1e-30, -2):
        with pytest.raises(ValueError):
            ops.transfer_index(src, bad)
    for bad_value in (float("nan"), float("inf"), -float("inf")):
        s = src.clone(); s[17, 1] = bad_value
        with pytest.raises(ValueError, match="finite"):
            ops.transfer_index(s, 0.1)
    wide = src.clone(); wide[0, 2] = 3.0e5
    with pytest.raises(ValueError, match="2\\^21"):
        ops.transfer_index(wide, 0.1)                                                # 3e6 cells on z
    for bad in (torch.rand(100, 2), torch.rand(0, 3), torch.rand(2, 100, 3)):
        with pytest.raises(ValueError):
            ops.transfer_index(bad, 0.1)
    with pytest.raises(TypeError):
        ops.transfer_index(src.double(), 0.1)
    with pytest.raises(_lib.PointSamHipError):                                       # every check passed: the HIP path has no CPU fallback
        ops.transfer_index(src, 0.1)
    index = ops.TransferIndex(torch.zeros(8, dtype=torch.int64), src, *ops.transfer_radius(0.1), (-1.0, -1.0, -1.0))
    assert index.num_source == 100
    bad4 = np.eye(4); bad4[3, 0] = 1
    with pytest.raises(ValueError, match="last row"):
        ops.transfer_plan(index, src, pose=bad4)
    with pytest.raises(ValueError, match="finite"):
        ops.transfer_plan(index, src, pose=np.full((3, 4), np.nan))
    for bad in (0, -1e-8, float("inf"), float("nan"), True):
        with pytest.raises(ValueError, match="eps"):
            ops.transfer_plan(index, src, eps=bad)
    with pytest.raises(ValueError):
        ops.transfer_plan(index, torch.rand(5, 4))
    with pytest.raises(TypeError):
        ops.transfer_plan("index", src)
    with pytest.raises(_lib.PointSamHipError):
        ops.transfer_plan(index, src)


def test_transfer_module_checks_and_thin_calls(monkeypatch):
    from point_sam_amd import ops, transfer as X
    plan = X.TransferPlan(torch.tensor([[0, 1, -1], [-1, -1, -1], [2, -1, -1]], dtype=torch.int32), torch.zeros(3, 3), 5)
    assert X.covered(plan).tolist() == [True, False, True]
    calls = []
    monkeypatch.setattr(ops, "scene_interp_rows", lambda rows, idx3, w3, fill=None: calls.append(("rows", rows, idx3, w3, fill)) or "R")
    monkeypatch.setattr(ops, "scene_interp_bits", lambda rows, idx3, w3, thr=0.0: calls.append(("bits", rows, idx3, w3, thr)) or ("B", "A"))
    rows = torch.zeros(2, 5)
    assert X.transfer_rows(plan, rows, -3.0) == "R" and X.transfer_bits(plan, rows, 0.5) == ("B", "A")
    assert calls[0][0] == "rows" and calls[0][1] is rows and calls[0][2] is plan.idx3 and calls[0][3] is plan.w3 and calls[0][4] == -3.0
    assert calls[1][0] == "bits" and calls[1][1] is rows and calls[1][4] == 0.5
    for fn in (X.transfer_rows, X.transfer_bits):
        with pytest.raises(ValueError):
            fn(plan, torch.zeros(2, 6))                                             # not the source cloud's width
        with pytest.raises(TypeError):
            fn((plan.idx3, plan.w3), rows)
    assert len(calls) == 2
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError):
            X.check_propagate_arguments(bad, None)
    for bad in ("x", float("nan"), True):
        with pytest.raises(ValueError):
            X.check_propagate_arguments(1, bad)
    X.check_propagate_arguments(2, -7.5)
    with pytest.raises(ValueError):
        X.check_threshold(float("nan"), "transfer_masks")
    snap = X.Snapshot(torch.zeros(5, 3), torch.zeros(2, 5), 2)
    assert X.check_snapshot(snap, "propagate") is snap
    with pytest.raises(ValueError):
        X.check_snapshot(X.Snapshot(torch.zeros(5, 3), torch.zeros(2, 4), 2), "propagate")
    with pytest.raises(TypeError):
        X.check_snapshot((snap.coords, snap.logits), "propagate")


class _State:
    def __init__(self, n, batch=1):
        self.coords = torch.zeros(batch, n, 3)


def test_predictor_refuses_before_a_cloud_under_a_crop_and_bad_arguments():
    from point_sam_amd import transfer as X
    from point_sam_amd.predictor import PointSAMPredictor
    pred = PointSAMPredictor(None)
    snap = X.Snapshot(torch.zeros(5, 3), torch.zeros(2, 5), 2)
    for call in (lambda: pred.snapshot(torch.zeros(2, 5)), lambda: pred.transfer_masks(snap, 0.1), lambda: pred.propagate(snap, 0.1)):
        with pytest.raises(RuntimeError, match="set_scene"):
            call()
    pred._state = _State(5)
    pred.crop = object()
    for call in (lambda: pred.snapshot(torch.zeros(2, 5)), lambda: pred.transfer_masks(snap, 0.1), lambda: pred.propagate(snap, 0.1)):
        with pytest.raises(RuntimeError, match="crop"):
            call()
    pred.crop = None
    with pytest.raises(ValueError, match="width"):
        pred.snapshot(torch.zeros(2, 6))
    with pytest.raises(ValueError):
        pred.snapshot(torch.zeros(5))
    with pytest.raises(TypeError):
        pred.snapshot(torch.zeros(2, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match="clicks"):
        pred.propagate(snap, 0.1, clicks=0)
    with pytest.raises(ValueError, match="fill"):
        pred.propagate(snap, 0.1, fill="low")
    with pytest.raises(ValueError, match="threshold"):
        pred.transfer_masks(snap, 0.1, threshold=float("nan"))
    with pytest.raises(TypeError):
        pred.propagate("snap", 0.1)
    pred._state = _State(5, batch=2)
    with pytest.raises(ValueError, match="one cloud"):
        pred.snapshot(torch.zeros(2, 5))
    # the radius and the pose are refused by ops.transfer_index / transfer_plan before the device is touched
    pred._state = _State(5)
    pred.model = type("M", (), {"device": torch.device("cpu")})()
    with pytest.raises(ValueError, match="radius"):
        pred.propagate(snap, -1.0)
    with pytest.raises(ValueError, match="radius"):
        pred.transfer_masks(snap, float("nan"))


# ------------------------------------------------------------------------------------------------ the demo route
class FakePropagator:
    """set_pointcloud / predict_masks as tests/test_demo_server_cpu.py's stand-in; snapshot keeps the logits and the cloud, propagate answers with the
    snapshot's rows shifted by one point, the last object lost."""

    def __init__(self):
        self.log = []

    def set_pointcloud(self, xyz, rgb):
        self.xyz = xyz

    def predict_masks(self, pts, labels, prompt_mask, multimask):
        logit = 0.5 - (self.xyz[0] - pts[0][-1]).norm(dim=-1)
        return logit[None, None], torch.tensor([[0.9]]), logit[None, None]

    def snapshot(self, logits):
        self.log.append(("snapshot", logits.clone(), self.xyz.clone()))
        return ("snap", logits.clone())

    def propagate(self, snap, radius, pose=None):
        from point_sam_amd.transfer import Propagated
        self.log.append(("propagate", radius, pose, self.xyz.clone()))
        logits = torch.roll(snap[1], 1, dims=1)
        K = logits.shape[0]
        lost = torch.zeros(K, dtype=torch.bool); lost[-1] = True
        logits[-1] = float("-inf")
        scores = torch.full((K,), 0.75); scores[-1] = float("nan")
        return Propagated(logits, scores, lost, torch.ones(K, dtype=torch.int64), 1.0, torch.zeros(K, 1, 3), torch.ones(K, 1, dtype=torch.bool))


def _write_ply(path, pts):
    with open(path, "w") as f:
        f.write(f"ply\nformat ascii 1.0\nelement vertex {len(pts)}\nproperty float x\nproperty float y\nproperty float z\n"
                "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
        for p in pts:
            f.write(f"{p[0]} {p[1]} {p[2]} 255 0 128\n")


def _req(port, method, path, body=None):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=10)
    c.request(method, path, None if body is None else json.dumps(body), {"Content-Type": "application/json"})
    r = c.getresponse()
    return r.status, json.loads(r.read())


def test_propagate_route_against_a_stand_in_predictor(tmp_path):
    from point_sam_amd.demo_server import DemoSession, serve
    pts = np.random.RandomState(0).rand(50, 3) * 4 + 1
    nxt = pts[::-1] + 0.25                                                           # the next scan: other points, shifted
    _write_ply(tmp_path / "scan0.ply", pts)
    _write_ply(tmp_path / "scan1.ply", nxt)
    pred = FakePropagator()
    sess = DemoSession(pred, models_dir=str(tmp_path), output_dir=str(tmp_path / "results"), device="cpu")
    srv = serve(sess, "127.0.0.1", 0)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    try:
        port = srv.server_address[1]
        body = {"pointcloud": "scan1.ply", "radius": 0.1}
        st, out = _req(port, "POST", "/propagate", body)
        assert st == 400 and "point cloud" in out["error"]
        st, out = _req(port, "GET", "/pointcloud/scan0.ply")
        xyz = np.array(out["xyz"]).reshape(-1, 3)
        st, out = _req(port, "POST", "/propagate", body)
        assert st == 400 and "before any /segment" in out["error"]                   # like /next
        _, seg0 = _req(port, "POST", "/segment", {"prompt_point": xyz[3].tolist(), "prompt_label": 1})
        assert _req(port, "POST", "/next")[0] == 200
        _, seg1 = _req(port, "POST", "/segment", {"prompt_point": xyz[20].tolist(), "prompt_label": 1})
        for bad in ({"radius": 0.1}, {"pointcloud": "scan1.ply"}, dict(body, radius=0), dict(body, radius="r"), dict(body, extra=1), dict(body, pointcloud=7),
                    dict(body, pose=[[1, 0, 0], [0, 1, 0]]), dict(body, pose=np.diag([1.0, 1, 1, 2]).tolist()), dict(body, pointcloud="missing.ply")):
            st, out = _req(port, "POST", "/propagate", bad)
            assert st in (400, 404) and "error" in out, bad
            assert sess.obj_path == "scan0.ply" and len(sess.masks) == 1 and sess.segment_mask is not None      # the previous state
        before = sess.pc_xyz.clone()
        pose = [[1, 0, 0, 0.01], [0, 1, 0, 0], [0, 0, 1, 0]]
        st, out = _req(port, "POST", "/propagate", dict(body, pose=pose))
        assert st == 200, out
        # the kept mask and the current one, as +-1 logits of the cloud they belong to
        kind, logits, cloud = pred.log[-2]                                              # (an earlier snapshot belongs to the refused missing.ply)
        assert kind == "snapshot" and torch.equal(cloud, before)
        want = np.stack([np.array(seg0["seg"]), np.array(seg1["seg"])])
        assert np.array_equal(logits.numpy(), np.where(want, 1.0, -1.0).astype(np.float32))
        # the new cloud in the previous cloud's normalisation
        shift = pts.mean(0)
        scale = np.linalg.norm(pts - shift, axis=-1).max()
        assert np.allclose(np.array(out["xyz"]).reshape(-1, 3), (nxt - shift) / scale)
        kind, radius, got_pose, cloud = pred.log[-1]
        assert [c[0] for c in pred.log].count("propagate") == 1
        assert kind == "propagate" and radius == 0.1 and got_pose == pose and np.allclose(cloud[0].numpy(), (nxt - shift) / scale, atol=1e-6)
        assert sess.obj_path == "scan1.ply"
        # /segment's format per object, plus lost
        assert [o["seg"] for o in out["objects"]] == [np.roll(want[0], 1).tolist(), [False] * 50]
        assert out["lost"] == [False, True] and out["scores"] == [0.75, None]
        assert len(sess.masks) == 2 and sess.segment_mask is None and sess.prompts == []
    finally:
        srv.shutdown()
