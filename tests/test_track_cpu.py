"""Scan map tracking without a GPU: the two forms of the numpy reference (tests/track_reference.py) against each other on every case of the step, the
seed of the cross-check against align_reference, the recorded constants of the loop fixture, the header / binding sync of the psam_track_* entries and
their refusals before any launch, ops.track_reach, the wrappers' refusals, and the demo's "track" against a stand-in predictor."""
import ctypes
import http.client
import json
import os
import re
import threading

import numpy as np
import pytest
import torch

import align_reference as AR
import scanmap_reference as SM
import track_reference as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("psam_track_workspace_bytes", "psam_track_step")
CROSS_SEED = 0


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("case", TR.cases() + [TR.lattice_case()], ids=lambda c: c["name"])
def test_vectorised_reference_equals_the_definition(case):
    ref = TR.build(case)
    near, sums, mass = TR.reference(case, ref)
    near_d, sums_d, mass_d = TR.reference(case, ref, definition=True)
    assert np.array_equal(near, near_d) and np.array_equal(sums, sums_d) and np.array_equal(mass, mass_d)


def test_hand_cases_of_the_reference():
    by = {c["name"]: c for c in TR.cases()}
    near, sums, _ = TR.reference(by["tie and q == r2"])
    assert near.tolist() == [0, 2, 4, 6, 8, 10, -1], "the lower id wins on either side and along every axis; q == r2 pairs, an ulp further does not"
    assert sums[0] == 6 and sums[19] == 7 and sums[1] == 6 * 2.0 ** -6
    near, sums, _ = TR.reference(by["skip hands on"])
    assert near.tolist() == [-1, 2] and sums[0] == 1 and sums[19] == 2
    near, sums, _ = TR.reference(by["boundary"])
    assert (near[:6] >= 0).all() and (near[6:12] == -1).all() and sums[19] == 8, "exactly +-1 has a cell; an ulp outside, NaN and inf have none"
    a, b, c = (TR.reference(by[f"reach {r}"]) for r in (1, 2, 4))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[1], c[1])
    assert TR.reference(by["min_count 2"])[1][0] < TR.reference(dict(by["min_count 2"], min_count=1))[1][0]
    near = TR.reference(by["V below the map's"])[0]
    assert near.max() < 700 and (TR.reference(dict(by["V below the map's"], V=None))[0] >= 700).any()
    ref = TR.build(by["sizes M=64"])
    assert max(ref.count) > 1, "voxels whose mean is no input point"
    assert TR.build(by["full table"]).V == 32 == by["full table"]["max_voxels"]


def test_cross_check_seed_the_two_references_agree_on_every_query():
    """What the GPU test then asserts of the two kernels: track's nearest == align_step's nearest on the map's cloud, row = voxel id."""
    case = TR.random_case(CROSS_SEED)
    ref, q, r = TR.build(case), case["qry"], case["h"]
    near = TR.step(ref, q, r)[0]
    other = AR.step(TR.means(ref), r, q)[0]
    assert np.array_equal(near, other) and (near >= 0).sum() > 400 and (near < 0).sum() > 50


def test_loop_fixture_constants():
    ref, a, b = TR.loop_case()
    assert ref.V == TR.REF_LOOP_VOXELS and TR.reach_of(TR.LOOP_RADIUS, TR.LOOP_H) == 2 and TR.reach_of(TR.LOOP_FINAL, TR.LOOP_H) == 1
    rot0, tr0 = AR.pose_error(TR.LOOP_INIT)
    assert abs(rot0 - np.deg2rad(0.5)) < 1e-12 and abs(tr0 - TR.LOOP_H / 2) < 1e-12
    out = TR.loop_reference(ref, b)
    assert out["converged"] and out["iterations"] == TR.REF_LOOP_ITERATIONS and out["pairs"] == TR.REF_LOOP_PAIRS == len(b)
    rot, tr = AR.pose_error(out["pose"])
    assert abs(rot - TR.REF_ROTATION_ERROR) < 1e-7 and abs(tr - TR.REF_TRANSLATION_ERROR) < 1e-7
    assert rot < rot0 and tr < tr0 / 10


# ------------------------------------------------------------------------------------------------ the C ABI
def _ctype(decl: str):
    from point_sam_amd import _lib
    decl = decl.strip()
    if "*" in decl or decl.startswith("psam_stream_t"):
        return _lib.ptr
    return {"float": _lib.f32, "int32_t": _lib.i32, "size_t": _lib.size_t}[decl.split()[-2] if len(decl.split()) > 1 else decl]


def test_header_and_binding_declare_the_same_track_entries():
    from point_sam_amd import _lib, ops
    from point_sam_amd.build import SOURCES
    hdr = open(os.path.join(ROOT, "include", "pointsam_hip.h")).read()
    declared = set(re.findall(r"\b(psam_track_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(ENTRY_POINTS) == {n for n in _lib.SIGNATURES if n.startswith("psam_track_")}
    for n in ENTRY_POINTS:
        ret, params = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % n, hdr).groups()
        assert _lib.SIGNATURES[n] == (_lib.size_t if n.endswith("_bytes") else _lib.i32, [_ctype(p) for p in params.split(",")]), n
        assert ret == ("size_t" if n.endswith("_bytes") else "int32_t")
    assert "scan map tracking */" in hdr
    assert int(re.search(r"#define PSAM_TRACK_MAX_REACH (\d+)", hdr).group(1)) == ops.TRACK_MAX_REACH == 4
    assert dict(SOURCES)["track.hip"] == ["-ffp-contract=off", "-fno-slp-vectorize"]
    scanmap = open(os.path.join(ROOT, "point_sam_amd", "csrc", "scanmap.hip")).read()
    block = open(os.path.join(ROOT, "point_sam_amd", "csrc", "map_block.h")).read()
    assert "float map_mean(" in block and "float map_mean(" not in scanmap, "one copy of the voxel mean"


def test_sizes_and_refusals_of_the_c_entry_before_any_launch():
    """Nothing is launched: every call is a size query or is refused by the argument checks.  The pointers are addresses inside a host buffer."""
    from point_sam_amd import _lib
    from point_sam_amd.build import build_library
    build_library()
    lib = _lib.load()
    for M in (1, 64, 65, 2113, 1 << 28):
        assert lib.psam_track_workspace_bytes(M) == lib.psam_align_workspace_bytes(M) == (M + 63) // 64 * 20 * 8
    for bad in (0, -1, (1 << 28) + 1):
        assert lib.psam_track_workspace_bytes(bad) == 0
    host = ctypes.create_string_buffer(1 << 18)
    p = (ctypes.addressof(host) + 15) & ~15
    mv, mp, M = 64, 128, 100
    nbytes, ws_bytes = lib.psam_map_bytes(mv, mp), lib.psam_track_workspace_bytes(M)
    sums, ws, q = p + (1 << 17), p + (1 << 17) + 256, p + (1 << 16)
    err = lambda: lib.psam_last_error_string().decode()
    pose = (ctypes.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    good = dict(map=p, map_bytes=nbytes, mv=mv, mp=mp, V=8, skip=None, min_count=1, reach=1, r2=0.01, qry=q, M=M, bits=None, pose=None, nearest=None, sums=sums,
                ws=ws, ws_bytes=ws_bytes)

    def call(**change):
        a = dict(good, **change)
        return lib.psam_track_step(a["map"], a["map_bytes"], a["mv"], a["mp"], a["V"], a["skip"], a["min_count"], a["reach"], a["r2"], a["qry"], a["M"], a["bits"],
                                   a["pose"], a["nearest"], a["sums"], a["ws"], a["ws_bytes"], None)
    for change in (dict(map=None), dict(qry=None), dict(sums=None), dict(ws=None), dict(M=0), dict(M=-1), dict(M=(1 << 28) + 1), dict(V=0), dict(V=mv + 1),
                   dict(mv=0), dict(mp=0), dict(mv=(1 << 28) + 1), dict(reach=0), dict(reach=5), dict(reach=-1), dict(min_count=0), dict(min_count=-3),
                   dict(r2=0.0), dict(r2=-1.0), dict(r2=float("nan")), dict(r2=float("inf"))):
        assert call(**change) == -1 and "psam_track_step" in err(), change
    bad_pose = (ctypes.c_float * 12)(*([1.0] * 11 + [float("nan")]))
    assert call(pose=ctypes.addressof(bad_pose)) == -1 and "pose" in err()
    for change in (dict(map=p + 8), dict(sums=sums + 4), dict(ws=ws + 4), dict(skip=p + 4), dict(bits=p + 4), dict(qry=q + 2), dict(nearest=q + 1)):
        assert call(**change) == -2 and "aligned" in err(), change
    assert call(map_bytes=nbytes - 1) == -3 and "map block too small" in err()
    assert call(ws_bytes=ws_bytes - 1) == -3 and "workspace too small" in err()
    assert call(pose=ctypes.addressof(pose), ws_bytes=0) == -3


# ------------------------------------------------------------------------------------------------ the wrappers
def test_track_reach():
    from point_sam_amd import ops
    above = lambda r: float(np.nextafter(np.float32(r), np.float32(10)))
    for h in (2.0 ** -3, 2.0 ** -4):                               # powers of two: fl32(r) * fl32(1 / h) is exact
        assert ops.track_reach(h, h) == 1 == TR.reach_of(h, h)
        assert ops.track_reach(above(h), h) == 2 == TR.reach_of(above(h), h)
        assert ops.track_reach(h / 2, h) == 1
        assert ops.track_reach(4 * h, h) == 4 == ops.TRACK_MAX_REACH
        with pytest.raises(ValueError, match="at most 4"):
            ops.track_reach(above(4 * h), h)
        with pytest.raises(ValueError):
            ops.track_reach(5 * h, h)
    for h in (0.1, 0.3, 0.07):                                     # elsewhere the product of the two fp32 values decides, as the definition says
        for r in (h, 2 * h, 3.3 * h):
            want = max(1, int(np.ceil(np.float64(np.float32(r)) * np.float64(np.float32(1) / np.float32(h)))))
            assert ops.track_reach(r, h) == want == TR.reach_of(r, h) and want in (1, 2, 3, 4)
    for bad in (0, -1.0, float("nan"), float("inf"), "x", None, True):
        with pytest.raises(ValueError):
            ops.track_reach(bad, 0.125)
        with pytest.raises(ValueError):
            ops.track_reach(0.125, bad)


def _host_map(voxel_size=0.125, max_voxels=64, V=0):
    """tests/test_carve_cpu.py's: a ScanMap put together by hand over a host block; every call made on it here is refused before it reaches the block."""
    from point_sam_amd import ops
    from point_sam_amd.scanmap import ScanMap
    m = ScanMap.__new__(ScanMap)
    m.voxel_size, (m.max_voxels, m.max_pairs) = voxel_size, ops.map_capacities(max_voxels)
    m._block = torch.zeros(ops.map_bytes(m.max_voxels, m.max_pairs) // 8 + 2, dtype=torch.int64)
    m._adds = m._flags = m._carves = 0
    m._V, m._carve = V, None
    return m


def test_wrappers_refuse_bad_arguments_before_device_work():
    from point_sam_amd import ops
    from point_sam_amd._lib import PointSamHipError
    from point_sam_amd.align import AlignConfig
    from point_sam_amd.scanmap import MapOverflow
    xyz = torch.zeros(100, 3)
    cfg = AlignConfig(radius=0.25, final_radius=0.125, shrink=0.8)
    m = _host_map(V=8)
    with pytest.raises(TypeError, match="AlignConfig"):
        m.track(xyz, {"radius": 0.25})
    with pytest.raises(ValueError, match="at most 4"):
        m.track(xyz, AlignConfig(radius=0.51))
    for bad in ("x", 1, [True] * 8):
        with pytest.raises(TypeError, match="occupied"):
            m.track(xyz, cfg, occupied=bad)
    for bad in (torch.ones(7, dtype=torch.bool), torch.ones(8, dtype=torch.int32), torch.ones(1, 8, dtype=torch.bool)):
        with pytest.raises(ValueError, match="occupied"):
            m.track(xyz, cfg, occupied=bad)
    with pytest.raises(ValueError, match="empty"):
        _host_map().track(xyz, cfg)
    with pytest.raises(ValueError, match="empty"):
        _host_map().track_step(xyz)
    dead = _host_map(V=8)
    dead._flags = 1
    for call in (lambda: dead.track(xyz, cfg), lambda: dead.track_step(xyz)):
        with pytest.raises(MapOverflow):
            call()
    # the step's own checks: map_add's for the cloud, the pose and the block, align_step's for the bits
    block, mv, mp = m._block, m.max_voxels, m.max_pairs
    step = lambda *a, **k: ops.track_step(block, mv, mp, 8, *a, voxel_size=0.125, **k)
    with pytest.raises(TypeError):
        step("x")
    with pytest.raises(TypeError):
        step(xyz.double())
    for bad in (torch.zeros(0, 3), torch.zeros(10, 2)):
        with pytest.raises(ValueError):
            step(bad)
    for pose in (np.eye(3), np.full((3, 4), np.nan), "x"):
        with pytest.raises(ValueError):
            step(xyz, pose)
    for radius in (0.0, -1.0, float("nan"), "r", 0.51):
        with pytest.raises(ValueError):
            step(xyz, None, radius)
    for bits in (torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int64), "x"):
        with pytest.raises(ValueError, match="bits"):
            step(xyz, bits=bits)
    for skip in (torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), [0]):
        with pytest.raises(ValueError, match="skip"):
            step(xyz, skip=skip)
    for n in (0, -1, 1.0, True, 2 ** 31):
        with pytest.raises(ValueError, match="min_count"):
            step(xyz, min_count=n)
    for V in (0, 65, 2.0, True):
        with pytest.raises(ValueError):
            ops.track_step(block, mv, mp, V, xyz, voxel_size=0.125)
    with pytest.raises(TypeError):
        ops.track_step("x", mv, mp, 8, xyz, voxel_size=0.125)
    with pytest.raises(ValueError):
        ops.track_step(block, 4096, 8192, 8, xyz, voxel_size=0.125)             # the block is too short for that map
    with pytest.raises(ValueError):
        ops.track_step(block, mv, mp, 8, xyz, voxel_size=0.0)
    # everything in order, but the block lives on the CPU: the project's "no CPU fallback" error, before any launch
    with pytest.raises(PointSamHipError):
        step(xyz, None, 0.125, torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int64))


def test_predictor_entries_refuse_before_any_cloud():
    from point_sam_amd.align import AlignConfig
    from point_sam_amd.predictor import PointSAMPredictor
    pred = PointSAMPredictor(model=None)
    with pytest.raises(TypeError):
        pred.map_align("not a map", AlignConfig(radius=0.1))
    with pytest.raises(TypeError):
        pred.map_nearest("not a map")
    with pytest.raises(RuntimeError):
        pred.map_align(_host_map(V=8), AlignConfig(radius=0.1))


# ------------------------------------------------------------------------------------------------ the demo's route
class _RefScanMap:
    def __init__(self, voxel_size, max_voxels):
        self.ref = SM.RefMap(voxel_size, max_voxels)

    num_voxels = property(lambda self: self.ref.V)
    num_adds = property(lambda self: self.ref.adds)


class FakeTracker:
    """A stand-in predictor that answers from the references: map_add takes (m, labels, pose), map_align (m, cfg, init)."""

    def __init__(self):
        self.calls = []

    def set_pointcloud(self, xyz, rgb):
        self.xyz, self.rgb = xyz, rgb

    def new_map(self, voxel_size, max_voxels):
        return _RefScanMap(voxel_size, max_voxels)

    def map_add(self, m, labels=None, pose=None):
        from point_sam_amd.scanmap import AddResult
        self.calls.append(("add", None if pose is None else np.asarray(pose, dtype=np.float64).tolist()))
        ids, new, acc, rej = m.ref.add(self.xyz[0].numpy(), self.rgb[0].numpy(), None if labels is None else labels.numpy(), pose)
        return AddResult(torch.from_numpy(ids), new, acc, rej)

    def map_align(self, m, cfg, init=None):
        from point_sam_amd.align import Alignment
        self.calls.append(("align", cfg, init))
        out = TR.icp(m.ref, self.xyz[0].numpy(), cfg.radius, cfg.final_radius, cfg.shrink, cfg.iterations, cfg.min_pairs, init)
        return Alignment(out["pose"], out["pairs"], out["coverage"], out["rms"], out["iterations"], out["converged"],
                         "fixed point" if out["converged"] else "iterations", out["history"])


def _req(port, path, body=None):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
    c.request("POST", path, None if body is None else json.dumps(body), {"Content-Type": "application/json"})
    r = c.getresponse()
    return r.status, json.loads(r.read())


def _upload(port, xyz, rgb):
    st, _ = _req(port, "/sampled_pointcloud", {"points": {str(i): float(v) for i, v in enumerate(xyz.flatten())},
                                               "colors": {str(i): float(v) for i, v in enumerate(rgb.flatten())}})
    assert st == 200


def test_map_add_route_tracks_before_it_adds():
    from point_sam_amd.demo_server import DemoSession, serve
    pred = FakeTracker()
    h = 0.125
    srv = serve(DemoSession(pred, device="cpu", map_voxel_size=h, map_max_voxels=4096), "127.0.0.1", 0)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    try:
        port = srv.server_address[1]
        a = AR.surfaces(600, 21).astype(np.float32)
        shift = np.array([[1, 0, 0, 0.02], [0, 1, 0, -0.01], [0, 0, 1, 0.015]], dtype=np.float64)
        b = (AR.surfaces(500, 22) - shift[:, 3]).astype(np.float32)
        track = {"radius": 2 * h, "final_radius": h, "shrink": 0.8, "iterations": 40}
        keys = {"new_voxels", "accepted", "rejected", "num_voxels", "num_adds"}
        _upload(port, a, np.zeros_like(a))
        # the map is empty: nothing to track against, the scan is added under the pose as given
        st, out = _req(port, "/map/add", {"track": track})
        assert st == 200 and set(out) == keys | {"pose", "pairs", "coverage", "rms", "converged", "reason"}
        assert out["pose"] == np.eye(4)[:3].tolist() and out["pairs"] == 0 and out["converged"] is False and out["rms"] is None and "empty" in out["reason"]
        assert [c[0] for c in pred.calls] == ["add"] and pred.calls[0][1] is None
        ref = SM.RefMap(h, 4096)
        ref.add(a, np.zeros_like(a))
        # the second scan: refined from the request's pose, then added under the refined one
        _upload(port, b, np.zeros_like(b))
        guess = np.concatenate([np.eye(3), np.array([[0.0], [0.0], [0.0]])], 1)
        st, out = _req(port, "/map/add", {"pose": guess.tolist(), "track": track})
        want = TR.icp(ref, b, 2 * h, h, 0.8, 40, init=guess)
        assert st == 200 and [c[0] for c in pred.calls[1:]] == ["align", "add"]
        assert pred.calls[1][2] == guess.tolist() and pred.calls[1][1].radius == 2 * h and pred.calls[1][1].iterations == 40
        assert out["pose"] == want["pose"].tolist() == pred.calls[2][1] and out["pairs"] == want["pairs"] > 400 and out["coverage"] == want["coverage"]
        assert out["rms"] == want["rms"] and out["converged"] == want["converged"] and isinstance(out["reason"], str) and out["num_adds"] == 2
        assert np.linalg.norm(np.asarray(out["pose"])[:, 3] - shift[:, 3]) < 0.01
        # without "track": the five keys of before, and no align
        n = len(pred.calls)
        st, out = _req(port, "/map/add", {})
        assert st == 200 and set(out) == keys and [c[0] for c in pred.calls[n:]] == ["add"]
        # bad fields: a 400, and nothing reaches the predictor
        n = len(pred.calls)
        for bad in ({"track": {}}, {"track": "x"}, {"track": {"radius": -1}}, {"track": {"radius": "r"}}, {"track": {"radius": h, "other": 1}},
                    {"track": {"radius": h, "shrink": 2}}, {"track": {"radius": h, "iterations": 0}}, {"track": {"radius": 4.5 * h}},
                    {"track": {"radius": h, "final_radius": 2 * h}}, {"track": track, "pose": [[1, 0, 0]]}):
            assert _req(port, "/map/add", bad)[0] == 400, bad
        assert len(pred.calls) == n
    finally:
        srv.shutdown()
        srv.server_close()
