"""Scan map relocalisation without a GPU: the two forms of the numpy reference (tests/track_score_reference.py) against each other and against
track_reference.step on every case of the step, the header / binding sync of the psam_relocalize_* entries and their refusals before any launch, the
wrappers' refusals, ScanMap.anchors' plain-torch core against the numpy reference, the demo's "search" beside "track" against a stand-in predictor,
and the recorded constants of the search fixture."""
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
import align_search_reference as ASR
import scanmap_reference as SM
import track_reference as TR
import track_score_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("psam_relocalize_workspace_bytes", "psam_relocalize_score")
POSES7 = R.seven_poses()


# ------------------------------------------------------------------------------------------------ the reference
def _arguments(case):
    radius = case.get("radius", case["h"])
    return radius, case.get("reach") or TR.reach_of(radius, case["h"])


@pytest.mark.parametrize("case", TR.cases() + [TR.lattice_case()], ids=lambda c: c["name"])
def test_the_two_forms_of_the_score_agree_and_equal_the_steps_pairs(case):
    ref = TR.build(case)
    radius, reach = _arguments(case)
    more = dict(V=case.get("V"), skip=case.get("skip"), min_count=case.get("min_count", 1))
    fast = R.score(ref, case["qry"], POSES7, radius, reach, **more)
    assert fast.dtype == np.int64 and fast.shape == (7,)
    assert np.array_equal(fast, R.score(ref, case["qry"], POSES7, radius, reach, definition=True, **more))
    pairs = [TR.step(ref, case["qry"], radius, p, None, more["V"], more["skip"], more["min_count"], reach)[1][0] for p in POSES7]
    assert fast.tolist() == pairs and fast[3] == 0, "the count of a pose is the step's word [0] under it; a translation of 3e6 leaves the map"


def test_the_seven_poses_are_rigid_and_distinct():
    assert POSES7.shape == (7, 3, 4) and np.array_equal(POSES7[0], np.eye(4)[:3]) and np.array_equal(POSES7[1], AR.TRUE_POSE)
    for p in POSES7:
        assert np.abs(p[:, :3] @ p[:, :3].T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(p[:, :3]) - 1) < 1e-12
    assert abs(AR.pose_error(POSES7[2], POSES7[0])[0] - np.pi) < 1e-12 and POSES7[3][0, 3] == 3e6
    assert len({p.tobytes() for p in POSES7}) == 7


def test_hand_cases_of_the_score():
    by = {c["name"]: c for c in TR.cases()}
    one = POSES7[:1]
    case = by["skip hands on"]
    ref = TR.build(case)
    assert R.score(ref, case["qry"], one, case["radius"], skip=case["skip"])[0] == 1 and R.score(ref, case["qry"], one, case["radius"])[0] == 2
    assert R.score(ref, case["qry"], one, case["radius"], skip=[True, True, True])[0] == 0
    case = by["tie and q == r2"]
    ref = TR.build(case)
    assert R.score(ref, case["qry"], one, case["h"])[0] == 6, "q == r2 counts, an ulp further does not"
    assert R.score(ref, case["qry"], one, case["h"], r2=np.nextafter(TR.r2_of(case["h"]), np.float32(0)))[0] == 0
    case = by["min_count 2"]
    ref = TR.build(case)
    assert R.score(ref, case["qry"], one, case["radius"], min_count=2)[0] < R.score(ref, case["qry"], one, case["radius"])[0]


# ------------------------------------------------------------------------------------------------ the C ABI
def _ctype(decl: str):
    from point_sam_amd import _lib
    decl = decl.strip()
    if "*" in decl or decl.startswith("psam_stream_t"):
        return _lib.ptr
    return {"float": _lib.f32, "int32_t": _lib.i32, "size_t": _lib.size_t}[decl.split()[-2] if len(decl.split()) > 1 else decl]


def test_header_and_binding_declare_the_same_relocalize_entries():
    from point_sam_amd import _lib, ops
    from point_sam_amd.build import SOURCES, build_library
    hdr = open(os.path.join(ROOT, "include", "pointsam_hip.h")).read()
    declared = set(re.findall(r"\b(psam_relocalize_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(ENTRY_POINTS) == {n for n in _lib.SIGNATURES if n.startswith("psam_relocalize_")}
    for n in ENTRY_POINTS:
        ret, params = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % n, hdr).groups()
        assert _lib.SIGNATURES[n] == (_lib.size_t if n.endswith("_bytes") else _lib.i32, [_ctype(p) for p in params.split(",")]), n
        assert ret == ("size_t" if n.endswith("_bytes") else "int32_t")
    assert "scan map relocalisation */" in hdr
    assert int(re.search(r"#define PSAM_RELOCALIZE_POSES (\d+)", hdr).group(1)) == ops.TRACK_SCORE_POSES
    assert dict(SOURCES)["track_score.hip"] == dict(SOURCES)["track.hip"] == ["-ffp-contract=off", "-fno-slp-vectorize"]
    build_library()
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in ENTRY_POINTS)
    text = open(os.path.join(ROOT, "point_sam_amd", "csrc", "track_score.hip")).read()
    assert "map_mean(" in text and "map_point<true>(" in text and "pose_apply(" in text and "asm" not in text, "the shared arithmetic, no inline assembly"


def test_sizes_and_refusals_of_the_c_entry_before_any_launch():
    """Nothing is launched: every call is a size query or is refused by the argument checks.  The pointers are addresses inside a host buffer."""
    from point_sam_amd import _lib
    from point_sam_amd.build import build_library
    build_library()
    lib = _lib.load()
    for V in (1, 63, 4096, 1 << 28):
        assert lib.psam_relocalize_workspace_bytes(V) == 16 * V
    for bad in (0, -1, (1 << 28) + 1):
        assert lib.psam_relocalize_workspace_bytes(bad) == 0
    host = ctypes.create_string_buffer(1 << 18)
    p = (ctypes.addressof(host) + 15) & ~15
    mv, mp, M, P, V = 64, 128, 100, 9, 8
    nbytes, ws_bytes = lib.psam_map_bytes(mv, mp), lib.psam_relocalize_workspace_bytes(V)
    assert nbytes < (1 << 16)
    counts, ws, q, poses = p + (1 << 17), p + (1 << 17) + 256, p + (1 << 16), p + (1 << 16) + 4096
    err = lambda: lib.psam_last_error_string().decode()
    good = dict(map=p, map_bytes=nbytes, mv=mv, mp=mp, V=V, skip=None, min_count=1, reach=1, r2=0.01, qry=q, M=M, poses=poses, P=P, counts=counts, ws=ws,
                ws_bytes=ws_bytes)

    def call(**change):
        a = dict(good, **change)
        return lib.psam_relocalize_score(a["map"], a["map_bytes"], a["mv"], a["mp"], a["V"], a["skip"], a["min_count"], a["reach"], a["r2"], a["qry"], a["M"],
                                         a["poses"], a["P"], a["counts"], a["ws"], a["ws_bytes"], None)
    for change in (dict(map=None), dict(qry=None), dict(poses=None), dict(counts=None), dict(ws=None), dict(M=0), dict(M=-1), dict(M=(1 << 28) + 1), dict(V=0),
                   dict(V=mv + 1), dict(mv=0), dict(mp=0), dict(mv=(1 << 28) + 1), dict(reach=0), dict(reach=5), dict(reach=-1), dict(min_count=0),
                   dict(min_count=-3), dict(r2=0.0), dict(r2=-1.0), dict(r2=float("nan")), dict(r2=float("inf")), dict(P=0), dict(P=-1), dict(P=(1 << 20) + 1)):
        assert call(**change) == -1 and err().startswith("psam_relocalize_score"), change
    assert call(P=0) == -1 and "2^20" in err()
    for change in (dict(map=p + 8), dict(ws=ws + 8), dict(skip=p + 4), dict(qry=q + 2), dict(poses=poses + 1), dict(counts=counts + 2)):
        assert call(**change) == -2 and err().startswith("psam_relocalize_score") and "aligned" in err(), change
    assert call(map_bytes=nbytes - 1) == -3 and err().startswith("psam_relocalize_score") and "map block too small" in err()
    assert call(ws_bytes=ws_bytes - 1) == -3 and "workspace too small (psam_relocalize_workspace_bytes)" in err()
    assert call(ws_bytes=0) == -3


# ------------------------------------------------------------------------------------------------ the wrappers
def _host_map(voxel_size=0.125, max_voxels=64, V=0):
    """tests/test_track_cpu.py's: a ScanMap put together by hand over a host block; every call made on it here is refused before it reaches the block."""
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
    from point_sam_amd.align import AlignConfig, PlaneConfig, SearchConfig
    from point_sam_amd.predictor import PointSAMPredictor
    from point_sam_amd.scanmap import MapOverflow
    xyz = torch.zeros(100, 3)
    one = np.eye(4)[None, :3]
    m = _host_map(V=8)
    block, mv, mp = m._block, m.max_voxels, m.max_pairs
    score = lambda *a, **k: ops.track_score(block, mv, mp, 8, *a, voxel_size=0.125, **k)
    with pytest.raises(TypeError):
        score("x", one)
    with pytest.raises(TypeError):
        score(xyz.double(), one)
    for bad in (torch.zeros(0, 3), torch.zeros(10, 2)):
        with pytest.raises(ValueError):
            score(bad, one)
    for poses in (np.eye(4)[:3], np.zeros((0, 3, 4)), np.full((2, 3, 4), np.nan), "x", np.zeros((2, 12)), torch.zeros(2, 12),
                  np.stack([np.eye(4), np.diag([1.0, 1.0, 1.0, 2.0])])):
        with pytest.raises(ValueError):
            score(xyz, poses)
    for radius in (0.0, -1.0, float("nan"), "r", 0.51):
        with pytest.raises(ValueError):
            score(xyz, one, radius)
    for skip in (torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), [0]):
        with pytest.raises(ValueError, match="skip"):
            score(xyz, one, skip=skip)
    for n in (0, -1, 1.0, True, 2 ** 31):
        with pytest.raises(ValueError, match="min_count"):
            score(xyz, one, min_count=n)
    for V in (0, 65, 2.0, True):
        with pytest.raises(ValueError):
            ops.track_score(block, mv, mp, V, xyz, one, voxel_size=0.125)
    with pytest.raises(TypeError):
        ops.track_score("x", mv, mp, 8, xyz, one, voxel_size=0.125)
    with pytest.raises(ValueError):
        ops.track_score(block, mv, mp, 8, xyz, one, voxel_size=0.0)
    with pytest.raises(PointSamHipError):                          # everything in order, but nothing lives on the GPU: no CPU fallback, no launch
        score(xyz, one, 0.125, torch.zeros(1, dtype=torch.int64))
    # ScanMap.track_score, relocalize and anchors
    with pytest.raises(ValueError, match="empty"):
        _host_map().track_score(xyz, one)
    with pytest.raises(ValueError, match="empty"):
        _host_map().anchors()
    dead = _host_map(V=8)
    dead._flags = 1
    cfg = AlignConfig(radius=0.25, final_radius=0.125, shrink=0.8)
    for call in (lambda: dead.track_score(xyz, one), lambda: dead.anchors(), lambda: dead.relocalize(xyz, cfg, SearchConfig())):
        with pytest.raises(MapOverflow):
            call()
    with pytest.raises(TypeError, match="search"):
        m.relocalize(xyz, cfg, {"yaw_steps": 4})
    with pytest.raises(TypeError, match="search"):
        m.relocalize(xyz, cfg, np.eye(4)[:3])                      # a pose is track()'s start: relocalize takes a SearchConfig in its place
    with pytest.raises(TypeError, match="AlignConfig"):
        m.relocalize(xyz, {"radius": 0.25}, SearchConfig())
    with pytest.raises(ValueError, match="exceeds"):
        m.relocalize(xyz, cfg, SearchConfig(radius=0.3))
    with pytest.raises(ValueError, match="at most 4"):
        m.relocalize(xyz, AlignConfig(radius=0.5), SearchConfig(radius=0.51))
    with pytest.raises(ValueError, match="at most 4"):
        m.relocalize(xyz, AlignConfig(radius=0.51), SearchConfig())
    with pytest.raises(TypeError, match="occupied"):
        m.relocalize(xyz, cfg, SearchConfig(), occupied="x")
    with pytest.raises(ValueError, match="needs normals"):
        m.relocalize(xyz, cfg, SearchConfig(), plane=PlaneConfig())
    with pytest.raises(ValueError, match="empty"):
        _host_map().relocalize(xyz, cfg, SearchConfig())
    for bad in (dict(cells=0), dict(cells=True), dict(cells=1.5), dict(min_voxels=0), dict(min_count=0), dict(occupied="x")):
        with pytest.raises((ValueError, TypeError)):
            m.anchors(**bad)
    pred = PointSAMPredictor(model=None)
    with pytest.raises(TypeError, match="search"):
        pred.map_relocalize(m, cfg, np.eye(4)[:3])
    with pytest.raises(TypeError):
        pred.map_relocalize("not a map", cfg, SearchConfig())
    with pytest.raises(RuntimeError):
        pred.map_relocalize(m, cfg, SearchConfig())                # no cloud was set


# ------------------------------------------------------------------------------------------------ anchors
def test_anchors_core_equals_the_reference():
    from point_sam_amd.scanmap import anchors_from_voxels
    g = np.random.default_rng(23)
    pts = g.uniform(-0.9, 0.9, size=(900, 3)).astype(np.float32)
    # two coarse cells (cells = 4 at h = 2^-4: coarse cells of size 0.25) filled by hand: one with exactly min_voxels = 5 voxels, one with 4
    fine = lambda c, k: ((np.asarray(c) * 4 + np.array([k % 4, k // 4, 0]) + 0.5) / 16.0 - 1.0)
    exact, short = (1, 1, 1), (6, 1, 1)
    hand = np.array([fine(exact, k) for k in range(5)] + [fine(short, k) for k in range(4)], dtype=np.float32)
    coarse_of = lambda p: tuple(np.floor((p + 1.0) * 16.0).astype(int) // 4)
    pts = pts[[coarse_of(p) not in (exact, short) for p in pts]]
    ref = SM.RefMap(2.0 ** -4, 4096)
    ref.add(np.concatenate([pts[:400], hand]), np.zeros((400 + len(hand), 3), dtype=np.float32))
    ref.add(pts[300:], np.zeros((len(pts) - 300, 3), dtype=np.float32))
    keys, means = np.asarray(ref.keys, dtype=np.int64), TR.means(ref)
    assert ref.V > 600 and max(ref.count) > 1
    tk, tm = torch.from_numpy(keys), torch.from_numpy(means)
    occupied = g.uniform(size=ref.V) < 0.8
    occupied[[ref.locate(hand[k:k + 1])[0] for k in range(len(hand))]] = True
    for cells, min_voxels, min_count, occ in ((4, 5, 1, None), (4, 5, 1, occupied), (4, 6, 1, None), (8, 8, 1, None), (1, 1, 2, occupied), (2, 3, 1, None),
                                              (1 << 21, 1, 1, None)):
        ok = R.pairable(ref, occ, min_count)
        want = R.anchors(keys, means, ok, cells, min_voxels)
        got = anchors_from_voxels(tk, tm, torch.from_numpy(ok), cells, min_voxels)
        assert got.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want), (cells, min_voxels)
        assert len(want) >= 1
    five = R.anchors(keys, means, R.pairable(ref), 4, 5)
    centre = lambda c, n: np.mean([fine(c, k) for k in range(n)], 0)
    has = lambda rows, c: bool((np.abs(rows - c).max(1) < 1e-6).any())
    assert has(five, centre(exact, 5)) and not has(five, centre(short, 4)), "exactly min_voxels voxels give an anchor, one fewer gives none"
    assert has(R.anchors(keys, means, R.pairable(ref), 4, 4), centre(short, 4))
    assert len(R.anchors(keys, means, R.pairable(ref), 1 << 21, 1)) == 1
    order = [tuple(np.floor((a + 1.0) * 16.0).astype(int) // 4)[::-1] for a in R.anchors(keys, means, R.pairable(ref), 4, 1)]
    assert order == sorted(order) and len(set(order)) == len(order), "ordered by coarse (cz, cy, cx)"
    assert anchors_from_voxels(tk, tm, torch.zeros(ref.V, dtype=torch.bool)).shape == (0, 3)
    from point_sam_amd.align import SearchConfig
    assert np.array_equal(SearchConfig(anchors=five).anchors, five), "the result goes straight into a SearchConfig"


# ------------------------------------------------------------------------------------------------ the demo's route
class _RefScanMap:
    def __init__(self, voxel_size, max_voxels):
        self.ref = SM.RefMap(voxel_size, max_voxels)

    num_voxels = property(lambda self: self.ref.V)
    num_adds = property(lambda self: self.ref.adds)


def _reference_search(ref, xyz, cfg, search):
    """The numpy search under a SearchConfig's yaw grid -> (the winner's icp dict, the record's fields)."""
    picked = np.asarray(ASR.sample_positions(len(xyz), search.sample))
    poses = ASR.candidates(ASR.yaw_grid(search.yaw_steps), R.search_centroid(ref), xyz[picked].astype(np.float64).mean(0), search.offsets, search.offset_step)
    counts = R.score(ref, xyz[picked], poses, cfg.radius if search.radius is None else search.radius)
    order = ASR.ordered(counts, search.keep)
    runs = [TR.icp(ref, xyz, cfg.radius, cfg.final_radius, cfg.shrink, cfg.iterations, cfg.min_pairs, poses[p]) for p in order]
    chosen = ASR.choose(runs)
    return runs[chosen], dict(poses=len(poses), sample=len(picked), chosen=chosen, candidates=[
        dict(pose_index=p, count=int(counts[p]), pairs=r["pairs"], rms=r["rms"], converged=r["converged"]) for p, r in zip(order, runs)])


class FakeRelocaliser:
    """A stand-in predictor that answers from the references: map_add takes (m, labels, pose), map_align (m, cfg, init), map_relocalize (m, cfg, search)."""

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
        self.calls.append(("align", cfg, init, None))
        return self._alignment(TR.icp(m.ref, self.xyz[0].numpy(), cfg.radius, cfg.final_radius, cfg.shrink, cfg.iterations, cfg.min_pairs, init), None)

    def map_relocalize(self, m, cfg, search):
        from point_sam_amd.align import SearchRecord
        self.calls.append(("relocalize", cfg, None, search))
        out, fields = _reference_search(m.ref, self.xyz[0].numpy(), cfg, search)
        return self._alignment(out, SearchRecord(fields["poses"], fields["sample"], fields["candidates"], fields["chosen"]))

    @staticmethod
    def _alignment(out, record):
        from point_sam_amd.align import Alignment
        return Alignment(out["pose"], out["pairs"], out["coverage"], out["rms"], out["iterations"], out["converged"],
                         "fixed point" if out["converged"] else "iterations", out["history"], record)


def _req(port, path, body=None):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=120)
    c.request("POST", path, None if body is None else json.dumps(body), {"Content-Type": "application/json"})
    r = c.getresponse()
    return r.status, json.loads(r.read())


def _upload(port, xyz, rgb):
    st, _ = _req(port, "/sampled_pointcloud", {"points": {str(i): float(v) for i, v in enumerate(xyz.flatten())},
                                               "colors": {str(i): float(v) for i, v in enumerate(rgb.flatten())}})
    assert st == 200


def test_map_add_route_searches_before_it_tracks_and_adds():
    from point_sam_amd.align import AlignConfig, SearchConfig
    from point_sam_amd.demo_server import DemoSession, serve
    pred = FakeRelocaliser()
    h = 0.125
    srv = serve(DemoSession(pred, device="cpu", map_voxel_size=h, map_max_voxels=4096), "127.0.0.1", 0)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    try:
        port = srv.server_address[1]
        a = AR.surfaces(600, 21).astype(np.float32)
        truth = np.concatenate([AR.rotation([0, 0, 1], 90.0), np.array([[0.02], [-0.01], [0.015]])], 1)
        b_in_a = AR.surfaces(500, 22)
        b = ((b_in_a - truth[:, 3]) @ truth[:, :3]).astype(np.float32)
        track = {"radius": 2 * h, "final_radius": h, "shrink": 0.8, "iterations": 40}
        search = {"yaw_steps": 4, "sample": 128, "keep": 2}
        keys = {"new_voxels", "accepted", "rejected", "num_voxels", "num_adds"}
        tracked = keys | {"pose", "pairs", "coverage", "rms", "converged", "reason"}
        _upload(port, a, np.zeros_like(a))
        # the map is empty: nothing to search in, the scan is added as given and the answer is the empty track's
        st, out = _req(port, "/map/add", {"track": track, "search": search})
        assert st == 200 and set(out) == tracked and out["pose"] == np.eye(4)[:3].tolist() and out["pairs"] == 0 and "empty" in out["reason"]
        assert [c[0] for c in pred.calls] == ["add"] and pred.calls[0][1] is None
        ref = SM.RefMap(h, 4096)
        ref.add(a, np.zeros_like(a))
        # the second scan, a quarter turn away: searched, refined, then added under the pose found
        _upload(port, b, np.zeros_like(b))
        st, out = _req(port, "/map/add", {"track": track, "search": search})
        want, record = _reference_search(ref, b, AlignConfig(**track), SearchConfig(**search))
        assert st == 200 and [c[0] for c in pred.calls[1:]] == ["relocalize", "add"] and set(out) == tracked | {"search"}
        assert pred.calls[1][2] is None and isinstance(pred.calls[1][3], SearchConfig) and pred.calls[1][3].yaw_steps == 4 and pred.calls[1][1].radius == 2 * h
        assert out["pose"] == want["pose"].tolist() == pred.calls[2][1] and out["pairs"] == want["pairs"] > 400 and out["rms"] == want["rms"]
        assert out["search"] == json.loads(json.dumps(record)) and out["search"]["poses"] == 4 and out["search"]["sample"] == 128
        assert len(out["search"]["candidates"]) == 2 and set(out["search"]["candidates"][0]) == {"pose_index", "count", "pairs", "rms", "converged"}
        rot, tr = AR.pose_error(np.asarray(out["pose"]), truth)
        assert rot < 0.05 and tr < 0.02, "the quarter turn was found"
        # "track" alone answers as before, and the stand-in sees no search
        n = len(pred.calls)
        st, out = _req(port, "/map/add", {"pose": want["pose"].tolist(), "track": track})
        assert st == 200 and set(out) == tracked and [c[0] for c in pred.calls[n:]] == ["align", "add"] and pred.calls[n][3] is None
        n = len(pred.calls)
        st, out = _req(port, "/map/add", {})
        assert st == 200 and set(out) == keys and [c[0] for c in pred.calls[n:]] == ["add"]
        # bad fields: a 400, and nothing reaches the predictor
        n = len(pred.calls)
        for bad in ({"search": search}, {"search": search, "pose": np.eye(4)[:3].tolist()}, {"track": track, "search": search, "pose": np.eye(4)[:3].tolist()},
                    {"track": track, "search": "x"}, {"track": track, "search": {"other": 1}}, {"track": track, "search": {"yaw_steps": 0}},
                    {"track": track, "search": {"radius": 3 * h}}, {"track": track, "search": {"radius": -1}}, {"track": track, "search": {"keep": 0}},
                    {"track": {"radius": -1}, "search": search}, {"track": track, "search": search, "more": 1}):
            assert _req(port, "/map/add", bad)[0] == 400, bad
        assert len(pred.calls) == n
    finally:
        srv.shutdown()
        srv.server_close()


# ------------------------------------------------------------------------------------------------ the search fixture
def test_search_fixture_constants():
    """Recomputes every recorded constant of tests/track_score_reference.py; about two minutes of numpy."""
    f = R.search_fixture()
    ref, b, counts = f["ref"], f["b"], f["counts"]
    assert ref.V == R.SEARCH_VOXELS and len(b) == R.SEARCH_QUERIES and len(f["poses"]) == R.SEARCH_POSES and len(f["picked"]) == ASR.SAMPLE
    assert TR.reach_of(ASR.ICP["radius"], R.SEARCH_H) == 4 and TR.reach_of(ASR.SCORE_RADIUS, R.SEARCH_H) == 2
    assert f["order"] == R.SEARCH_ORDER and [int(counts[p]) for p in f["order"]] == R.SEARCH_COUNTS and int(np.median(counts)) == R.SEARCH_MEDIAN
    assert [r["pairs"] for r in f["runs"]] == R.SEARCH_PAIRS and all(r["converged"] for r in f["runs"][:6]) and not any(r["converged"] for r in f["runs"][6:])
    for r in f["runs"][6:]:
        assert 0.09 < AR.pose_error(r["pose"], ASR.YAW_TRUTH)[1] < 0.13, "a false optimum about 0.10 off in translation"
    assert f["chosen"] == R.SEARCH_CHOSEN and f["order"][f["chosen"]] == 738
    assert f["runs"][1]["rms"] < f["runs"][0]["rms"], "chosen by the lower rms among the ties at 4405 pairs"
    rot, tr = AR.pose_error(f["runs"][f["chosen"]]["pose"], ASR.YAW_TRUTH)
    assert abs(rot - R.SEARCH_ROTATION_ERROR) < 1e-7 and abs(tr - R.SEARCH_TRANSLATION_ERROR) < 1e-8
    good = R.refine(ref, b, ASR.YAW_TRUTH)
    rot, tr = AR.pose_error(good["pose"], ASR.YAW_TRUTH)
    assert good["converged"] and good["iterations"] == R.REF_ITERATIONS and good["pairs"] == R.SEARCH_QUERIES and abs(good["rms"] - R.REF_RMS) < 1e-7
    assert abs(rot - R.REF_ROTATION_ERROR) < 1e-7 and abs(tr - R.REF_TRANSLATION_ERROR) < 1e-8
    plain = R.refine(ref, b)
    assert plain["pairs"] == R.IDENTITY_PAIRS and not plain["converged"] and abs(AR.pose_error(plain["pose"], ASR.YAW_TRUTH)[0] - R.IDENTITY_ROTATION_ERROR) < 0.01
