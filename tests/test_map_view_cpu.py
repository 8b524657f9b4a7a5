"""Scan map views without a GPU: the truncated integer walk of the reference (tests/map_view_reference.py) against the exact-rational definition of a
ray's cells, the fp32 recipe of a pixel's direction, hand cases of the reference view, the header / binding sync of the psam_mapview entries and
their refusals before any launch, the wrappers' refusals, and the demo's /map/view against a stand-in predictor."""
import base64
import ctypes
import http.client
import itertools
import json
import os
import re
import threading

import numpy as np
import pytest
import torch

import carve_reference as CR
import map_view_reference as R
import scanmap_reference as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("psam_mapview_ws_bytes", "psam_mapview")
F = np.float32


# ------------------------------------------------------------------------------------------------ the walk
@pytest.mark.parametrize("o", [(2, 2, 2), (0, 0, 0), (4, 1, 3)])
def test_truncated_walk_is_the_geometric_ray_cut_at_the_grid(o):
    """Every direction with |N_a| <= 4 in a 5^3 grid: the cells visited before the walk leaves the grid are the cells of the exact-rational segment
    from o to o + N that lie in the grid, in the order of carve_reference's own walks."""
    cmax, checked = 4, 0
    for N in itertools.product(range(-4, 5), repeat=3):
        if N == (0, 0, 0):
            continue
        e = tuple(o[a] + N[a] for a in range(3))
        inside = lambda c: min(c) >= 0 and max(c) <= cmax
        got = R.truncated(o, N, cmax)
        assert set(got) == {c for c in CR.geometric(o, e) if inside(c)} and len(set(got)) == len(got), (o, N)
        full = CR.walk_by_differences(o, e)
        assert full == CR.walk(o, e) == list(R.walk_cells(o, N))
        cut = next((i for i, c in enumerate(full) if not inside(c)), len(full))
        assert got == full[:cut], "the grid and the segment are convex: the walk never returns"
        assert all(inside(c) for c in got) and len(got) <= 3 * (cmax + 1)
        checked += 1
    assert checked == 9 ** 3 - 1


def test_walk_towards_a_far_cell_is_lazy_and_leaves_the_grid_within_the_bound():
    for N, o, cmax in (((1 << 21, 0, 0), (3, 4, 5), 16), ((-(1 << 21), 1 << 21, 0), (7, 7, 7), 16), ((1 << 21, 12345, -(1 << 21)), (0, 2047, 2048), 2048),
                       ((0, 0, -(1 << 21)), (5, 5, 0), 64)):
        got = R.truncated(o, N, cmax)
        assert len(got) <= 3 * (cmax + 1) and all(0 <= v <= cmax for c in got for v in c)
    assert R.truncated((3, 4, 5), (1 << 21, 0, 0), 16) == [(x, 4, 5) for x in range(4, 17)]
    assert R.truncated((7, 7, 7), (-(1 << 21), 1 << 21, 0), 16) == [(7 - k, 7 + k, 7) for k in range(1, 8)], "tied axes step together"
    assert R.truncated((5, 5, 0), (0, 0, -(1 << 21)), 64) == []


# ------------------------------------------------------------------------------------------------ the direction
def _random_camera(g, width=7, height=5):
    from point_sam_amd.views import Camera
    q = g.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    eye = g.uniform(-0.8, 0.8, size=3)
    return Camera(np.concatenate([Rm, (-Rm @ eye)[:, None]], 1), g.uniform(3, 40), g.uniform(3, 40), g.uniform(0, width), g.uniform(0, height), width, height), eye


def test_the_longest_axis_of_a_direction_is_exactly_two_to_the_21():
    g = np.random.default_rng(5)
    cams = [_random_camera(g)[0] for _ in range(40)]
    cams += [R.axis_camera((0.1, 0.2, 0.3), 9, 7, 8.0, 4.5, 3.5), R.diagonal_camera((0.1, 0.2, 0.3), 9, 7, 8.0, 4.5, 3.5)]
    for cam in cams:
        N, ok = R.directions(cam)
        assert ok.all() and N.shape == (cam.height, cam.width, 3)
        assert (np.abs(N).max(-1) == 1 << 21).all() and (np.abs(N) <= 1 << 21).all()
    N, _ = R.directions(cams[-2])
    assert N[3, 4].tolist() == [0, 0, 1 << 21], "axis-aligned, cx = px + 0.5: two axes never move"
    N, _ = R.directions(cams[-1])
    assert N[3, 4].tolist() == [1 << 21, 1 << 21, 0], "two equal words in the third rotation row: a walk of tied steps"


def test_eye_and_cell_of_the_wrapper_are_the_references():
    from point_sam_amd import ops
    g = np.random.default_rng(6)
    for h in (0.125, 2.0 ** -7, 0.03):
        for _ in range(20):
            cam, eye = _random_camera(g)
            got, cell = ops.map_view_eye(cam, h)
            assert got.dtype == np.float32 and np.array_equal(got, R.eye_of(cam.pose_words)) and np.abs(got - eye).max() < 1e-6
            assert cell == R.eye_cell(got, SM.inv_h_of(h)) and all(0 <= c <= R.cmax_of(SM.inv_h_of(h)) for c in cell)
    assert R.cmax_of(SM.inv_h_of(0.125)) == 16 and R.cmax_of(SM.inv_h_of(2.0 ** -10)) == 2048 and R.cmax_of(SM.inv_h_of(2.0 ** -21)) == (1 << 21) - 1
    assert ops.map_view_eye(R.axis_camera((1.0, -1.0, 1.0), 4, 4, 2.0, 2.0, 2.0), 0.125)[1] == (16, 0, 16)


# ------------------------------------------------------------------------------------------------ the reference view, by hand
def _centre(cell, h):
    return (np.asarray(cell, dtype=np.float64) + 0.5) * h - 1.0


def test_hand_cases_of_the_reference_view():
    h = 0.125
    ref = SM.RefMap(h, 64)
    cells = [(8, 8, 12), (8, 8, 14), (8, 8, 8), (8, 8, 9)]          # two on the axis, the eye's own cell, the cell next to the eye
    pts = np.array([_centre(c, h) for c in cells], dtype=F)
    pts[3, 2] = (9 * h - 1.0) + 1e-4                                # just behind the eye's cell: in front of a near of 0.1
    ref.add(pts, np.zeros_like(pts))
    ref.add(pts[1:2], np.zeros((1, 3), dtype=F))                    # voxel 1 has two observations
    cam = R.axis_camera(_centre((8, 8, 8), h), 3, 3, 1.0, 1.5, 1.5, near=0.1)
    keys, visited = R.view(ref, cam)
    depth = R.depths(ref, cam.pose_words)
    assert keys[1, 1] == R.key_of(depth[0], 0) and (np.delete(keys.reshape(-1), 4) == R.EMPTY).all()
    assert visited[(1, 1)] == [(8, 8, z) for z in range(9, 13)], "the eye's own cell is no candidate; the voxel in front of near is passed"
    assert depth[3] < 0.1 <= depth[0] and abs(depth[0] - 4 * h) < 1e-6
    assert visited[(0, 0)][-1][2] == 16 or min(visited[(0, 0)][-1]) == 0, "an empty pixel's ray is walked to the grid's bound"
    assert R.view(ref, cam, skip=np.array([True, False, False, False]))[0][1, 1] == R.key_of(depth[1], 1)
    assert R.view(ref, cam, min_count=2)[0][1, 1] == R.key_of(depth[1], 1)
    assert R.view(ref, cam, V=1)[0][1, 1] == R.key_of(depth[0], 0) and R.view(ref, cam, skip=np.ones(4, dtype=bool))[0][1, 1] == R.EMPTY
    near = R.axis_camera(_centre((8, 8, 8), h), 3, 3, 1.0, 1.5, 1.5, near=1e-3)
    assert R.view(ref, near)[0][1, 1] == R.key_of(depth[3], 3)
    ref.dead = True
    assert (R.view(ref, cam)[0] == R.EMPTY).all()


def test_home_slots_are_the_tables():
    assert R.capacity(1) == 64 and R.capacity(4096) == 8192 and R.capacity(4097) == 16384
    assert R.voxel_hash(0) == 0 and R.voxel_hash(1) == 0xb456bcfc34c2cb2c, "the finaliser of MurmurHash3"
    assert all(0 <= s < 64 for s in R.home_slots(range(100), 8))


# ------------------------------------------------------------------------------------------------ the C ABI
def _ctype(decl: str):
    from point_sam_amd import _lib
    decl = decl.strip()
    if "*" in decl or decl.startswith("psam_stream_t"):
        return _lib.ptr
    return {"float": _lib.f32, "int32_t": _lib.i32, "size_t": _lib.size_t}[decl.split()[-2] if len(decl.split()) > 1 else decl]


def test_header_binding_and_library_declare_the_same_map_view_entries():
    from point_sam_amd import _lib, ops
    from point_sam_amd.build import SOURCES, build_library
    hdr = open(os.path.join(ROOT, "include", "pointsam_hip.h")).read()
    declared = set(re.findall(r"\b(psam_mapview[a-z0-9_]*)\s*\(", hdr))
    assert declared == set(ENTRY_POINTS) == {n for n in _lib.SIGNATURES if n.startswith("psam_mapview")}
    for n in ENTRY_POINTS:
        ret, params = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % n, hdr).groups()
        assert _lib.SIGNATURES[n] == (_lib.size_t if n.endswith("_bytes") else _lib.i32, [_ctype(p) for p in params.split(",")]), n
        assert ret == ("size_t" if n.endswith("_bytes") else "int32_t")
    assert "scan map views */" in hdr
    assert int(re.search(r"#define PSAM_MAP_VIEW_NO_GATE (\d+)", hdr).group(1)) == ops.MAP_VIEW_NO_GATE
    assert int(re.search(r"#define PSAM_MAP_VIEW_NO_LDS (\d+)", hdr).group(1)) == ops.MAP_VIEW_NO_LDS
    assert dict(SOURCES)["map_view.hip"] == dict(SOURCES)["carve.hip"] == ["-ffp-contract=off", "-fno-slp-vectorize"]
    build_library()
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in ENTRY_POINTS)
    text = open(os.path.join(ROOT, "point_sam_amd", "csrc", "map_view.hip")).read()
    assert "map_mean(" in text and "pose_apply(" in text and "voxel_axis(" in text and "voxel_find(" in text and "asm" not in text, \
        "the shared arithmetic, no inline assembly"


def test_sizes_and_refusals_of_the_c_entry_before_any_launch():
    """Nothing is launched: every call is a size query or is refused by the argument checks.  The pointers are addresses inside a host buffer."""
    from point_sam_amd import _lib
    from point_sam_amd.build import build_library
    build_library()
    lib = _lib.load()
    words = lambda nb: -(-(nb ** 3) // 32)
    pad = lambda b: (b + 15) & ~15
    for inv_h, nb in ((8.0, 3), (128.0, 33), (256.0, 65), (1024.0, 257), (4096.0, 257), (1048576.0, 256), (7.9, 2), (0.25, 1)):
        assert lib.psam_mapview_ws_bytes(inv_h) == pad(4 * words(nb)), inv_h
    assert lib.psam_mapview_ws_bytes(2048.0) == pad(4 * words(257)) and lib.psam_mapview_ws_bytes(4000.0) == pad(4 * words(251)), "past 257 bricks per axis a brick grows: 16^3, then 32^3 cells"
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.psam_mapview_ws_bytes(bad) == 0
    host = ctypes.create_string_buffer(1 << 18)
    p = (ctypes.addressof(host) + 15) & ~15
    mv, mp, V, inv_h = 64, 128, 8, 8.0
    nbytes, ws_bytes = lib.psam_map_bytes(mv, mp), lib.psam_mapview_ws_bytes(inv_h)
    assert nbytes < (1 << 16)
    keys, ws, stats = p + (1 << 16), p + (1 << 17), p + (1 << 17) + 4096
    pose = (ctypes.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    eye = (ctypes.c_float * 3)(0, 0, 0)
    err = lambda: lib.psam_last_error_string().decode()
    good = dict(map=p, map_bytes=nbytes, mv=mv, mp=mp, V=V, inv_h=inv_h, pose=ctypes.addressof(pose), fx=8.0, fy=8.0, cx=4.0, cy=4.0, width=8, height=8,
                near=0.01, eye=ctypes.addressof(eye), skip=None, min_count=1, flags=0, keys=keys, stats=None, ws=ws, ws_bytes=ws_bytes)

    def call(**change):
        a = dict(good, **change)
        return lib.psam_mapview(a["map"], a["map_bytes"], a["mv"], a["mp"], a["V"], a["inv_h"], a["pose"], a["fx"], a["fy"], a["cx"], a["cy"], a["width"],
                                 a["height"], a["near"], a["eye"], a["skip"], a["min_count"], a["flags"], a["keys"], a["stats"], a["ws"], a["ws_bytes"], None)
    nan, inf = float("nan"), float("inf")
    bad_pose = (ctypes.c_float * 12)(1, 0, 0, 0, 0, nan, 0, 0, 0, 0, 1, 0)
    far_eye, nan_eye = (ctypes.c_float * 3)(0, 1.5, 0), (ctypes.c_float * 3)(nan, 0, 0)
    for change in (dict(map=None), dict(pose=None), dict(eye=None), dict(keys=None), dict(ws=None), dict(V=0), dict(V=-1), dict(V=mv + 1), dict(mv=0),
                   dict(mp=0), dict(mv=(1 << 28) + 1), dict(inv_h=0.0), dict(inv_h=nan), dict(inv_h=inf), dict(inv_h=-8.0), dict(width=0), dict(width=8193),
                   dict(height=0), dict(height=-1), dict(fx=0.0), dict(fx=nan), dict(fy=-1.0), dict(fy=inf), dict(cx=nan), dict(cy=inf), dict(near=0.0),
                   dict(near=nan), dict(pose=ctypes.addressof(bad_pose)), dict(eye=ctypes.addressof(far_eye)), dict(eye=ctypes.addressof(nan_eye)),
                   dict(min_count=0), dict(min_count=-3), dict(flags=4), dict(flags=-1)):
        assert call(**change) == -1 and err().startswith("psam_mapview"), change
    assert call(V=0) == -1 and "empty map" in err()
    for change in (dict(map=p + 8), dict(ws=ws + 8), dict(skip=p + 4), dict(keys=keys + 4), dict(stats=stats + 4)):
        assert call(**change) == -2 and err().startswith("psam_mapview") and "aligned" in err(), change
    assert call(map_bytes=nbytes - 1) == -3 and "map block too small" in err()
    assert call(ws_bytes=ws_bytes - 1) == -3 and "workspace too small (psam_mapview_ws_bytes)" in err()
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
    from point_sam_amd.predictor import PointSAMPredictor
    from point_sam_amd.scanmap import MapOverflow
    from point_sam_amd.views import View
    m = _host_map(V=8)
    block, mv, mp = m._block, m.max_voxels, m.max_pairs
    cam = R.axis_camera((0.0, 0.0, 0.0), 8, 6, 8.0, 4.0, 3.0)
    view = lambda *a, **k: ops.map_view(block, mv, mp, 8, *a, voxel_size=0.125, **k)
    for bad in ("x", None, {"pose": np.eye(4)}, np.eye(4)[:3]):
        with pytest.raises(TypeError, match="views.Camera"):
            view(bad)
        with pytest.raises(TypeError, match="views.Camera"):
            ops.map_view_eye(bad, 0.125)
        with pytest.raises(TypeError, match="views.Camera"):
            m.view(bad)
    for eye in ((0.0, 0.0, 1.5), (-1.001, 0.0, 0.0), (0.0, 3e6, 0.0)):
        outside = R.axis_camera(eye, 8, 6, 8.0, 4.0, 3.0)
        with pytest.raises(ValueError, match="outside"):
            ops.map_view_eye(outside, 0.125)
        with pytest.raises(ValueError, match="outside"):
            view(outside)
        with pytest.raises(ValueError, match="outside"):
            m.view(outside)
    with pytest.raises(ValueError, match="outside"):
        ops.map_view_eye(R.axis_camera((1.0, 0.0, 0.0), 8, 6, 8.0, 4.0, 3.0), 2.0 ** -20)      # the cell 2^21 does not exist
    for n in (0, -1, 1.0, True, 2 ** 31):
        with pytest.raises(ValueError, match="min_count"):
            view(cam, min_count=n)
    for skip in (torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), [0]):
        with pytest.raises(ValueError, match="skip"):
            view(cam, skip=skip)
    for flags in (4, -1, True, 1.0):
        with pytest.raises(ValueError, match="flags"):
            view(cam, flags=flags)
    for stats in (torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), [0, 0]):
        with pytest.raises(ValueError, match="stats"):
            view(cam, stats=stats)
    for V in (0, 65, 2.0, True):
        with pytest.raises(ValueError):
            ops.map_view(block, mv, mp, V, cam, voxel_size=0.125)
    with pytest.raises(TypeError):
        ops.map_view("x", mv, mp, 8, cam, voxel_size=0.125)
    with pytest.raises(ValueError):
        ops.map_view(block, mv, mp, 8, cam, voxel_size=0.0)
    with pytest.raises(PointSamHipError):                          # everything in order, but nothing lives on the GPU: no CPU fallback, no launch
        view(cam)
    # ScanMap.view, label_image and predictor.map_view
    with pytest.raises(ValueError, match="empty"):
        _host_map().view(cam)
    dead = _host_map(V=8)
    dead._flags = 1
    for call in (lambda: dead.view(cam), lambda: dead.label_image(View(torch.zeros(6, 8, dtype=torch.int64), cam, 8, 0))):
        with pytest.raises(MapOverflow):
            call()
    with pytest.raises(TypeError, match="occupied"):
        m.view(cam, occupied="x")
    with pytest.raises(ValueError, match="occupied"):
        m.view(cam, occupied=torch.ones(7, dtype=torch.bool))
    with pytest.raises(TypeError):
        m.label_image("not a view")
    with pytest.raises(ValueError, match="7 points"):
        m.label_image(View(torch.zeros(6, 8, dtype=torch.int64), cam, 7, 0))
    pred = PointSAMPredictor(model=None)
    with pytest.raises(TypeError, match="ScanMap"):
        pred.map_view("not a map", cam)
    with pytest.raises(TypeError, match="views.Camera"):
        pred.map_view(m, "not a camera")
    with pytest.raises(ValueError, match="empty"):
        pred.map_view(_host_map(), cam, occupied=None)             # needs no cloud to be set


# ------------------------------------------------------------------------------------------------ the demo's route
class _RefScanMap:
    """A stand-in ScanMap that answers view(), label_image(), cloud() and occupied() from the references, on the host."""

    def __init__(self, voxel_size, max_voxels):
        self.ref = SM.RefMap(voxel_size, max_voxels)
        self.free = set()

    num_voxels = property(lambda self: self.ref.V)
    num_adds = property(lambda self: self.ref.adds)

    def occupied(self, min_misses=2):
        return torch.tensor([v not in self.free for v in range(self.ref.V)])

    def cloud(self):
        return tuple(torch.from_numpy(a) for a in self.ref.cloud())

    def view(self, camera, occupied=None, min_count=1):
        from point_sam_amd.views import View
        skip = None if occupied is None else ~occupied.numpy()
        return View(torch.from_numpy(R.view(self.ref, camera, skip, min_count)[0]), camera, self.ref.V, 0)

    def label_image(self, view, min_votes=1):
        label = torch.from_numpy(self.ref.labels(min_votes)[0])
        idx = view.index
        return torch.where(idx >= 0, label[idx.clamp_min(0).long()], torch.full_like(idx, -1))


class FakeViewer:
    def __init__(self):
        self.calls = []

    def set_pointcloud(self, xyz, rgb):
        self.xyz, self.rgb = xyz, rgb

    def new_map(self, voxel_size, max_voxels):
        return _RefScanMap(voxel_size, max_voxels)

    def map_add(self, m, labels=None, pose=None):
        from point_sam_amd.scanmap import AddResult
        ids, new, acc, rej = m.ref.add(self.xyz[0].numpy(), self.rgb[0].numpy(), None if labels is None else labels.numpy(), pose)
        return AddResult(torch.from_numpy(ids), new, acc, rej)

    def map_view(self, m, camera, occupied=True, min_count=1):
        self.calls.append((camera, occupied))
        return m.view(camera, occupied, min_count)


def _req(port, path, body=None):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=120)
    c.request("POST", path, None if body is None else json.dumps(body), {"Content-Type": "application/json"})
    r = c.getresponse()
    return r.status, json.loads(r.read())


def test_map_view_route_answers_with_colour_index_depth_and_labels():
    from point_sam_amd.demo_server import DemoSession, serve
    pred = FakeViewer()
    h = 0.125
    srv = serve(DemoSession(pred, device="cpu", map_voxel_size=h, map_max_voxels=4096), "127.0.0.1", 0)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    try:
        port = srv.server_address[1]
        camera = {"eye": [0.03, -0.02, 0.05], "target": [0.9, 0.1, 0.0], "up": [0, 0, 1], "fov_y_degrees": 70.0, "width": 12, "height": 8}
        st, out = _req(port, "/map/view", {"camera": camera})
        assert st == 400 and "empty" in out["error"]
        # a wall at x = 0.8 with a ghost voxel in front of it, labelled by height
        ys, zs = np.meshgrid(np.arange(-0.9, 0.9, h / 2), np.arange(-0.9, 0.9, h / 2))
        wall = np.stack([np.full(ys.size, 0.8), ys.reshape(-1), zs.reshape(-1)], 1)
        xyz = np.concatenate([wall, [[0.4, 0.03, 0.03]]]).astype(np.float32)
        rgb = np.tile(np.array([[0.2, 0.4, 0.6]], dtype=np.float32), (len(xyz), 1))
        labels = (xyz[:, 2] > 0).astype(int).tolist()
        st, _ = _req(port, "/sampled_pointcloud", {"points": {str(i): float(v) for i, v in enumerate(xyz.flatten())},
                                                   "colors": {str(i): float(v) for i, v in enumerate(rgb.flatten())}})
        assert st == 200
        st, out = _req(port, "/map/add", {"labels": labels})
        assert st == 200 and out["num_voxels"] > 100
        ref = SM.RefMap(h, 4096)
        ref.add(xyz, rgb, np.asarray(labels))
        ghost = int(ref.locate(xyz[-1:])[0])
        from point_sam_amd.demo_server import DemoSession as D
        cam = D._camera(camera)
        want, _ = R.view(ref, cam)
        st, out = _req(port, "/map/view", {"camera": camera})
        assert st == 200 and set(out) == {"width", "height", "rgb", "index", "depth", "labels"} and (out["width"], out["height"]) == (12, 8)
        index = np.frombuffer(base64.b64decode(out["index"]), dtype="<i4").reshape(8, 12)
        depth = np.frombuffer(base64.b64decode(out["depth"]), dtype="<f4").reshape(8, 12)
        label = np.frombuffer(base64.b64decode(out["labels"]), dtype="<i4").reshape(8, 12)
        img = np.frombuffer(base64.b64decode(out["rgb"]), dtype=np.uint8).reshape(8, 12, 3)
        hit = want != R.EMPTY
        assert hit.sum() > 40 and np.array_equal(index, np.where(hit, want & 0xffffffff, -1)) and (index == ghost).any()
        assert np.array_equal(depth[hit].view(np.uint32), (want[hit] >> 32).astype(np.uint32)) and np.isinf(depth[~hit]).all()
        assert np.array_equal(label, np.where(hit, ref.labels()[0][np.where(hit, index, 0)], -1)) and set(label[hit]) == {0, 1}
        assert (img[hit] == np.array([51, 102, 153])).all() and (img[~hit] == 0).all()
        assert pred.calls[-1][1] is None, "without min_misses nothing is seen through"
        # with min_misses the map's occupied() goes to the predictor
        st, out2 = _req(port, "/map/view", {"camera": camera, "min_misses": 2, "min_votes": 1000})
        assert st == 200 and pred.calls[-1][1].dtype == torch.bool and out2["index"] == out["index"]
        assert (np.frombuffer(base64.b64decode(out2["labels"]), dtype="<i4") == -1).all(), "no voxel has a thousand votes"
        for bad in ({}, {"camera": "x"}, {"camera": camera, "splat": 1}, {"camera": camera, "min_misses": -1}, {"camera": camera, "min_votes": 0},
                    {"camera": dict(camera, eye=[0.0, 0.0, 1.5])}, {"camera": dict(camera, width=0)}):
            n = len(pred.calls)
            st, err = _req(port, "/map/view", bad)
            assert st == 400 and "error" in err and len(pred.calls) == n, bad
    finally:
        srv.shutdown()
        srv.server_close()
