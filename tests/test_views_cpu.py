"""Camera views, the part that needs no GPU: the numpy reference's rules on hand-made points and on the inputs the GPU tests use, the C entry points'
declarations and refusals, Camera.look_at, every ValueError of the Python host raised before any device work, and the demo's /view and /click_pixel
routes against a stand-in predictor."""
import base64
import ctypes
import http.client
import json
import os
import re
import threading
import warnings

import numpy as np
import pytest
import torch

import view_reference as V
from point_sam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEW_ENTRY_POINTS = ("psam_view_splat", "psam_view_pick", "psam_view_paint_ids", "psam_view_paint_rows", "psam_view_lift_bits")


# ------------------------------------------------------------------------------------------------ the reference's rules
def _pixels(pts, cam):
    ok, px, py, _ = V.project(pts, cam)
    return [(int(x), int(y)) if o else None for o, x, y in zip(ok, px, py)]


def test_reference_rules_on_hand_made_points():
    with warnings.catch_warnings():
        warnings.simplefilter("error")                     # no overflow or invalid-cast warning may turn into a pixel
        pts, want = V.hand_points()
        assert _pixels(pts, V.Cam()) == want
        cam, p = V.negzero_case()
        ok, px, py, depth = V.project(p, cam)
        assert ok.tolist() == [True] and (px[0], py[0]) == (0, 0) and depth[0] == 1
        cam, p, want = V.tiny_case()
        assert _pixels(p, cam) == want
        p, cam_in, cam_out = V.near_case()
        assert V.project(p, cam_in)[0].tolist() == [True] and V.project(p, cam_out)[0].tolist() == [False]
        keys = V.splat(pts, V.Cam(), 0)
    assert (keys != V.EMPTY).sum() == 3                    # four points in view, two of them on the principal ray
    assert V.index_of(keys)[48, 64] == 0                   # the principal point beats the far point on the same ray (index 0 < the last, depth 1 < 3e38)
    assert V.depth_of(keys)[48, 64] == 1 and np.isinf(V.depth_of(keys)[0, 1]) and V.index_of(keys)[0, 1] == -1


def test_plane_case_every_pixel_is_decided_by_the_index():
    pts, cam = V.plane_case(), V.Cam()
    assert pts.shape == (3200, 3)
    keys = V.splat(pts, cam, 0)
    full = keys != V.EMPTY
    assert full.sum() == 1089 and full.sum() >= 1000
    ok, px, py, depth = V.project(pts, cam)
    win_depth = V.depth_of(keys)
    tied = np.zeros(keys.shape, dtype=np.int64)
    np.add.at(tied, (py[ok], px[ok]), depth[ok] == win_depth[py[ok], px[ok]])
    assert (tied[full] >= 2).all()                         # at least two points at the winning depth in every non-empty pixel
    assert (V.index_of(keys)[full] < 1600).all()           # ties go to the lower index: the first copy


def test_sphere_case_footprint_and_visibility():
    pts, cam = V.sphere_case(), V.Cam()
    near = {}
    for s in (0, 1):
        keys = V.splat(pts, cam, s)
        idx = V.index_of(keys)[keys != V.EMPTY]
        near[s] = (pts[idx, 2] < 0).mean()
    assert near[0] < 0.70 and near[1] >= 0.99, near        # s = 0 shows the back through the gaps, s = 1 closes them
    bits, area = V.lift(pts, cam, V.splat(pts, cam, 1), None, 0.05)
    vis = V.unpack(bits, len(pts))[0]
    assert area[0] == vis.sum() and 0.15 <= vis.mean() <= 0.35, vis.mean()
    assert (vis & (pts[:, 2] > 0.2)).mean() < 0.01


def test_reference_pick_rules():
    keys = np.full((9, 9), V.EMPTY, dtype=np.uint64)
    k = lambda depth, i: (np.uint64(np.float32(depth).view(np.uint32)) << np.uint64(32)) | np.uint64(i)
    keys[4, 4] = k(2.0, 7)
    keys[4, 6] = k(1.0, 3)                                 # distance^2 4 from (4, 4), nearer in depth
    keys[2, 4] = k(1.5, 5)                                 # distance^2 4 from (4, 4) too
    assert V.pick(keys, [[4, 4]], 0).tolist() == [7]       # an exact hit
    assert V.pick(keys, [[4, 4]], 2).tolist() == [7]       # the nearest in the window, not the nearest in depth
    # (5, 3): pixel (4, 4) at d^2 = 2, pixel (6, 4) at d^2 = 2, pixel (4, 2) at d^2 = 2 -- an equal-distance triple the key decides: depth 1.0 wins
    assert V.pick(keys, [[5, 3]], 1).tolist() == [3] and V.pick(keys, [[5, 3]], 2).tolist() == [3]
    assert V.pick(keys, [[4, 3]], 1).tolist() == [5] and V.pick(keys, [[5, 4]], 1).tolist() == [3]      # the pair (4,4) / (6,4): the key decides
    assert V.pick(keys, [[0, 8]], 2).tolist() == [-1] and V.pick(keys, [[8, 8]], 0).tolist() == [-1]      # an empty window
    assert V.pick(keys, [[-3, 4], [4, -10]], 16).tolist() == [7, 5]                                        # clicks outside the image: the window is clipped


def test_reference_paint_and_lift_rules():
    pts, cam = V.sphere_case(500), V.Cam(width=37, height=53, cx=18.0, cy=26.0, fx=40.0, fy=40.0)
    keys = V.splat(pts, cam, 0)
    bits = V.random_bits(3, 500, zero_rows=(0,), one_rows=(2,))
    rows, ids = V.paint_rows(keys, bits, 500), V.paint_ids(keys, bits, 500)
    full = keys != V.EMPTY
    assert not rows[0].any() and (rows[2].astype(bool) == full).all() and set(np.unique(ids)) <= {-1, 1, 2} and (ids[~full] == -1).all()
    assert (ids[full & (rows[1] == 1)] == 1).all()
    lifted, area = V.lift(pts, cam, keys, rows, 0.0)
    m, src = V.unpack(lifted, 500), V.unpack(bits, 500)
    assert (m <= src).all() and (area == m.sum(1)).all()
    win = V.index_of(keys)[full]
    for k in range(3):
        assert m[k][win[src[k][win]]].all()                # every winner whose bit was set comes back


# ------------------------------------------------------------------------------------------------ the C entry points
def test_view_entry_points_are_declared_bound_and_exported():
    from point_sam_amd.build import SOURCES, build_library
    build_library()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pointsam_hip.h")).read()
    declared = set(re.findall(r"\b(psam_view_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(VIEW_ENTRY_POINTS) == {n for n in _lib.SIGNATURES if n.startswith("psam_view_")}
    for n in VIEW_ENTRY_POINTS:
        assert hasattr(lib, n), n
        ret, args = re.search(r"(\w+) %s\(([^)]*)\)" % n, hdr).groups()
        want = [_lib.ptr if "*" in a or "psam_stream_t" in a else {"int32_t": _lib.i32, "float": _lib.f32}[a.split()[0]] for a in args.split(",")]
        assert ret == "int32_t" and _lib.SIGNATURES[n] == (_lib.i32, want), n
    flags = dict(SOURCES)["views.hip"]
    assert "-ffp-contract=off" in flags and "-fno-slp-vectorize" in flags
    csrc = os.path.join(ROOT, "point_sam_amd", "csrc")
    src = open(os.path.join(csrc, "views.hip")).read()
    assert '#include "rigid_pose.h"' in src and '#include "row_popcount.h"' in src and "atomicMin(" in src
    # one copy of the pose arithmetic: transfer.hip and views.hip share rigid_pose.h
    assert '#include "rigid_pose.h"' in open(os.path.join(csrc, "transfer.hip")).read()
    for f in ("transfer.hip", "views.hip"):
        assert "P.m[0] *" not in open(os.path.join(csrc, f)).read(), f


def test_view_entry_points_reject_bad_arguments_on_the_host():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 15) & ~15               # a non-null, aligned pointer; never dereferenced by the device: every call below is refused
    pose = (ctypes.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 3)
    nan, inf = float("nan"), float("inf")

    def bad_pose(a, v):
        w = (ctypes.c_float * 12)(*pose)
        w[a] = v
        return w

    def refused(status, code, word):
        assert status == code, (status, lib.psam_last_error_string())
        assert word in lib.psam_last_error_string(), lib.psam_last_error_string()

    def camera_refusals(call):
        for name in ("width", "height"):
            for bad in (0, -1, 8193):
                refused(call(**{name: bad}), -1, b"width and height")
        for name in ("fx", "fy"):
            for bad in (0.0, -1.0, inf, nan):
                refused(call(**{name: bad}), -1, b"fx and fy")
        for name in ("cx", "cy"):
            for bad in (inf, -inf, nan):
                refused(call(**{name: bad}), -1, b"cx and cy")
        for bad in (0.0, -1.0, inf, nan):
            refused(call(near=bad), -1, b"near")
        for a, v in ((0, nan), (7, inf), (11, -inf)):
            w = bad_pose(a, v)
            refused(call(pose=ctypes.addressof(w)), -1, b"pose")
        for bad in (0, -3, (1 << 28) + 1):
            refused(call(N=bad), -1, b"0 < N")

    cam = dict(pose=ctypes.addressof(pose), fx=100.0, fy=100.0, cx=32.0, cy=24.0, width=64, height=48, near=0.01)
    good = dict(xyz=p, N=1000, **cam, s=1, keys=p)
    splat = lambda **kw: lib.psam_view_splat(*{**good, **kw}.values(), None)
    for name in ("xyz", "pose", "keys"):
        refused(splat(**{name: None}), -1, b"null")
    camera_refusals(splat)
    for bad in (-1, 4, 100):
        refused(splat(s=bad), -1, b"footprint")
    refused(splat(keys=p + 4), -2, b"aligned")
    refused(splat(xyz=p + 2), -2, b"aligned")

    good_pick = dict(keys=p, width=64, height=48, pixels=p, P=10, w=2, out=p)
    pick = lambda **kw: lib.psam_view_pick(*{**good_pick, **kw}.values(), None)
    for name in ("keys", "pixels", "out"):
        refused(pick(**{name: None}), -1, b"null")
    for name in ("width", "height"):
        for bad in (0, 8193):
            refused(pick(**{name: bad}), -1, b"width and height")
    for bad in (0, -1):
        refused(pick(P=bad), -1, b"0 < P")
    for bad in (-1, 17):
        refused(pick(w=bad), -1, b"window")
    refused(pick(keys=p + 4), -2, b"aligned")

    good_paint = dict(keys=p, width=64, height=48, bits=p, K=3, N=1000, out=p)
    for fn in (lib.psam_view_paint_ids, lib.psam_view_paint_rows):
        paint = lambda **kw: fn(*{**good_paint, **kw}.values(), None)
        for name in ("keys", "bits", "out"):
            refused(paint(**{name: None}), -1, b"null")
        for name in ("width", "height"):
            for bad in (0, 8193):
                refused(paint(**{name: bad}), -1, b"width and height")
        for kw in (dict(K=0), dict(K=-1), dict(N=0), dict(N=(1 << 28) + 1)):
            refused(paint(**kw), -1, b"K > 0")
        refused(paint(bits=p + 4), -2, b"aligned")

    good_lift = dict(xyz=p, N=1000, **cam, keys=p, img=p, K=2, tau=0.05, bits=p, area=p)
    lift = lambda **kw: lib.psam_view_lift_bits(*{**good_lift, **kw}.values(), None)
    for name in ("xyz", "pose", "keys", "bits"):
        refused(lift(**{name: None}), -1, b"null")
    camera_refusals(lift)
    for bad in (-1e-6, -inf, nan):
        refused(lift(tau=bad), -1, b"tau")
    for kw in (dict(K=0), dict(K=-2), dict(img=None, K=2)):
        refused(lift(**kw), -1, b"K")
    refused(lift(bits=p + 4), -2, b"aligned")
    refused(lift(area=p + 2), -2, b"aligned")


# ------------------------------------------------------------------------------------------------ the Python host
def test_camera_validation_and_look_at():
    from point_sam_amd.views import Camera
    cam = Camera(V.IDENTITY, 160, 160, 64, 48, 128, 96, near=0.01)
    ref = V.Cam()
    assert np.array_equal(cam.pose_words, ref.pose_words) and cam.pose.shape == (3, 4)
    assert (cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height, cam.near) == (ref.fx, ref.fy, ref.cx, ref.cy, ref.width, ref.height, ref.near)
    P4 = np.concatenate([V.IDENTITY.astype(np.float64), [[0, 0, 0, 1]]], 0)
    assert np.array_equal(Camera(P4, 1, 1, 0, 0, 1, 1).pose_words, cam.pose_words)          # a 4 x 4 is accepted, as by ops.transfer_pose
    bad4 = P4.copy(); bad4[3, 3] = 2
    for kw in (dict(pose=None), dict(pose=bad4), dict(pose=np.full((3, 4), np.nan)), dict(pose=np.eye(3)), dict(fx=0), dict(fy=-1.0), dict(fx=float("inf")),
               dict(fy=float("nan")), dict(fx="1"), dict(cx=float("nan")), dict(cy=float("inf")), dict(cx=1e300), dict(width=0), dict(height=8193),
               dict(width=12.0), dict(height=True), dict(near=0), dict(near=-1e-3), dict(near=float("nan")), dict(near=1e-60)):
        args = dict(pose=V.IDENTITY, fx=160, fy=160, cx=64, cy=48, width=128, height=96, near=0.01)
        with pytest.raises(ValueError):
            Camera(**{**args, **kw})
    # hand-computed: from (0, 0, -3) towards the origin with the image's top along -y, the rotation is the identity and the translation (0, 0, 3);
    # a 90 degree vertical field of view over 96 rows gives fy = 48 / tan(45 deg) = 48
    cam = Camera.look_at((0, 0, -3), (0, 0, 0), (0, -1, 0), 90.0, 128, 96)
    assert np.array_equal(cam.pose, V.IDENTITY)
    assert abs(cam.fy - 48) < 1e-5 and cam.fx == cam.fy and (cam.cx, cam.cy, cam.width, cam.height, cam.near) == (64, 48, 128, 96, float(np.float32(1e-3)))
    # from (3, 0, 0) towards the origin, z up: the camera's z is -x of the world, its x is z x up = (-1,0,0) x (0,0,1) = (0, 1, 0), its y is z x x = (0, 0, -1)
    cam = Camera.look_at((3, 0, 0), (0, 0, 0), (0, 0, 1), 60.0, 64, 64)
    assert np.allclose(cam.pose, [[0, 1, 0, 0], [0, 0, -1, 0], [-1, 0, 0, 3]], atol=1e-7)
    assert abs(cam.fy - 32 / np.tan(np.pi / 6)) < 1e-4
    for bad in (dict(eye=(0, 0, 0)), dict(up=(0, 0, 2)), dict(fov=0), dict(fov=180), dict(eye=(float("nan"), 0, 0)), dict(eye=(1, 2))):
        a = dict(eye=(0, 0, -3), target=(0, 0, 0), up=(0, -1, 0), fov=60.0)
        a.update(bad)
        with pytest.raises(ValueError):
            Camera.look_at(a["eye"], a["target"], a["up"], a["fov"], 64, 64)


def test_view_properties_and_colour_on_the_cpu():
    from point_sam_amd.views import Camera, View
    pts, ref = V.sphere_case(300), V.Cam(width=16, height=12, cx=8, cy=6, fx=20, fy=20)
    keys = V.splat(pts, ref, 1)
    view = View(torch.from_numpy(keys.view(np.int64).copy()), Camera(V.IDENTITY, 20, 20, 8, 6, 16, 12, 0.01), 300)
    assert np.array_equal(view.index.numpy(), V.index_of(keys)) and view.index.dtype == torch.int32
    assert np.array_equal(view.depth.numpy(), V.depth_of(keys))
    assert (keys == V.EMPTY).any() and (keys != V.EMPTY).any()
    rgb = torch.rand(300, 3)
    img = view.colour(rgb, background=(0.25, 0.5, 0.75))
    idx = V.index_of(keys)
    assert img.shape == (12, 16, 3)
    assert torch.equal(img[torch.from_numpy(idx >= 0)], rgb[torch.from_numpy(idx[idx >= 0]).long()])
    assert torch.equal(img[torch.from_numpy(idx < 0)], torch.tensor([0.25, 0.5, 0.75]).expand(int((idx < 0).sum()), 3))
    with pytest.raises(ValueError):
        view.colour(torch.rand(299, 3))


def test_view_ops_refuse_bad_arguments_before_any_device_work():
    from point_sam_amd import ops
    from point_sam_amd.views import Camera
    cam = Camera(V.IDENTITY, 160, 160, 64, 48, 128, 96, 0.01)
    xyz = torch.rand(100, 3)
    for bad in (-1, 4, 1.0, True, None):
        with pytest.raises(ValueError, match="splat"):
            ops.view_splat(xyz, cam, bad)
    with pytest.raises(TypeError):
        ops.view_splat(xyz, "camera")
    with pytest.raises(TypeError):
        ops.view_splat(xyz.double(), cam)
    with pytest.raises(ValueError):
        ops.view_splat(torch.rand(100, 2), cam)
    with pytest.raises(_lib.PointSamHipError):             # every check passed: the HIP path has no CPU fallback
        ops.view_splat(xyz, cam)
    keys = torch.full((96, 128), -1, dtype=torch.int64)
    for call in (lambda: ops.view_pick(keys, torch.zeros(3, 2, dtype=torch.int32)), lambda: ops.view_paint_ids(keys, torch.zeros(2, 2, dtype=torch.int64), 100),
                 lambda: ops.view_paint_rows(keys, torch.zeros(2, 2, dtype=torch.int64), 100), lambda: ops.view_lift_bits(xyz, cam, keys, None, 0.0)):
        with pytest.raises(_lib.PointSamHipError):
            call()


class _State:
    def __init__(self, n, batch=1):
        self.coords = torch.zeros(batch, n, 3)


def test_predictor_refuses_foreign_views_and_bad_arguments():
    from point_sam_amd.predictor import PointSAMPredictor
    from point_sam_amd.views import Camera, View
    cam = Camera(V.IDENTITY, 160, 160, 64, 48, 128, 96, 0.01)
    pred = PointSAMPredictor(None)
    view = View(torch.full((96, 128), -1, dtype=torch.int64), cam, 50)
    for call in (lambda: pred.render_view(cam), lambda: pred.pick(view, [[1, 2]]), lambda: pred.click_pixels(view, [[1, 2]], [1]),
                 lambda: pred.mask_images(view, torch.zeros(1, 1, dtype=torch.int64)), lambda: pred.lift_masks(view, torch.zeros(96, 128, dtype=torch.uint8), 0.0),
                 lambda: pred.visible_bits(view, 0.0)):
        with pytest.raises(RuntimeError, match="set_pointcloud"):
            call()
    pred._state = _State(60)
    pred._keepalive = (torch.zeros(1, 60, 3), torch.zeros(1, 60, 3))
    with pytest.raises(TypeError, match="Camera"):
        pred.render_view("camera")
    with pytest.raises(ValueError, match="cloud"):
        pred.render_view(cam, cloud=1)
    for call in (lambda: pred.pick(view, [[1, 2]]), lambda: pred.click_pixels(view, [[1, 2]], [1]), lambda: pred.mask_images(view, torch.zeros(1, 1, dtype=torch.int64)),
                 lambda: pred.lift_masks(view, torch.zeros(96, 128, dtype=torch.uint8), 0.0), lambda: pred.visible_bits(view, 0.0)):
        with pytest.raises(ValueError, match="50 points.*60"):       # a view of another cloud: both counts are named
            call()
    with pytest.raises(TypeError, match="View"):
        pred.pick("view", [[1, 2]])
    view = View(torch.full((96, 128), -1, dtype=torch.int64), cam, 60)
    with pytest.raises(ValueError, match="pixels"):
        pred.pick(view, [[1, 2, 3]])
    with pytest.raises(TypeError, match="integers"):
        pred.pick(view, [[1.5, 2.0]])
    with pytest.raises(ValueError, match="labels"):
        pred.click_pixels(view, [[1, 2], [3, 4]], [1])
    with pytest.raises(ValueError, match="window"):
        pred.pick(view, [[1, 2]], window=17)
    with pytest.raises(ValueError, match="words"):                   # the width check and its message are mask_geometry's
        pred.mask_images(view, torch.zeros(2, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="rows"):
        pred.mask_images(view, torch.zeros(2, 1, dtype=torch.int64), rows=1)
    with pytest.raises(ValueError, match="tau"):
        pred.visible_bits(view, -1.0)
    with pytest.raises(ValueError, match="tau"):
        pred.lift_masks(view, torch.zeros(96, 128, dtype=torch.uint8), float("nan"))
    with pytest.raises(ValueError, match="images"):
        pred.lift_masks(view, torch.zeros(2, 96, 127, dtype=torch.uint8), 0.0)


# ------------------------------------------------------------------------------------------------ the demo routes
class FakeViewer:
    """set_pointcloud / predict_masks as tests/test_demo_server_cpu.py's stand-in; render_view / click_pixels answer from the numpy reference."""

    def __init__(self):
        self.calls = []

    def set_pointcloud(self, xyz, rgb):
        self.xyz, self.rgb = xyz, rgb

    def predict_masks(self, pts, labels, prompt_mask, multimask):
        self.calls.append((pts.clone(), labels.clone(), None if prompt_mask is None else prompt_mask.clone(), multimask))
        logit = 0.5 - (self.xyz[0] - pts[0][-1]).norm(dim=-1)
        return logit[None, None], torch.tensor([[0.9]]), logit[None, None]

    def render_view(self, camera, splat=1):
        from point_sam_amd.views import View
        keys = V.splat(self.xyz[0].numpy(), camera, splat)
        return View(torch.from_numpy(keys.view(np.int64).copy()), camera, self.xyz.shape[1], splat)

    def click_pixels(self, view, pixels, labels, window=2):
        idx = V.pick(view.keys.numpy().view(np.uint64), pixels, window)
        if (idx < 0).any():
            raise ValueError(f"click_pixels: the click at pixel ({pixels[0][0]}, {pixels[0][1]}) hits no point within {window} pixels")
        return self.xyz[0][torch.from_numpy(idx).long()][None], torch.as_tensor(labels)[None]


def _req(port, method, path, body=None):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=10)
    c.request(method, path, None if body is None else json.dumps(body), {"Content-Type": "application/json"})
    r = c.getresponse()
    return r.status, json.loads(r.read())


def test_view_and_click_pixel_routes_against_a_stand_in_predictor(tmp_path):
    from point_sam_amd.demo_server import DemoSession, serve
    pts = V.sphere_case(400).astype(np.float64)
    with open(tmp_path / "ball.ply", "w") as f:
        f.write(f"ply\nformat ascii 1.0\nelement vertex {len(pts)}\nproperty float x\nproperty float y\nproperty float z\n"
                "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
        for i, p in enumerate(pts):
            f.write(f"{p[0]} {p[1]} {p[2]} {i % 256} 0 128\n")
    pred = FakeViewer()
    sess = DemoSession(pred, models_dir=str(tmp_path), output_dir=str(tmp_path / "results"), device="cpu")
    srv = serve(sess, "127.0.0.1", 0)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    try:
        port = srv.server_address[1]
        camera = {"pose": V.IDENTITY.tolist(), "fx": 40, "fy": 40, "cx": 16, "cy": 12, "width": 32, "height": 24, "near": 0.01}
        st, out = _req(port, "POST", "/view", {"camera": camera})
        assert st == 400 and "point cloud" in out["error"]
        _req(port, "GET", "/pointcloud/ball.ply")
        st, out = _req(port, "POST", "/click_pixel", {"pixel": [16, 12], "label": 1})
        assert st == 400 and "before any /view" in out["error"]
        for bad in ({}, {"camera": 3}, {"camera": dict(camera, width=0)}, {"camera": dict(camera, fx=-1)}, {"camera": dict(camera, extra=1)},
                    {"camera": {k: v for k, v in camera.items() if k != "pose"}}, {"camera": camera, "splat": 9}, {"camera": camera, "other": 1}):
            st, out = _req(port, "POST", "/view", bad)
            assert st == 400 and "error" in out, bad
        st, out = _req(port, "POST", "/view", {"camera": camera})
        assert st == 200 and out["width"] == 32 and out["height"] == 24
        img = np.frombuffer(base64.b64decode(out["rgb"]), dtype=np.uint8).reshape(24, 32, 3)
        ref = V.Cam(fx=40, fy=40, cx=16, cy=12, width=32, height=24)
        keys = V.splat(sess.pc_xyz[0].numpy(), ref, 1)
        idx = V.index_of(keys)
        assert (img[idx < 0] == 0).all() and (idx >= 0).sum() > 100
        want = np.round(sess.pc_rgb[0].numpy()[idx[idx >= 0]] * 255).astype(np.uint8)
        assert np.array_equal(img[idx >= 0], want)
        # a look_at camera is accepted too
        st, out2 = _req(port, "POST", "/view", {"camera": {"eye": [0, 0, -3], "target": [0, 0, 0], "up": [0, -1, 0], "fov_y_degrees": 43.6, "width": 32, "height": 24}})
        assert st == 200 and len(base64.b64decode(out2["rgb"])) == 24 * 32 * 3
        _req(port, "POST", "/view", {"camera": camera})
        # a click on a pixel == a click on the picked point through /segment
        for bad in ({"pixel": [16, 12]}, {"pixel": [16], "label": 1}, {"pixel": [1.5, 2], "label": 1}, {"pixel": [16, 12], "label": 1, "extra": 0}):
            st, out = _req(port, "POST", "/click_pixel", bad)
            assert st == 400 and sess.prompts == [], bad
        st, out = _req(port, "POST", "/click_pixel", {"pixel": [0, 0], "label": 1, "window": 0})
        assert st == 400 and "(0, 0)" in out["error"] and sess.prompts == []                      # the corner shows nothing
        st, got = _req(port, "POST", "/click_pixel", {"pixel": [16, 12], "label": 1})
        assert st == 200
        picked = int(V.pick(keys, [[16, 12]], 2)[0])
        assert picked >= 0 and np.allclose(sess.prompts[-1], sess.pc_xyz[0][picked].tolist())
        assert _req(port, "POST", "/clear")[0] == 200
        st, want = _req(port, "POST", "/segment", {"prompt_point": sess.pc_xyz[0][picked].tolist(), "prompt_label": 1})
        assert st == 200 and got == want
        assert torch.equal(pred.calls[-1][0], pred.calls[-2][0]) and torch.equal(pred.calls[-1][1], pred.calls[-2][1])
        # another cloud drops the view
        _req(port, "GET", "/pointcloud/ball.ply")
        st, out = _req(port, "POST", "/click_pixel", {"pixel": [16, 12], "label": 1})
        assert st == 400 and "before any /view" in out["error"]
    finally:
        srv.shutdown()
