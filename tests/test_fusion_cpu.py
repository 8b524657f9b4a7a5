"""Multi-view label fusion, the part that needs no GPU: the numpy reference's identities and hand cases, the ring fixture's conditions on the reference,
the host-side linking (point_sam_amd/fusion.py), the C entry points' declarations and refusals, every error of the Python host raised before any device
work, and the demo's /fuse_labels route against a stand-in predictor."""
import base64
import ctypes
import http.client
import json
import os
import re
import shutil
import subprocess
import threading

import numpy as np
import pytest
import torch

import frames_reference as R
import fusion_reference as FR
import view_reference as V
from point_sam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSION_ENTRY_POINTS = ("psam_fuse_region_bits", "psam_fuse_vote", "psam_label_bits")
I32 = np.iinfo(np.int32)


def _camera(ref):
    from point_sam_amd.views import Camera
    return Camera(ref.pose_words.reshape(3, 4), ref.fx, ref.fy, ref.cx, ref.cy, ref.width, ref.height, ref.near)


@pytest.fixture(scope="module")
def ring():
    case = FR.ring_case()
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


# ------------------------------------------------------------------------------------------------ the reference's identities
@pytest.mark.parametrize("tau", [0.0, 0.05])
def test_region_rows_are_lifts_per_view_and_label(tau):
    depth, rgb, cams, far = R.pattern_case(3, 24, 43)
    xyz, ncams, keys = FR.frames_case(depth, rgb, cams, far)
    labels = FR.pattern_labels(depth.shape, 4)
    rb = np.array([0, 4, 4, 7], dtype=np.int32)                    # an empty view in the middle, three regions in the last
    bits, area = FR.region_bits(xyz, ncams, keys, labels, rb, tau)
    assert bits.shape == (7 + 3, (len(xyz) + 63) // 64)
    for v in range(3):
        for l in range(int(rb[v + 1] - rb[v])):
            want, n = V.lift(xyz, ncams[v], keys[v], (labels[v] == l)[None], tau)
            assert np.array_equal(bits[rb[v] + l], want[0]) and area[rb[v] + l] == n[0], (v, l)
        want, n = V.lift(xyz, ncams[v], keys[v], None, tau)
        assert np.array_equal(bits[7 + v], want[0]) and area[7 + v] == n[0] and n[0] > 0, v
    assert area[:7].sum() > 0 and np.array_equal(FR.label_bits(np.array([0, 2, 2, -1, 3, I32.max], dtype=np.int32), 3)[1], [1, 0, 2])


# ------------------------------------------------------------------------------------------------ hand cases of the vote
def _one_point_views(labels):
    """One point straight ahead of Cam() at depth 1, seen by len(labels) identical views; view v's label image is the constant labels[v]."""
    cam = V.Cam()
    xyz = np.array([[0.0, 0.0, -2.0]], dtype=np.float32)
    keys = np.stack([V.splat(xyz, cam, 0)] * len(labels))
    lab = np.stack([np.full((cam.height, cam.width), l, dtype=np.int32) for l in labels])
    return xyz, [cam] * len(labels), keys, lab


def test_vote_tie_goes_to_the_lower_label_not_the_earlier_view():
    xyz, cams, keys, lab = _one_point_views([7, 3, 7, 3])
    out = FR.vote(xyz, cams, keys, lab, 0.0)
    assert (out["label"][0], out["votes"][0], out["seen"][0], out["labelled"][0], out["dropped"][0]) == (3, 2, 4, 4, 0)
    out = FR.vote(xyz, cams, keys, lab, 0.0, min_votes=3)
    assert (out["label"][0], out["votes"][0], out["seen"][0]) == (-1, 0, 4)
    out = FR.vote(*_one_point_views([7, 3, 7]), 0.0)
    assert (out["label"][0], out["votes"][0]) == (7, 2)


def test_vote_out_of_range_labels_are_seen_but_unlabelled():
    xyz, cams, keys, lab = _one_point_views([-1, 2, I32.max, I32.min, 1])
    rb = np.array([0, 2, 4, 6, 8, 10], dtype=np.int32)              # count_v = 2 everywhere: the 2 of view 1 is count_v itself
    out = FR.vote(xyz, cams, keys, lab, 0.0, rb)
    assert (out["label"][0], out["votes"][0], out["seen"][0], out["labelled"][0]) == (1, 1, 5, 1)
    out = FR.vote(xyz, cams, keys, lab, 0.0)                        # consistent ids: every l >= 0 is valid
    assert (out["label"][0], out["seen"][0], out["labelled"][0]) == (1, 5, 3)
    remap = np.array([5, -1] * 5, dtype=np.int32)                   # the one valid observation maps to an empty region
    out = FR.vote(xyz, cams, keys, lab, 0.0, rb, remap)
    assert (out["label"][0], out["votes"][0], out["seen"][0], out["labelled"][0]) == (-1, 0, 5, 0)


def test_vote_overflow_ten_identical_frames():
    depth, rgb, cams, far = FR.tiled_room(10)
    xyz, ncams, keys = FR.frames_case(depth, rgb, cams, far)
    assert len(xyz) == 10 * (R.ROOM_KEPT // 2)
    lab = np.stack([np.full(depth.shape[1:], v, dtype=np.int32) for v in range(10)])
    out = FR.vote(xyz[::97], ncams, keys, lab, 0.0)                  # a sample of all ten frames' points: the table is walked in Python
    assert (out["seen"] == 10).all() and (out["dropped"] == 2).all() and (out["label"] == 0).all() and (out["votes"] == 1).all()
    assert (out["labelled"] == 10).all()


# ------------------------------------------------------------------------------------------------ the ring fixture
def test_ring_fixture_reference(ring):
    """Measured on the reference: M = 30493 points, every one seen at tau = 0.02; overlap 0.5 and 0.8 both give 4 instances, and 8 points (0.026 %)
    carry an instance other than their object's."""
    M = len(ring["xyz"])
    assert M == 30493
    for overlap in (0.5, 0.8):
        out = FR.fuse(ring["xyz"], ring["cams"], ring["keys"], ring["labels"], FR.RING_TAU, overlap, 20)
        wrong = FR.ring_disagreement(out["label"], out["remap"], out["row_base"], ring["perm"], ring["obj"])
        print(f"ring overlap {overlap}: instances {out['num_instances']}, seen min {out['seen'].min()}, disagree {wrong} of {M}")
        assert out["num_instances"] == 4 and (out["seen"] > 0).all()
        assert wrong <= 0.001 * M


def test_ring_fixture_linked_on_a_voxel_working_cloud(ring):
    """The links made on the working cloud set_scene(max_points=4096) builds -- one point per voxel of the ladder size that leaves at most 4096, 3130 points
    here -- and the vote on the scan: measured on the reference, again 4 instances and the same 8 points of 30493 that disagree."""
    import scene_reference as S
    from point_sam_amd.scene import choose_voxel_size, ladder
    xyz = ring["xyz"]
    h = choose_voxel_size(None, 4096, count=lambda k: len(np.unique(S.keys(xyz, ladder(k)))))
    keep = S.downsample(xyz, h)[0]
    assert len(keep) == 3130
    out = FR.fuse(xyz, ring["cams"], ring["keys"], ring["labels"], FR.RING_TAU, 0.5, 20, link_xyz=xyz[keep])
    wrong = FR.ring_disagreement(out["label"], out["remap"], out["row_base"], ring["perm"], ring["obj"])
    assert out["num_instances"] == 4 and wrong <= 0.001 * len(xyz)


def test_ring_fixture_with_a_split_floor():
    """The floor's right image half is a fifth id in odd frames: 4 instances at overlap 0.5 (the half is contained in the floor), 6 at 0.8."""
    case = FR.ring_case(split_floor=True)
    got = [FR.fuse(case["xyz"], case["cams"], case["keys"], case["labels"], FR.RING_TAU, overlap, 20)["num_instances"] for overlap in (0.5, 0.8)]
    assert got == [4, 6]


def test_host_linking_equals_the_reference_on_the_ring(ring):
    from point_sam_amd.fusion import FusionConfig, link_regions
    rb = FR.row_base_of(ring["labels"])
    bits, area = FR.region_bits(ring["xyz"], ring["cams"], ring["keys"], ring["labels"], rb, FR.RING_TAU)
    inter = FR.intersections(bits)
    assert np.array_equal(np.diagonal(inter), area)
    for overlap in (0.5, 0.8):
        remap = link_regions(torch.from_numpy(inter), rb, FusionConfig(FR.RING_TAU, overlap=overlap))
        assert remap.dtype == np.int32 and np.array_equal(remap, FR.link_regions(inter, rb, overlap, 20))


# ------------------------------------------------------------------------------------------------ linking
def test_components_do_not_depend_on_the_edge_order_and_number_by_smallest_row():
    from point_sam_amd.fusion import components
    nonempty = np.array([1, 1, 0, 1, 1, 1, 1, 0, 1, 1], dtype=bool)
    edges = np.array([[8, 3], [3, 5], [1, 9], [4, 6], [6, 9]])
    want = np.array([0, 1, -1, 2, 1, 2, 1, -1, 2, 1], dtype=np.int32)      # {0}, {1, 4, 6, 9}, {3, 5, 8}: numbered by the rows 0 < 1 < 3
    rng = np.random.default_rng(0)
    for _ in range(20):
        e = edges[rng.permutation(len(edges))]
        flip = rng.random(len(e)) < 0.5
        e[flip] = e[flip][:, ::-1]
        assert np.array_equal(components(nonempty, e), want)
    assert np.array_equal(components(nonempty, np.zeros((0, 2), dtype=np.int64)), [0, 1, -1, 2, 3, 4, 5, -1, 6, 7])
    assert np.array_equal(components(np.zeros(3, dtype=bool), []), [-1, -1, -1]) and components(np.zeros(0, dtype=bool), []).shape == (0,)
    assert np.array_equal(FR.components(nonempty, [tuple(e) for e in edges.tolist()]), want)


def test_link_rule_on_a_hand_made_matrix():
    from point_sam_amd.fusion import FusionConfig, link_edges, link_regions
    rb = [0, 2, 3, 4]                                               # regions 0, 1 in view 0; 2 in view 1; 3 in view 2 (empty)
    inter = np.zeros((7, 7), dtype=np.int32)

    def put(a, b, n):
        inter[a, b] = inter[b, a] = n
    for r, n in ((0, 100), (1, 50), (2, 120), (3, 0)):
        inter[r, r] = n
    put(0, 2, 40)                                                   # n
    put(0, 4 + 1, 80)                                               # ca: the points of 0 that view 1 sees
    put(2, 4 + 0, 60)                                               # cb: the points of 2 that view 0 sees
    put(1, 2, 29); put(1, 4 + 1, 30)                                # region 1: 29 of its 30 co-visible points shared, but 29 < 0.5 * 60
    cfg = FusionConfig(0.0, overlap=0.5, min_points=20)
    assert link_edges(inter, rb, cfg).tolist() == [[0, 2]]          # 40 >= 0.5 * 80 exactly
    assert link_regions(inter, rb, cfg).tolist() == [0, 1, 0, -1]
    assert link_edges(inter, rb, FusionConfig(0.0, overlap=0.5 + 1e-12)).tolist() == []      # the product and the compare are fp64
    assert link_edges(inter, rb, FusionConfig(0.0, overlap=0.5, min_points=61)).tolist() == []      # min(ca, cb) = 60
    assert link_edges(inter, np.array(rb), FusionConfig(0.0, overlap=0.25)).tolist() == [[0, 2], [1, 2]]
    assert link_regions(inter, rb, FusionConfig(0.0, overlap=0.25)).tolist() == [0, 0, 0, -1]
    put(0, 1, 100)                                                  # regions of ONE view are never linked, whatever the matrix says
    assert link_edges(inter, rb, cfg).tolist() == [[0, 2]]
    for bad_rb in ([1, 2, 3, 4], [0, 2, 1, 4], [0], [0.0, 1.0]):
        with pytest.raises(ValueError, match="row_base"):
            link_regions(inter, bad_rb, cfg)
    with pytest.raises(ValueError, match="inter"):
        link_regions(inter[:6, :6], rb, cfg)
    with pytest.raises(ValueError, match="inter"):
        link_regions(inter.astype(np.int64), rb, cfg)
    assert link_regions(np.zeros((2, 2), dtype=np.int32), [0, 0, 0], cfg).shape == (0,)


def test_fusion_config_refuses_bad_fields():
    from point_sam_amd.fusion import FusionConfig
    cfg = FusionConfig(0.02)
    assert (cfg.overlap, cfg.min_points, cfg.min_votes, cfg.max_regions) == (0.5, 20, 1, 8192) and "tuned" in FusionConfig.__doc__
    for kw in (dict(tau=-1), dict(tau=float("nan")), dict(tau="x"), dict(tau=True), dict(tau=0, overlap=0), dict(tau=0, overlap=1.5), dict(tau=0, overlap="a"),
               dict(tau=0, min_points=0), dict(tau=0, min_points=2.5), dict(tau=0, min_votes=0), dict(tau=0, min_votes=True), dict(tau=0, max_regions=0),
               dict(tau=0, max_regions=(1 << 20) + 1)):
        with pytest.raises(ValueError, match="FusionConfig"):
            FusionConfig(**kw)
    with pytest.raises(TypeError):
        FusionConfig(0.0, colour=1)
    for bad in ({"tau": 0, "colour": 1}, {"overlap": 0.5}, None, [("tau", 0)]):
        with pytest.raises(ValueError, match="FusionConfig"):
            FusionConfig.from_overrides(bad)
    assert FusionConfig.from_overrides({"tau": 0.1, "min_votes": 2}) == FusionConfig(0.1, min_votes=2)


# ------------------------------------------------------------------------------------------------ the C entry points
def test_fusion_entry_points_are_declared_bound_and_exported(tmp_path):
    from point_sam_amd.build import SOURCES, build_library
    build_library()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pointsam_hip.h")).read()
    assert "label fusion" in hdr
    declared = set(re.findall(r"\b(psam_fuse_[a-z0-9_]+|psam_label_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(FUSION_ENTRY_POINTS) == {n for n in _lib.SIGNATURES if n.startswith(("psam_fuse_", "psam_label_"))}
    for n in FUSION_ENTRY_POINTS:
        assert hasattr(lib, n), n
        ret, args = re.search(r"(\w+) %s\(([^)]*)\)" % n, hdr).groups()
        want = [_lib.ptr if "*" in a or "psam_stream_t" in a else {"int32_t": _lib.i32, "float": _lib.f32}[a.split()[0]] for a in args.split(",")]
        assert ret == "int32_t" and _lib.SIGNATURES[n] == (_lib.i32, want), n
    assert dict(SOURCES)["fusion.hip"] == dict(SOURCES)["views.hip"]
    csrc = os.path.join(ROOT, "point_sam_amd", "csrc")
    src = open(os.path.join(csrc, "fusion.hip")).read()
    assert '#include "rigid_pose.h"' in src and '#include "row_popcount.h"' in src and '#include "view_camera.h"' in src
    assert "atomic" not in src.replace("no atomic", "") and "P.m[0] *" not in src
    # one copy of the projection and of the visibility rule: views.hip and fusion.hip share view_camera.h
    assert '#include "view_camera.h"' in open(os.path.join(csrc, "views.hip")).read()
    for f in ("views.hip", "fusion.hip"):
        assert "bool view_project(" not in open(os.path.join(csrc, f)).read(), f
    assert "bool view_project(" in open(os.path.join(csrc, "view_camera.h")).read()
    if shutil.which("gcc") is None:
        pytest.skip("needs gcc")
    prog = ['#include "pointsam_hip.h"', "int main(void) {"]
    prog += [f"    void* p{i} = (void*){n};" for i, n in enumerate(FUSION_ENTRY_POINTS)]
    prog += ["    return " + " && ".join(f"p{i} != 0" for i in range(len(FUSION_ENTRY_POINTS))) + " ? 0 : 1;", "}"]
    c = tmp_path / "fusion_symbols.c"
    c.write_text("\n".join(prog))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-Wno-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "fusion_symbols.o")],
                   check=True)


def test_fusion_entry_points_reject_bad_arguments_on_the_host():
    buf = ctypes.create_string_buffer(1 << 16)
    FR.entry_point_refusals(_lib.load(), (ctypes.addressof(buf) + 15) & ~15)      # never dereferenced: every call is refused


# ------------------------------------------------------------------------------------------------ the Python host
def test_ops_refuse_bad_arguments_before_any_device_work():
    from point_sam_amd import ops
    cams = [_camera(c) for c in R.pattern_case(2, 5, 13)[2]]
    xyz, keys, labels = torch.zeros(9, 3), torch.zeros(2, 5, 13, dtype=torch.int64), torch.zeros(2, 5, 13, dtype=torch.int32)
    rb = [0, 1, 3]

    def both(match, exc=ValueError, **kw):
        a = dict(xyz=xyz, cameras=cams, keys=keys, labels=labels, row_base=rb, tau=0.0)
        a.update(kw)
        with pytest.raises(exc, match=match):
            ops.fuse_region_bits(**a)
        with pytest.raises(exc, match=match):
            ops.fuse_vote(**a)
    both("xyz", xyz=torch.zeros(9, 2)); both("xyz", TypeError, xyz=np.zeros((9, 3))); both("xyz", TypeError, xyz=torch.zeros(9, 3, dtype=torch.float64))
    both("keys", TypeError, keys=keys.int()); both("keys", keys=keys[0]); both("keys", keys=torch.zeros(0, 5, 13, dtype=torch.int64))
    both("labels", TypeError, labels=labels.long()); both("labels", labels=labels[:, :4]); both("labels", TypeError, labels=None)
    both("cameras", cameras=cams[:1]); both("cameras", cameras=cams[0]); both(r"cameras\[1\]", TypeError, cameras=[cams[0], 3])
    both(r"cameras\[1\]", cameras=[cams[0], _camera(V.Cam())])      # another size
    from point_sam_amd.views import Camera
    for field, value in (("fx", float("nan")), ("fy", -1.0), ("near", 0.0), ("cx", float("inf")), ("pose_words", np.full(12, np.inf, dtype=np.float32))):
        c = cams[1]
        broken = Camera.from_fp32(c.pose_words, c.fx, c.fy, c.cx, c.cy, c.width, c.height, c.near)
        setattr(broken, field, value)
        both(r"cameras\[1\] must be finite", cameras=[cams[0], broken])
    for bad in ([1, 1, 3], [0, 2, 1], [0, 1], [0, 1, 3, 4], [0.0, 1.0, 3.0], "abc", None, [0, 1, (1 << 20) + 1]):
        with pytest.raises(ValueError, match="row_base"):
            ops.fuse_region_bits(xyz, cams, keys, labels, bad, 0.0)
    for bad in ([1, 1, 3], [0, 2, 1], [0, 1]):
        with pytest.raises(ValueError, match="row_base"):
            ops.fuse_vote(xyz, cams, keys, labels, 0.0, bad)
    for bad in (-1.0, float("nan"), "1", True, None):
        both("tau", tau=bad)
    for bad in (0, -1, 1.5, True, 4097):
        with pytest.raises(ValueError, match="min_votes"):
            ops.fuse_vote(xyz, cams, keys, labels, 0.0, rb, min_votes=bad)
    remap = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match="remap needs"):
        ops.fuse_vote(xyz, cams, keys, labels, 0.0, None, remap)
    with pytest.raises(TypeError, match="remap"):
        ops.fuse_vote(xyz, cams, keys, labels, 0.0, rb, remap.long())
    with pytest.raises(ValueError, match="remap"):
        ops.fuse_vote(xyz, cams, keys, labels, 0.0, rb, remap[:2])
    # everything right but the device: the last check, and the message of the HIP path
    with pytest.raises(_lib.PointSamHipError, match="GPU"):
        ops.fuse_region_bits(xyz, cams, keys, labels, rb, 0.0)
    with pytest.raises(_lib.PointSamHipError, match="GPU"):
        ops.fuse_vote(xyz, cams, keys, labels, 0.0, rb, remap)

    lab = torch.zeros(9, dtype=torch.int32)
    for bad, exc in ((lab.long(), TypeError), (None, TypeError), (lab[None], ValueError), (lab[:0], ValueError)):
        with pytest.raises(exc, match="labels"):
            ops.label_bits(bad, 3)
    for bad in (0, -1, 2.0, True, (1 << 20) + 1):
        with pytest.raises(ValueError, match="K"):
            ops.label_bits(lab, bad)
    with pytest.raises(_lib.PointSamHipError, match="GPU"):
        ops.label_bits(lab, 3)


def test_fuse_labels_refuses_bad_arguments_before_any_device_work():
    from point_sam_amd.fusion import FusionConfig, Fused, check_labels, fuse
    from point_sam_amd.predictor import PointSAMPredictor
    from point_sam_amd.views import View
    pred = PointSAMPredictor(None)
    cfg = FusionConfig(0.0)
    with pytest.raises(TypeError, match="views"):
        pred.fuse_labels(None, np.zeros((1, 2, 2), dtype=np.int32), cfg)
    with pytest.raises(TypeError, match="views"):
        pred.fuse_labels([], np.zeros((1, 2, 2), dtype=np.int32), cfg)
    cam = _camera(V.Cam(width=13, height=5, cx=6.0, cy=2.0))
    views = [View(torch.zeros(5, 13, dtype=torch.int64), cam, 9, 0), View(torch.zeros(5, 13, dtype=torch.int64), cam, 9, 0)]
    with pytest.raises(RuntimeError, match="set_pointcloud"):
        pred.fuse_labels(views, np.zeros((2, 5, 13), dtype=np.int32), cfg)
    pred._state, pred._keepalive = object(), (torch.zeros(1, 9, 3), torch.zeros(1, 9, 3))      # a cached cloud of nine points, nothing encoded
    labels = np.zeros((2, 5, 13), dtype=np.int32)
    with pytest.raises(TypeError, match=r"view must be a views\.View"):
        pred.fuse_labels([views[0], 3], labels, cfg)
    with pytest.raises(ValueError, match="cloud of 8 points"):
        pred.fuse_labels([views[0], View(views[1].keys, cam, 8, 0)], labels, cfg)
    with pytest.raises(ValueError, match="one size"):
        pred.fuse_labels([views[0], View(torch.zeros(5, 12, dtype=torch.int64), cam, 9, 0)], labels, cfg)
    for bad, exc in ((labels.astype(np.int64), TypeError), (labels[:1], ValueError), (torch.zeros(2, 5, 13), TypeError), ("x", TypeError)):
        with pytest.raises(exc, match="labels"):
            pred.fuse_labels(views, bad, cfg)
    with pytest.raises(TypeError, match="FusionConfig"):
        pred.fuse_labels(views, labels, {"tau": 0.0})
    with pytest.raises(ValueError, match="consistent"):
        pred.fuse_labels(views, labels, cfg, consistent=1)
    many = labels.copy()
    many[0, 0, 0], many[1, 0, 0] = 5000, 4000
    with pytest.raises(ValueError, match=r"9002 regions.*max_regions = 8192"):
        pred.fuse_labels(views, many, cfg)
    many[0, 0, 0] = I32.max                                         # the count does not wrap
    with pytest.raises(ValueError, match=r"2147487649 regions"):
        pred.fuse_labels(views, many, cfg)
    assert check_labels(torch.from_numpy(labels), (2, 5, 13), "cpu", "t").dtype == torch.int32 and fuse is not None

    fused = Fused(*(torch.full((9,), -1, dtype=torch.int32) for _ in range(5)), num_instances=0)
    bits, area = fused.bits()
    assert tuple(bits.shape) == (0, 1) and bits.dtype == torch.int64 and tuple(area.shape) == (0,)
    with pytest.raises(ValueError, match="ids"):
        Fused(*(torch.zeros(9, dtype=torch.int32) for _ in range(5)), num_instances=1).bits([1])


# ------------------------------------------------------------------------------------------------ the demo's route
class FakeFuser:
    """set_frames / fuse_labels answer from the numpy references."""

    def __init__(self):
        self.fuse_calls = []

    def set_pointcloud(self, xyz, rgb):
        self.xyz, self.rgb = xyz, rgb

    def set_frames(self, depth, rgb, cameras, far, edge=0.05, depth_scale=None, max_points=None):
        from point_sam_amd.views import Camera, FrameSet
        out = R.frames(depth, rgb, cameras, far, edge, depth_scale)
        self.ref = out
        ncams = [Camera(n.pose_words.reshape(3, 4), n.fx, n.fy, n.cx, n.cy, n.width, n.height, n.near) for n in out["cams"]]
        return FrameSet(torch.from_numpy(out["keys"].view(np.int64)), ncams, torch.from_numpy(out["index"]), torch.from_numpy(out["xyz"]),
                        torch.from_numpy(out["rgb"]), out["center"], out["scale"])

    def fuse_labels(self, views, labels, cfg, consistent=False):
        from point_sam_amd.fusion import Fused, check_labels
        lab = check_labels(labels, views.keys.shape, "cpu", "fuse_labels").numpy()
        self.fuse_calls.append((lab.copy(), cfg, consistent))
        ref = self.ref
        if consistent:
            out = FR.vote(ref["xyz"], ref["cams"], ref["keys"], lab, cfg.tau, min_votes=cfg.min_votes)
            count = int(out["label"].max()) + 1
        else:
            out = FR.fuse(ref["xyz"], ref["cams"], ref["keys"], lab, cfg.tau, cfg.overlap, cfg.min_points, cfg.min_votes)
            count = out["num_instances"]
        return Fused(*(torch.from_numpy(out[k]) for k in ("label", "votes", "seen", "labelled", "dropped")), num_instances=count)


def _req(port, method, path, body=None):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
    c.request(method, path, None if body is None else json.dumps(body), {"Content-Type": "application/json"})
    r = c.getresponse()
    return r.status, json.loads(r.read())


def _b64(a):
    return base64.b64encode(np.ascontiguousarray(a).tobytes()).decode("ascii")


def test_fuse_labels_route(tmp_path):
    from point_sam_amd.demo_server import DemoSession, serve
    from point_sam_amd.fusion import FusionConfig
    depth, rgb, cams, far = R.pattern_case(2, 24, 43)
    specs = [{"pose": c.pose_words.reshape(3, 4).tolist(), "fx": c.fx, "fy": c.fy, "cx": c.cx, "cy": c.cy, "width": c.width, "height": c.height, "near": c.near}
             for c in cams]
    labels = np.stack([np.where(np.arange(43)[None, :] < 20, 0, 1) + np.zeros((24, 1), dtype=np.int64),
                       np.where(np.arange(43)[None, :] < 20, 1, 0) + np.zeros((24, 1), dtype=np.int64)]).astype(np.int32)
    pred = FakeFuser()
    sess = DemoSession(pred, models_dir=str(tmp_path), output_dir=str(tmp_path / "results"), device="cpu")
    srv = serve(sess, "127.0.0.1", 0)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    try:
        port = srv.server_address[1]
        body = {"labels": _b64(labels), "tau": 0.01, "min_points": 1}
        st, out = _req(port, "POST", "/fuse_labels", body)
        assert st == 400 and "before any /frames" in out["error"]
        st, out = _req(port, "POST", "/frames", {"depth": _b64(depth), "rgb": _b64(rgb), "cameras": specs, "far": far, "edge": None})
        assert st == 200
        M = out["num_points"]
        st, out = _req(port, "POST", "/fuse_labels", dict(body, labels=_b64(labels[:, :, :42])))
        assert st == 400 and "2 frames of 24 x 43 need 8256 bytes" in out["error"]
        for bad in ({}, {"labels": _b64(labels)}, {"tau": 0.01}, dict(body, extra=1), dict(body, labels=3), dict(body, labels="not base64!"), dict(body, tau=-1),
                    dict(body, tau="x"), dict(body, overlap=0), dict(body, min_points=0), dict(body, min_votes=0.5), dict(body, consistent=1),
                    dict(body, max_regions=10)):
            st, out = _req(port, "POST", "/fuse_labels", bad)
            assert st == 400 and "error" in out, bad.keys()
        assert pred.fuse_calls == []

        st, out = _req(port, "POST", "/fuse_labels", body)
        assert st == 200
        lab, cfg, consistent = pred.fuse_calls[-1]
        assert np.array_equal(lab, labels) and cfg == FusionConfig(0.01, min_points=1) and consistent is False
        want = FR.fuse(pred.ref["xyz"], pred.ref["cams"], pred.ref["keys"], labels, 0.01, 0.5, 1)
        assert out["labels"] == want["label"].tolist() and len(out["labels"]) == M and out["num_instances"] == want["num_instances"]
        assert out["sizes"] == np.bincount(want["label"][want["label"] >= 0], minlength=want["num_instances"]).tolist() and sum(out["sizes"]) > 0

        st, out = _req(port, "POST", "/fuse_labels", dict(body, consistent=True, min_votes=2, overlap=0.7))
        assert st == 200 and pred.fuse_calls[-1][1:] == (FusionConfig(0.01, overlap=0.7, min_points=1, min_votes=2), True)
        want = FR.vote(pred.ref["xyz"], pred.ref["cams"], pred.ref["keys"], labels, 0.01, min_votes=2)
        assert out["labels"] == want["label"].tolist() and out["num_instances"] == int(want["label"].max()) + 1
        # another cloud drops the frames
        sess.sampled_pointcloud({"points": {str(i): 0.1 * i for i in range(9)}, "colors": {str(i): 0.5 for i in range(9)}})
        st, out = _req(port, "POST", "/fuse_labels", body)
        assert st == 400 and "before any /frames" in out["error"]
    finally:
        srv.shutdown()
