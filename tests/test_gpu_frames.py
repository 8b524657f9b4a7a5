"""RGB-D frames on the device (csrc/frames.hip) against the numpy reference (tests/frames_reference.py).  Every comparison is exact: coordinates and
colours as their 32-bit words, index as int32, keys as int64, M as an integer."""
import functools

import numpy as np
import pytest
import torch

import frames_reference as R
import view_reference as V
from point_sam_amd.config import get_config
from point_sam_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()      # a copy: the shared references are read-only


def _camera(ref):
    from point_sam_amd.views import Camera
    cam = Camera(ref.pose_words.reshape(3, 4), ref.fx, ref.fy, ref.cx, ref.cy, ref.width, ref.height, ref.near)
    assert np.array_equal(cam.pose_words.view(np.uint32), ref.pose_words.view(np.uint32))
    return cam


def _same_words(t, want):
    got = t.cpu().numpy()
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _check(ops, depth, rgb, cams, far, edge=None, depth_scale=None, center=None, scale=None, want=None):
    """Both calls against the reference, every output exactly.  center / scale None: the reference's automatic ones.  -> the reference's dict."""
    if want is None:
        want = R.frames(depth, rgb, cams, far, edge, depth_scale, center, scale)
    cameras = [_camera(c) for c in cams]
    world, col, index, M = ops.frames_unproject(_dev(depth), _dev(rgb), cameras, far, edge, depth_scale)
    assert M == want["M"] and isinstance(M, int) and world.shape == (M, 3) and col.shape == (M, 3) and world.is_contiguous() and col.is_contiguous()
    assert index.dtype == torch.int32 and np.array_equal(index.cpu().numpy(), want["index"])
    assert _same_words(world, want["world"]), "xyz before normalisation"
    assert _same_words(col, want["rgb"]), "rgb"
    xyz, keys, ncams = ops.frames_finish(world, index, cameras, want["center"], float(want["scale"]))
    assert xyz.data_ptr() == world.data_ptr()               # in place
    assert _same_words(xyz, want["xyz"]), "xyz after normalisation"
    assert keys.dtype == torch.int64 and np.array_equal(keys.cpu().numpy().view(np.uint64), want["keys"])
    for got, ref in zip(ncams, want["cams"]):
        assert np.array_equal(got.pose_words.view(np.uint32), ref.pose_words.view(np.uint32)) and got.near == ref.near
        assert (got.fx, got.fy, got.cx, got.cy, got.width, got.height) == (ref.fx, ref.fy, ref.cx, ref.cy, ref.width, ref.height)
    return want


@functools.lru_cache(maxsize=None)
def _room(edge):
    """The reference of the room fixture, computed once per edge setting and never modified."""
    depth, rgb, cams, far = R.room_case()
    out = R.frames(depth, rgb, cams, far, edge)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 64), (1, 64, 1), (3, 5, 13), (1, 1, 63), (1, 1, 65), (1, 1, 1023), (1, 1, 1024), (1, 1, 1025), (2, 24, 43)])
@pytest.mark.parametrize("edge", [None, 0.25])
def test_small_shapes_equal_the_reference(ops, shape, edge):
    """A wave's and a block's edge as (1, 1, n); (2, 24, 43): 2064 pixels, a row end, a frame end and a block end all inside the images -- the edge
    filter must not look across a row end or into the next frame (the pattern has jumps at every seventh pixel, so it would show)."""
    depth, rgb, cams, far = R.pattern_case(*shape, seed=sum(shape))
    out = _check(ops, depth, rgb, cams, far, edge)
    assert 1 <= out["M"] <= depth.size
    if edge is not None and depth.size > 1000:
        assert out["M"] < R.unproject(depth, rgb, cams, far, None)[3]                # the filter drops something


def test_more_than_1024_blocks(ops):
    """(5, 512, 512) is 1280 blocks of 1024 pixels: the second-level scan's spans hold more than one block."""
    depth, rgb, cams, far = R.pattern_case(5, 512, 512, seed=5)
    out = _check(ops, depth, rgb, cams, far, 0.25)
    assert 0.3 * depth.size < out["M"] < 0.9 * depth.size


def test_kept_fractions_none_all_every_other_and_a_dead_frame(ops):
    shape = (3, 17, 70)                                    # 3570 pixels: four blocks, frames that end inside a wave
    depth, rgb, cams, far = R.pattern_case(*shape, seed=1)
    cameras = [_camera(c) for c in cams]
    with pytest.raises(ValueError, match="no pixel"):
        ops.frames_unproject(_dev(np.zeros(shape, dtype=np.float32)), _dev(rgb), cameras, far)
    with pytest.raises(ValueError, match="no pixel"):
        ops.frames_unproject(_dev(np.full(shape, np.nan, dtype=np.float32)), _dev(rgb), cameras, far, 0.25)
    out = _check(ops, np.full(shape, 1.5, dtype=np.float32), rgb, cams, far, 0.25)
    assert out["M"] == 3570 and np.array_equal(out["index"].reshape(-1), np.arange(3570))
    depth, rgb, cams, far = R.pattern_case(*shape, seed=2, every_other=True)
    out = _check(ops, depth, rgb, cams, far, 0.25)
    assert not (out["index"].reshape(-1)[1::2] >= 0).any() and out["M"] > 500
    depth, rgb, cams, far = R.pattern_case(*shape, seed=3, dead_frame=1)
    out = _check(ops, depth, rgb, cams, far, None)
    assert (out["index"][1] == -1).all() and out["index"][2].min() == -1 and out["index"][2].max() == out["M"] - 1 and (out["keys"][1] == R.EMPTY).all()


def test_hand_made_frame_nan_inf_range_ends_and_the_exact_edge(ops):
    depth, rgb, cams, far, edge, keep = R.hand_case()
    out = _check(ops, depth, rgb, cams, far, edge)
    assert np.array_equal(out["index"] >= 0, keep)
    out = _check(ops, depth, rgb, cams, far, None)
    assert out["M"] == int(keep[:3].sum()) + 8
    # the same rules on 16-bit depth: raw 0, raw 65535, and scales that put a value exactly on near and on far
    raw = np.array([[[0, 1, 8, 9, 65535, 2, 7, 3]]], dtype=np.uint16)
    cam = [V.Cam(fx=6.0, fy=6.0, cx=4.0, cy=0.5, width=8, height=1, near=0.5)]
    out = _check(ops, raw, rgb[:1], cam, 4.0, None, 0.5)
    assert (out["index"].reshape(-1) >= 0).tolist() == [False, True, True, False, False, True, True, True]
    out = _check(ops, raw, rgb[:1], cam, 4.0, 0.25, 2.0 ** -14)
    assert (out["index"].reshape(-1) >= 0).tolist() == [False, False, False, False, True, False, False, False]


# ------------------------------------------------------------------------------------------------ the room
@pytest.mark.parametrize("edge", [None, 0.05])
@pytest.mark.parametrize("u16", [False, True], ids=["depth_f32", "depth_u16"])
@pytest.mark.parametrize("u8", [True, False], ids=["rgb_u8", "rgb_f32"])
def test_room_fixture(ops, edge, u16, u8):
    depth, rgb, cams, far = R.room_case()
    scale = None
    if u16:
        depth, scale = R.room_case_u16()
    if not u8:
        rgb = R.colours(rgb)
    want = None if u16 else _room(edge)                  # the colours are the same numbers either way; millimetre depth is its own reference
    out = _check(ops, depth, rgb, cams, far, edge, scale, want=want)
    assert out["M"] == (R.ROOM_KEPT if edge is None else R.ROOM_KEPT_EDGE)


def test_two_runs_and_another_stream_give_identical_bits(ops):
    depth, rgb, cams, far = R.room_case()
    want = _room(0.05)
    d, c, cameras = _dev(depth), _dev(rgb), [_camera(v) for v in cams]

    def run():
        world, col, index, M = ops.frames_unproject(d, c, cameras, far, 0.05)
        world_words = world.clone()
        xyz, keys, _ = ops.frames_finish(world, index, cameras, want["center"], float(want["scale"]))
        return world_words, col, index, xyz, keys

    a, b = run(), run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s = run()
    torch.cuda.current_stream().wait_stream(side)
    for x, y, z in zip(a, b, s):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, z.view(torch.int32) if z.dtype == torch.float32 else z)
    assert np.array_equal(s[4].cpu().numpy().view(np.uint64), want["keys"])


# ------------------------------------------------------------------------------------------------ the predictor
@pytest.fixture(scope="module")
def frames(ops):
    from point_sam_amd.model import PointCloudSAM
    from point_sam_amd.predictor import PointSAMPredictor
    cfg = get_config("tiny")
    pred = PointSAMPredictor(PointCloudSAM(cfg, random_state_dict(cfg, 3), "cuda", precision="f16x3"))
    depth, rgb, cams, far = R.room_case()
    cameras = [_camera(c) for c in cams]
    fs = pred.set_frames(depth, rgb, cameras, far, edge=0.05, max_points=2048)
    assert not pred.scene.identity and pred.scene.num_working <= 2048           # a voxel working cloud
    return pred, fs, cameras


def test_set_frames_normalisation_and_outputs(ops, frames):
    from point_sam_amd.views import FrameSet
    pred, fs, cameras = frames
    depth, rgb, cams, far = R.room_case()
    assert isinstance(fs, FrameSet) and fs.num_points == R.ROOM_KEPT_EDGE and len(fs.views) == 2
    # the automatic centre and scale against numpy's fp64 values; with them passed back in, everything is exact
    world = R.unproject(depth, rgb, cams, far, 0.05)[0].astype(np.float64)
    mean = world.mean(0)
    radius = np.sqrt(((world - mean) ** 2).sum(1).max())
    assert np.abs(np.array(fs.center) - mean).max() <= 1e-6 * np.abs(mean).max() and abs(fs.scale - radius) <= 1e-6 * radius
    want = R.frames(depth, rgb, cams, far, 0.05, None, np.array(fs.center, dtype=np.float32), np.float32(fs.scale))
    assert _same_words(fs.xyz, want["xyz"]) and _same_words(fs.rgb, want["rgb"]) and np.array_equal(fs.index.cpu().numpy(), want["index"])
    assert np.array_equal(fs.keys.cpu().numpy().view(np.uint64), want["keys"])
    for f, view in enumerate(fs.views):
        assert view.splat == 0 and view.num_points == fs.num_points and torch.equal(view.keys, fs.keys[f]) and torch.equal(view.index, fs.index[f])
        assert np.array_equal(view.camera.pose_words.view(np.uint32), want["cams"][f].pose_words.view(np.uint32)) and view.camera.near == want["cams"][f].near
    # the next batch of frames, normalised identically
    again = pred.set_frames(_dev(depth), _dev(rgb), cameras, far, edge=0.05, center=fs.center, scale=fs.scale, max_points=2048)
    assert again.center == fs.center and again.scale == fs.scale and torch.equal(again.xyz.view(torch.int32), fs.xyz.view(torch.int32))
    assert torch.equal(again.keys, fs.keys)
    mm, step = R.room_case_u16()
    third = pred.set_frames(mm, rgb, cameras, far, edge=0.05, depth_scale=step, center=fs.center, scale=fs.scale, max_points=2048)
    assert third.num_points == R.ROOM_KEPT_EDGE and torch.equal(third.index, fs.index)
    pred.set_frames(_dev(depth), _dev(rgb), cameras, far, edge=0.05, center=fs.center, scale=fs.scale, max_points=2048)      # leave the first scan loaded
    with pytest.raises(ValueError, match="no pixel"):
        pred.set_frames(np.zeros_like(depth), rgb, cameras, far, max_points=2048)


def test_frames_are_views_of_the_scan(ops, frames):
    pred, fs, cameras = frames
    pred.set_scene(fs.xyz, fs.rgb, max_points=2048)
    M = fs.num_points
    index = fs.index.cpu().numpy()
    # a click on the photograph is a click on the pixel's own point
    own = int(index[0, 45, 60])
    assert own >= 0
    pts, lab = pred.click_pixels(fs.views[0], [[60, 45]], [1])
    assert pts.shape == (1, 1, 3) and torch.equal(pts[0, 0], fs.xyz[own])
    idx, _ = pred.pick(fs.views[1], [[60, 45], [10, 10], [0, 0]], window=0)
    assert idx.tolist() == [int(index[1, 45, 60]), -1, -1]                    # the NaN pixel and the zero rows show nothing
    a = pred.predict_masks(pts, lab, None, True)
    b = pred.predict_masks(fs.xyz[own][None, None].clone(), torch.tensor([[1]], device="cuda"), None, True)
    assert a[0].shape[-1] == M and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # masks as images of each photograph: the bits gathered through the frame's index
    bits, _, _ = pred.predict_mask_bits(pts, lab, None, True)
    member = V.unpack(bits.cpu().numpy(), M)
    for f in range(2):
        has = index[f] >= 0
        gathered = member[:, np.where(has, index[f], 0)] & has[None]
        rows = pred.mask_images(fs.views[f], bits, rows=True).cpu().numpy()
        ids = pred.mask_images(fs.views[f], bits).cpu().numpy()
        assert np.array_equal(rows, gathered.astype(np.uint8))
        assert np.array_equal(ids, np.where(gathered.any(0), gathered.argmax(0), -1)) and (ids[~has] == -1).all()
    # an image mask drawn on photograph 0 reaches the points of both frames: all of its own under the mask, frame 1's where the measured depth lets them
    img = np.zeros((96, 128), dtype=np.uint8)
    img[35:55, 45:85] = 1
    xyz, keys = fs.xyz.cpu().numpy(), fs.keys.cpu().numpy().view(np.uint64)
    ref_cam = V.Cam(pose=fs.views[0].camera.pose, near=fs.views[0].camera.near)
    for tau in (0.0, 0.02, 1e30):
        lifted, area = pred.lift_masks(fs.views[0], _dev(img), tau)
        want_bits, want_area = V.lift(xyz, ref_cam, keys[0], img[None], tau)
        assert np.array_equal(lifted.cpu().numpy(), want_bits) and area.tolist() == want_area.tolist()
        on = V.unpack(lifted.cpu().numpy(), M)[0]
        under = index[0][(img > 0) & (index[0] >= 0)]
        assert len(under) == 20 * 40 and on[under].all()
        first = int((index[0] >= 0).sum())
        assert not on[:first][np.setdiff1d(np.arange(first), under)].any()       # of frame 0, nothing but the pixels under the mask
        # frame 1's points that fall under the mask lie far behind the surface frame 0 measured: only a depth test that lets everything pass sets them
        assert on[first:].any() == (tau == 1e30)
    vis, varea = pred.visible_bits(fs.views[1], 0.0)
    seen = V.unpack(vis.cpu().numpy(), M)[0]
    assert seen[first:].all() and int(varea[0]) == int(seen.sum())             # every pixel's own point is visible at tau = 0
