"""Camera views on the device (csrc/views.hip) against the numpy reference (tests/view_reference.py).  Every comparison is exact: keys as int64, bits as
int64, ids and indices as int32."""
import functools

import numpy as np
import pytest
import torch

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


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, copy=True, order="C"))           # a copy: the shared references are read-only
    return (t if dtype is None else t.to(dtype)).cuda()


def _camera(ref):
    from point_sam_amd.views import Camera
    cam = Camera(ref.pose_words.reshape(3, 4), ref.fx, ref.fy, ref.cx, ref.cy, ref.width, ref.height, ref.near)
    assert np.array_equal(cam.pose_words.view(np.uint32), ref.pose_words.view(np.uint32))      # bit for bit, -0.0 included
    return cam


def _keys(ops, pts, ref, s):
    return ops.view_splat(_dev(pts), _camera(ref), s).cpu().numpy().view(np.uint64)


@functools.lru_cache(maxsize=None)
def _sphere():
    return V.sphere_case()


@functools.lru_cache(maxsize=None)
def _sphere_keys(s=1):
    """The reference picture the pick / paint / lift tests share (computed once, never modified)."""
    k = V.splat(_sphere(), V.Cam(), s)
    k.setflags(write=False)
    return k


SMALL = dict(width=37, height=53, fx=45.0, fy=45.0, cx=18.3, cy=26.1)


# ------------------------------------------------------------------------------------------------ splat
@pytest.mark.parametrize("s", [0, 1, 2, 3])
def test_splat_equals_reference_on_the_sphere(ops, s):
    pts = _sphere()
    for ref in (V.Cam(), V.Cam(**SMALL), V.Cam(pose=V.ROTATED), V.Cam(pose=V.ROTATED, **SMALL)):
        want = V.splat(pts, ref, s)
        assert (want != V.EMPTY).mean() > 0.2 and (want == V.EMPTY).any()
        assert np.array_equal(_keys(ops, pts, ref, s), want), (s, ref.width)


@pytest.mark.parametrize("shape", [(1, 1), (1, 64), (64, 1)])
def test_splat_on_degenerate_images(ops, shape):
    pts = _sphere()
    w, h = shape
    ref = V.Cam(width=w, height=h, cx=w / 2, cy=h / 2, fx=30.0, fy=30.0)
    for s in (0, 1, 3):
        want = V.splat(pts, ref, s)
        assert (want != V.EMPTY).any()
        assert np.array_equal(_keys(ops, pts, ref, s), want)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025])
def test_splat_point_counts_around_a_wave_and_a_block(ops, n):
    pts, ref = V.sphere_case(n, seed=n), V.Cam(**SMALL)
    for s in (0, 2):
        want = V.splat(pts, ref, s)
        assert (want != V.EMPTY).any()
        assert np.array_equal(_keys(ops, pts, ref, s), want)


def test_hand_made_border_nan_and_inf_points(ops):
    pts, _ = V.hand_points()
    cases = [(pts, V.Cam())]
    cam, p = V.negzero_case()
    cases.append((p, cam))
    cam, p, _ = V.tiny_case()
    cases.append((p, cam))
    p, cam_in, cam_out = V.near_case()
    cases += [(p, cam_in), (p, cam_out)]
    filled = []
    for p, cam in cases:
        for s in (0, 1):
            want = V.splat(p, cam, s)
            assert np.array_equal(_keys(ops, p, cam, s), want)
        filled.append(int((V.splat(p, cam, 0) != V.EMPTY).sum()))
    assert filled == [3, 1, 1, 1, 0]                       # -0.0 is in pixel 0, near itself is in, one ulp below is out
    # the same points through the lift: in view <=> visible at tau = +large
    pts_d = _dev(pts)
    keys = ops.view_splat(pts_d, _camera(V.Cam()), 0)
    bits, area = ops.view_lift_bits(pts_d, _camera(V.Cam()), keys, None, 1e30)
    want_bits, want_area = V.lift(pts, V.Cam(), V.splat(pts, V.Cam(), 0), None, 1e30)
    assert np.array_equal(bits.cpu().numpy(), want_bits) and area.tolist() == want_area.tolist() == [3]      # the far point on the principal ray is in view but 3e38 behind the winner


def test_ties_and_duplicates_go_to_the_lower_index(ops):
    pts, ref = V.plane_case(), V.Cam()
    for s in (0, 1):
        got = _keys(ops, pts, ref, s)
        assert np.array_equal(got, V.splat(pts, ref, s))
        assert (V.index_of(got)[got != V.EMPTY] < 1600).all()
    # the same cloud with the copies swapped in memory still shows the lower INDEX
    swapped = np.concatenate([pts[1600:], pts[:1600]])
    assert np.array_equal(_keys(ops, swapped, ref, 0), V.splat(pts, ref, 0))


def test_contention_in_one_pixel_and_the_early_out(ops):
    """20 000 points on one ray: far-to-near every atomic wins, near-to-far every later offer should be skipped by the plain load, shuffled is in
    between.  Ordinary contended atomics; all three leave one key, the nearest point's: the same depth word, and as index that point's place in the order."""
    pts, ref = V.ray_case(), V.Cam()
    orders = [np.arange(len(pts))[::-1], np.arange(len(pts)), np.random.default_rng(5).permutation(len(pts))]
    for order in orders:
        p = np.ascontiguousarray(pts[order])
        got = _keys(ops, p, ref, 0)
        assert (got != V.EMPTY).sum() == 1
        key = got[50, 70]
        nearest = int(np.nonzero(order == 0)[0][0])
        assert int(key & np.uint64(0xFFFFFFFF)) == nearest and np.uint32(key >> np.uint64(32)).view(np.float32) == np.float32(1.0)
        assert np.array_equal(got, V.splat(p, ref, 0))
    got = _keys(ops, pts, ref, 3)                          # 49 contended pixels
    assert np.array_equal(got, V.splat(pts, ref, 3)) and (got != V.EMPTY).sum() == 49


def test_footprint_is_clipped_at_corners_and_edges(ops):
    ref = V.Cam()
    W, H = ref.width, ref.height
    pix = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2, H - 1), (0, H // 2), (W - 1, H // 2), (1, 1), (W - 3, H - 2)]
    pts = np.array([[(x + 0.5 - ref.cx) / ref.fx * (1 + 0.1 * i), (y + 0.5 - ref.cy) / ref.fy * (1 + 0.1 * i), (1 + 0.1 * i) - 3] for i, (x, y) in enumerate(pix)],
                   dtype=np.float32)
    ok, px, py, _ = V.project(pts, ref)
    assert ok.all() and list(zip(px.tolist(), py.tolist())) == pix
    for s in (1, 3):
        want = V.splat(pts, ref, s)
        assert np.array_equal(_keys(ops, pts, ref, s), want)
    assert (want != V.EMPTY).sum() < len(pix) * 49         # clipped


def test_two_runs_and_another_stream_give_identical_bits(ops):
    pts, cam = _dev(_sphere()), _camera(V.Cam())
    a = ops.view_splat(pts, cam, 2)
    b = ops.view_splat(pts, cam, 2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = ops.view_splat(pts, cam, 2)
        vis_c, _ = ops.view_lift_bits(pts, cam, c, None, 0.05)
    torch.cuda.current_stream().wait_stream(side)
    vis_a, _ = ops.view_lift_bits(pts, cam, a, None, 0.05)
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(vis_a, vis_c)
    assert np.array_equal(a.cpu().numpy().view(np.uint64), _sphere_keys(2))


# ------------------------------------------------------------------------------------------------ pick
@pytest.mark.parametrize("w", [0, 2, 16])
def test_pick_equals_reference(ops, w):
    ref = V.Cam()
    keys = _sphere_keys(0 if w == 16 else 1)               # the sparse picture has empty pixels inside wide windows too
    keys_d = _dev(keys.view(np.int64))
    corners = [[0, 0], [ref.width - 1, 0], [0, ref.height - 1], [ref.width - 1, ref.height - 1], [-5, -5], [ref.width + 3, 40], [64, 48]]
    rng = np.random.default_rng(11)
    n = 1000
    many = np.concatenate([np.array(corners), np.stack([rng.integers(-4, ref.width + 4, n - len(corners)), rng.integers(-4, ref.height + 4, n - len(corners))], 1)])
    want = V.pick(keys, many, w)
    assert (want >= 0).any() and (want < 0).any()
    got = ops.view_pick(keys_d, _dev(many, torch.int32), w)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    one = ops.view_pick(keys_d, _dev(np.array([[64, 48]]), torch.int32), w)
    assert one.tolist() == V.pick(keys, [[64, 48]], w).tolist() and one[0] >= 0


def test_pick_ties_in_distance_go_to_the_key(ops):
    keys = np.full((9, 9), V.EMPTY, dtype=np.uint64)
    k = lambda depth, i: (np.uint64(np.float32(depth).view(np.uint32)) << np.uint64(32)) | np.uint64(i)
    keys[4, 4], keys[4, 6], keys[2, 4] = k(2.0, 7), k(1.0, 3), k(1.5, 5)
    clicks = np.array([[4, 4], [5, 3], [4, 3], [5, 4], [0, 8], [-3, 4], [4, -10]])
    for w in (0, 1, 2, 16):
        got = ops.view_pick(_dev(keys.view(np.int64)), _dev(clicks, torch.int32), w)
        assert np.array_equal(got.cpu().numpy(), V.pick(keys, clicks, w)), w
    assert got.tolist() == [7, 3, 5, 3, 7, 7, 5]


# ------------------------------------------------------------------------------------------------ paint
@pytest.mark.parametrize("K", [1, 3, 65])
def test_paint_equals_reference(ops, K):
    keys, N = _sphere_keys(1), len(_sphere())
    assert (keys == V.EMPTY).any()                         # an image with empty pixels
    zero, one = ((), ()) if K == 1 else ((0, K - 1), (1,))
    bits = V.random_bits(K, N, seed=K, zero_rows=zero, one_rows=one)
    keys_d, bits_d = _dev(keys.view(np.int64)), _dev(bits)
    ids, rows = ops.view_paint_ids(keys_d, bits_d, N), ops.view_paint_rows(keys_d, bits_d, N)
    assert ids.dtype == torch.int32 and rows.dtype == torch.uint8 and rows.shape == (K,) + keys.shape
    want_rows = V.paint_rows(keys, bits, N)
    assert np.array_equal(rows.cpu().numpy(), want_rows) and np.array_equal(ids.cpu().numpy(), V.paint_ids(keys, bits, N))
    if K > 1:
        assert not want_rows[0].any() and (want_rows[1].astype(bool) == (keys != V.EMPTY)).all()
        assert set(np.unique(ids.cpu().numpy())) == {-1, 1}            # row 0 is empty, row 1 holds every point: the lowest set row is 1
    for all_zero in (True, False):                                      # every row zeros / every row ones
        b = _dev(V.pack(np.full((K, N), not all_zero)))
        i = ops.view_paint_ids(keys_d, b, N).cpu().numpy()
        assert np.array_equal(i, np.where((keys == V.EMPTY) | all_zero, -1, 0))


def test_paint_with_keys_of_a_larger_cloud_is_a_wrong_answer_not_a_wild_load(ops):
    keys, N = _sphere_keys(1), 1000                        # indices up to 19 999 against masks of 1000 points
    bits = V.random_bits(3, N, seed=2)
    ids = ops.view_paint_ids(_dev(keys.view(np.int64)), _dev(bits), N)
    rows = ops.view_paint_rows(_dev(keys.view(np.int64)), _dev(bits), N)
    assert np.array_equal(ids.cpu().numpy(), V.paint_ids(keys, bits, N)) and np.array_equal(rows.cpu().numpy(), V.paint_rows(keys, bits, N))
    assert (ids.cpu().numpy()[V.index_of(keys) >= N] == -1).all()


# ------------------------------------------------------------------------------------------------ lift
@pytest.mark.parametrize("n", [63, 64, 65, 20000])
def test_lift_equals_reference(ops, n):
    pts, ref = V.sphere_case(n), V.Cam()
    keys = V.splat(pts, ref, 1)
    pts_d, keys_d, cam = _dev(pts), _dev(keys.view(np.int64)), _camera(ref)
    rng = np.random.default_rng(n)
    for K in (None, 1, 3, 9):
        img = None if K is None else (rng.random((K,) + keys.shape) < 0.5).astype(np.uint8) * rng.integers(1, 255, (K,) + keys.shape, dtype=np.uint8)
        for tau in (0.0, 0.05, 1e30):
            bits, area = ops.view_lift_bits(pts_d, cam, keys_d, None if img is None else _dev(img), tau)
            want_bits, want_area = V.lift(pts, ref, keys, img, tau)
            assert bits.dtype == torch.int64 and bits.shape == (K or 1, (n + 63) // 64) and area.dtype == torch.int32
            assert np.array_equal(bits.cpu().numpy(), want_bits), (K, tau)
            assert np.array_equal(area.cpu().numpy(), want_area) and area.tolist() == [int(v) for v in V.unpack(want_bits, n).sum(1)]
    vis = V.unpack(V.lift(pts, ref, keys, None, 0.0)[0], n)[0]
    assert vis.any() and not vis.all()


def test_round_trip_paint_then_lift(ops):
    """s = 0, tau = 0: lifting the painted image of row k gives a subset of row k that holds every winner whose bit was set."""
    pts, ref = _sphere(), V.Cam()
    N = len(pts)
    pts_d, cam = _dev(pts), _camera(ref)
    keys_d = ops.view_splat(pts_d, cam, 0)
    bits = V.random_bits(4, N, seed=9, one_rows=(3,))
    rows = ops.view_paint_rows(keys_d, _dev(bits), N)
    lifted, area = ops.view_lift_bits(pts_d, cam, keys_d, rows, 0.0)
    m, src = V.unpack(lifted.cpu().numpy(), N), V.unpack(bits, N)
    assert (m <= src).all() and area.tolist() == m.sum(1).tolist()
    keys = keys_d.cpu().numpy().view(np.uint64)
    win = V.index_of(keys)[keys != V.EMPTY]
    for k in range(4):
        assert m[k][win[src[k][win]]].all() and m[k].sum() >= src[k][win].sum() > 0


# ------------------------------------------------------------------------------------------------ the predictor
@pytest.fixture(scope="module")
def scene(ops):
    from point_sam_amd.model import PointCloudSAM
    from point_sam_amd.predictor import PointSAMPredictor
    cfg = get_config("tiny")
    pred = PointSAMPredictor(PointCloudSAM(cfg, random_state_dict(cfg, 3), "cuda", precision="f16x3"))
    xyz = _dev(_sphere())
    rgb = torch.rand(len(xyz), 3, generator=torch.Generator().manual_seed(7)).cuda()      # its own generator: the same colours whatever ran before
    pred.set_scene(xyz, rgb, max_points=2048)
    assert not pred.scene.identity
    return pred, xyz, rgb


def test_predictor_views_of_a_scene(ops, scene):
    from point_sam_amd.views import View
    pred, xyz, rgb = scene
    cam = _camera(V.Cam())
    view = pred.render_view(cam)
    assert isinstance(view, View) and view.num_points == len(xyz) and view.splat == 1
    assert np.array_equal(view.keys.cpu().numpy().view(np.uint64), _sphere_keys(1))
    assert np.array_equal(view.index.cpu().numpy(), V.index_of(_sphere_keys(1))) and np.array_equal(view.depth.cpu().numpy(), V.depth_of(_sphere_keys(1)))
    img = view.colour(rgb, 0.5)
    full = view.index >= 0
    assert img.shape == (96, 128, 3) and torch.equal(img[full], rgb[view.index[full].long()]) and (img[~full] == 0.5).all()
    # pixel clicks are point prompts: bit for bit what the picked points' coordinates give
    pixels = [[64, 48], [50, 40]]
    idx, picked = pred.pick(view, pixels)
    assert idx.tolist() == V.pick(_sphere_keys(1), pixels, 2).tolist() and torch.equal(picked, xyz[idx.long()])
    pts, lab = pred.click_pixels(view, pixels, [1, 0])
    assert pts.shape == (1, 2, 3) and lab.shape == (1, 2) and torch.equal(pts[0], picked)
    a = pred.predict_masks(pts, lab, None, True)
    b = pred.predict_masks(picked[None].clone(), torch.tensor([[1, 0]], device="cuda"), None, True)
    assert a[0].shape[-1] == len(xyz) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError, match=r"\(0, 0\)"):
        pred.click_pixels(view, [[64, 48], [0, 0]], [1, 1], window=0)
    idx, nowhere = pred.pick(view, [[0, 0]], window=0)
    assert idx.tolist() == [-1] and torch.isnan(nowhere).all()
    # masks as images
    bits, area, _ = pred.predict_mask_bits(pts, lab, None, True)
    again = pred.predict_mask_bits(pts, lab, None, True)
    assert torch.equal(again[0], bits) and torch.equal(again[1], area), "the same scene and prompts: the same masks, run after run"
    K = bits.shape[0]
    ids = pred.mask_images(view, bits)
    rows = pred.mask_images(view, bits, rows=True)
    assert ids.shape == (96, 128) and ids.dtype == torch.int32 and int(ids.min()) >= -1 and int(ids.max()) < K
    assert rows.shape == (K, 96, 128) and np.array_equal(ids.cpu().numpy(), V.paint_ids(_sphere_keys(1), bits.cpu().numpy(), len(xyz)))
    # and back
    lifted, larea = pred.lift_masks(view, rows, 0.05)
    vis, varea = pred.visible_bits(view, 0.05)
    # a visible point takes the row's value at its own pixel, whatever its own bit was: a point near the front one that won the pixel is lifted too
    want_lifted, want_larea = V.lift(_sphere(), V.Cam(), _sphere_keys(1), rows.cpu().numpy(), 0.05)
    assert np.array_equal(lifted.cpu().numpy(), want_lifted) and larea.tolist() == want_larea.tolist()
    assert torch.equal(lifted & ~vis, torch.zeros_like(bits))
    want_vis, want_area = V.lift(_sphere(), V.Cam(), _sphere_keys(1), None, 0.05)
    assert np.array_equal(vis.cpu().numpy(), want_vis) and varea.tolist() == want_area.tolist()
    assert torch.equal(pred.lift_masks(view, rows[0].bool(), 0.05)[0], lifted[:1])


def test_predictor_view_under_a_crop_and_foreign_views(ops, scene):
    from point_sam_amd.views import View
    pred, xyz, rgb = scene
    cam = _camera(V.Cam())
    pred.set_crop((0.0, 0.0, -0.8), 0.4)
    try:
        assert pred.crop is not None and pred.crop.num_members < len(xyz)
        view = pred.render_view(cam)                       # still the scan's picture
        assert view.num_points == len(xyz) and np.array_equal(view.keys.cpu().numpy().view(np.uint64), _sphere_keys(1))
        pts, lab = pred.click_pixels(view, [[64, 48]], [1])                # the pixel shows the sphere's near pole, inside the ball
        logits = pred.predict_masks(pts, lab, None, True)[0]
        assert logits.shape[-1] == len(xyz) and torch.isinf(logits[0, 0]).any()
    finally:
        pred.clear_crop()
    foreign = View(view.keys, cam, len(xyz) - 1)
    for call in (lambda: pred.pick(foreign, [[1, 1]]), lambda: pred.click_pixels(foreign, [[1, 1]], [1]), lambda: pred.visible_bits(foreign, 0.0),
                 lambda: pred.mask_images(foreign, torch.zeros(1, (len(xyz) + 63) // 64, dtype=torch.int64, device="cuda"))):
        with pytest.raises(ValueError, match=f"{len(xyz) - 1} points.*{len(xyz)}"):
            call()


def test_predictor_view_of_a_batch_cloud(ops):
    from point_sam_amd.model import PointCloudSAM
    from point_sam_amd.predictor import PointSAMPredictor
    cfg = get_config("tiny")
    pred = PointSAMPredictor(PointCloudSAM(cfg, random_state_dict(cfg, 3), "cuda", precision="f16x3"))
    a, b = V.sphere_case(1024, seed=1), V.sphere_case(1024, seed=2)
    xyz = _dev(np.stack([a, b]))
    pred.set_pointcloud(xyz, torch.full_like(xyz, 0.5))
    ref = V.Cam(**SMALL)
    for c, pts in enumerate((a, b)):
        view = pred.render_view(_camera(ref), splat=2, cloud=c)
        assert view.cloud == c and np.array_equal(view.keys.cpu().numpy().view(np.uint64), V.splat(pts, ref, 2))
        idx, picked = pred.pick(view, [[18, 26]])
        assert idx[0] >= 0 and torch.equal(picked[0], xyz[c, int(idx[0])])
