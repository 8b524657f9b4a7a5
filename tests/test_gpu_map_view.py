"""Scan map views on the GPU (csrc/map_view.hip, ScanMap.view, ScanMap.label_image, predictor.map_view) against tests/map_view_reference.py.  Every
comparison is exact: torch.equal on the int64 keys.  The count of visited cells that the kernel can report is compared with the reference's lists, so
the WALK is checked, not only where it ends; the forms of the kernel that the measurement switches select give the same words."""
import numpy as np
import pytest
import torch

import carve_reference as CR
import map_view_reference as R
import scanmap_reference as SM

pytestmark = pytest.mark.gpu
f32 = np.float32
H3 = 2.0 ** -3


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd import scanmap
    return scanmap


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _centre(cell, h):
    return (np.asarray(cell, dtype=np.float64) + 0.5) * h - 1.0


class Pair:
    """A device map beside its reference."""

    def __init__(self, S, h, max_voxels):
        self.h = h
        self.m, self.ref = S.ScanMap(h, max_voxels), SM.RefMap(h, max_voxels)

    def add(self, xyz, rgb=None, labels=None):
        xyz = np.ascontiguousarray(xyz, dtype=f32)
        rgb = np.zeros_like(xyz) if rgb is None else rgb
        res = self.m.add(_dev(xyz), _dev(rgb), None if labels is None else _dev(labels.astype(np.int32)))
        want = self.ref.add(xyz, rgb, labels)
        assert np.array_equal(res.ids.cpu().numpy(), want[0]) and self.m.num_voxels == self.ref.V
        return want[0]

    def check(self, cam, occupied=None, min_count=1, forms=True):
        """One view on both sides -> (the View, the reference's keys, its visited cells).  The keys are equal; so is the number of visited cells; the
        forms without the brick gate and without its staging give the same words."""
        from point_sam_amd import ops
        skip = None if occupied is None else ~occupied
        want, visited = R.view(self.ref, cam, skip, min_count)
        view = self.m.view(cam, None if occupied is None else _dev(occupied), min_count)
        assert view.keys.dtype == torch.int64 and tuple(view.keys.shape) == (cam.height, cam.width) and view.num_points == self.ref.V and view.splat == 0
        assert torch.equal(view.keys.cpu(), torch.from_numpy(want))
        if forms:
            crossed = sum(len(c) for c in visited.values())
            row = None if occupied is None else self.m._skip("view", _dev(occupied), self.ref.V)
            lead = (self.m._block, self.m.max_voxels, self.m.max_pairs, self.ref.V, cam, row, min_count)
            seen = []
            for flags in (0, ops.MAP_VIEW_NO_LDS, ops.MAP_VIEW_NO_GATE, ops.MAP_VIEW_NO_GATE | ops.MAP_VIEW_NO_LDS):
                stats = torch.zeros(2, dtype=torch.int64, device="cuda")
                assert torch.equal(ops.map_view(*lead, voxel_size=self.h, flags=flags, stats=stats), view.keys), flags
                seen.append(stats.tolist())
            assert [s[0] for s in seen] == [crossed] * 4, "the gate skips a lookup, never a step"
            assert seen[2][1] == seen[3][1] == crossed and seen[0][1] == seen[1][1] <= crossed
        return view, want, visited


def _box_points(lo=2, hi=14, seed=3):
    """One jittered point in every cell of the shell of the cube of cells lo .. hi, in a seeded order."""
    g = np.random.default_rng(seed)
    r = range(lo, hi + 1)
    cells = np.array([(x, y, z) for x in r for y in r for z in r if lo in (x, y, z) or hi in (x, y, z)])
    cells = cells[g.permutation(len(cells))]
    return ((cells + g.uniform(0.2, 0.8, cells.shape)) * H3 - 1.0).astype(f32)


@pytest.fixture(scope="module")
def box(S):
    p = Pair(S, H3, 2048)
    pts = _box_points()
    g = np.random.default_rng(4)
    p.add(pts, g.uniform(0.1, 1.0, pts.shape).astype(f32), (pts[:, 2] > 0).astype(np.int64) + (pts[:, 0] > 0.3))
    assert p.ref.V == 13 ** 3 - 11 ** 3
    return p


def _look(eye, target, width, height, fov=80.0, near=1e-3):
    from point_sam_amd.views import Camera
    return Camera.look_at(eye, target, (0.0, 0.0, 1.0), fov, width, height, near)


# ------------------------------------------------------------------------------------------------ the cases of the definition
def test_hollow_box_from_its_centre_every_pixel_hits(box):
    cam = _look(_centre((8, 8, 8), H3), (0.7, 0.3, 0.2), 16, 12)
    view, want, visited = box.check(cam)
    assert (want != R.EMPTY).all() and min(len(c) for c in visited.values()) >= 5
    xyz = box.m.cloud()[0].cpu().numpy()
    assert np.array_equal(xyz, box.ref.cloud()[0])
    w = cam.pose_words
    idx = view.index.cpu().numpy()
    p = xyz[idx]
    depth = ((w[8] * p[..., 0] + w[9] * p[..., 1]) + w[10] * p[..., 2]) + w[11]
    assert depth.dtype == f32 and np.array_equal(view.depth.cpu().numpy().view(np.uint32), depth.view(np.uint32))
    assert idx.min() >= 0 and idx.max() < box.ref.V


def test_corner_cell_looking_outwards_is_empty(box):
    cam = _look(_centre((0, 0, 0), H3), (-2.0, -2.0, -2.0), 16, 12, fov=40.0)
    _, want, visited = box.check(cam)
    assert (want == R.EMPTY).all() and max(len(c) for c in visited.values()) <= 3
    out = _look((1.0, -0.9375, 1.0), (2.0, -2.0, 2.0), 8, 8, fov=40.0)             # the eye at +1 on two axes: their last cell, 16
    assert (box.check(out)[1] == R.EMPTY).all()


def test_axis_aligned_and_tied_diagonal_rays(S):
    p = Pair(S, H3, 64)
    on_axis, on_diagonal, beside = (8, 8, 11), (9, 9, 8), (6, 5, 8)
    ids = p.add(np.array([_centre(c, H3) for c in (on_axis, on_diagonal, beside)]))
    cam = R.axis_camera(_centre((8, 8, 4), H3), 5, 5, 4.0, 2.5, 2.5)
    assert R.directions(cam)[0][2, 2].tolist() == [0, 0, 1 << 21]
    view, want, visited = p.check(cam)
    assert int(view.index[2, 2]) == ids[0] and visited[(2, 2)] == [(8, 8, z) for z in range(5, 12)], "two axes never move"
    cam = R.diagonal_camera(_centre((3, 3, 8), H3), 5, 5, 4.0, 2.5, 2.5)
    assert R.directions(cam)[0][2, 2].tolist() == [1 << 21, 1 << 21, 0] and R.eye_cell(R.eye_of(cam.pose_words), p.ref.inv_h) == (3, 3, 8)
    view, want, visited = p.check(cam)
    assert visited[(2, 2)] == [(k, k, 8) for k in range(4, 10)], "tied axes step together: the cells beside the diagonal are touched, not crossed"
    assert int(view.index[2, 2]) == ids[1] and beside not in visited[(2, 2)]


def test_voxels_that_are_passed_through(S):
    p = Pair(S, H3, 64)
    pts = np.array([_centre(c, H3) for c in ((8, 8, 12), (8, 8, 14), (8, 8, 8), (8, 8, 9))], dtype=f32)
    pts[3, 2] = (9 * H3 - 1.0) + 1e-4                               # in the cell next to the eye's, 0.0626 from the eye: in front of a near of 0.1
    p.add(pts)
    p.add(pts[1:2])                                                 # voxel 1 has two observations
    eye = _centre((8, 8, 8), H3)
    cam = R.axis_camera(eye, 3, 3, 1.0, 1.5, 1.5, near=0.1)
    at = lambda view: int(view.index[1, 1])
    view, _, visited = p.check(cam)
    assert at(view) == 0 and visited[(1, 1)][0] == (8, 8, 9), "the eye's own cell holds voxel 2 and is no candidate; voxel 3 lies in front of near"
    assert at(p.check(cam, occupied=np.array([False, True, True, True]))[0]) == 1, "a skipped voxel is seen through"
    assert at(p.check(cam, min_count=2)[0]) == 1, "a voxel with one observation is seen through at min_count = 2"
    assert at(p.check(R.axis_camera(eye, 3, 3, 1.0, 1.5, 1.5, near=1e-3))[0]) == 3
    assert at(p.check(cam, occupied=np.zeros(4, dtype=bool))[0]) == -1


@pytest.mark.parametrize("width, height", [(13, 7), (1, 1), (9, 1), (17, 19)])
def test_image_sides_that_are_no_multiple_of_the_tile(box, width, height):
    _, want, _ = box.check(_look(_centre((5, 9, 7), H3) + 0.01, (-0.4, 0.9, 0.1), width, height, fov=70.0))
    assert (want != R.EMPTY).all()


def test_a_long_walk_to_the_far_corner(S):
    h = 2.0 ** -10
    p = Pair(S, h, 64)
    far, eye = (2040, 2040, 2040), (10, 10, 10)
    p.add(np.array([_centre(far, h), _centre((2040, 2040, 100), h), _centre((100, 2040, 2040), h)]))
    cam = _look(_centre(eye, h), _centre(far, h), 3, 3, fov=10.0)
    assert R.cmax_of(p.ref.inv_h) == 2048
    view, want, visited = p.check(cam)
    assert int(view.index[1, 1]) == 0 and visited[(1, 1)][-1] == far and len(visited[(1, 1)]) > 2000
    others = np.delete(want.reshape(-1), 4)
    assert (others == R.EMPTY).all() and min(len(c) for k, c in visited.items() if k != (1, 1)) > 1000, "its neighbours leave the grid empty-handed"


def test_a_bitmap_past_any_lds_budget(S):
    h = 2.0 ** -12
    p = Pair(S, h, 64)
    cells = [(100, 100, 5000), (101, 100, 4995), (100, 99, 5001), (100, 100, 7000), (3000, 3000, 3000)]
    p.add(np.array([_centre(c, h) for c in cells]))
    cam = R.axis_camera(_centre((100, 100, 100), h), 1, 1, 1.0, 0.5, 0.5)
    view, _, visited = p.check(cam)
    assert int(view.index[0, 0]) == 0 and len(visited[(0, 0)]) == 4900
    assert int(p.check(cam, occupied=np.array([False, True, True, True, True]))[0].index[0, 0]) == 3


def test_a_table_with_displaced_keys_seen_from_random_poses(S):
    h = 2.0 ** -5
    g = np.random.default_rng(11)
    d = g.normal(size=(12000, 3))
    pts = np.concatenate([0.7 * d / np.linalg.norm(d, axis=1, keepdims=True), g.uniform(-0.6, 0.6, (1000, 3))]).astype(f32)
    p = Pair(S, h, 16384)
    p.add(pts[:7000])
    p.add(pts[5000:])
    keys = p.m.keys().cpu().numpy()
    assert np.array_equal(keys, np.asarray(p.ref.keys, dtype=np.int64)) and p.ref.V >= 4096
    assert len(set(R.home_slots(keys, p.m.max_voxels))) < p.ref.V, "two voxels share a home slot: one of them is found by a second probe"
    for k in range(2):
        eye, target = g.uniform(-0.3, 0.3, 3), g.uniform(-1.0, 1.0, 3)
        _, want, _ = p.check(_look(eye, target, 64, 48, fov=75.0), min_count=1 + k, forms=(k == 0))
        assert (want != R.EMPTY).mean() > 0.5


# ------------------------------------------------------------------------------------------------ invariants and interop
def test_a_view_writes_nothing_and_repeats_itself_and_occupied_hides_a_ghost(S):
    p = Pair(S, H3, 2048)
    wall = _box_points()
    ghost = np.array([_centre((8, 8, 11), H3)], dtype=f32)
    ids = p.add(np.concatenate([wall, ghost]))
    origin = _centre((8, 8, 8), H3).tolist()
    for _ in range(2):
        p.m.carve(_dev(wall), origin)
    occupied = p.m.occupied()
    assert not bool(occupied[ids[-1]]) and int(occupied.sum()) == p.ref.V - 1
    cam = R.axis_camera(origin, 9, 9, 6.0, 4.5, 4.5)
    block, carve = p.m._block.clone(), p.m._carve.clone()
    shown = p.m.view(cam)
    hidden = p.m.view(cam, occupied=True)
    assert torch.equal(p.m._block, block) and torch.equal(p.m._carve, carve), "the map block and the carve block are only read"
    assert torch.equal(p.m.view(cam).keys, shown.keys) and torch.equal(p.m.view(cam, occupied=True).keys, hidden.keys)
    assert torch.equal(shown.keys.cpu(), torch.from_numpy(R.view(p.ref, cam)[0]))
    assert torch.equal(hidden.keys.cpu(), torch.from_numpy(R.view(p.ref, cam, ~occupied.cpu().numpy())[0]))
    assert int(shown.index[4, 4]) == ids[-1] and int(hidden.index[4, 4]) == int(p.ref.locate(np.array([_centre((8, 8, 14), H3)], dtype=f32))[0])
    assert not bool((hidden.index == int(ids[-1])).any())
    p.check(cam, occupied=occupied.cpu().numpy())


def test_the_keys_go_through_every_reader_of_a_view(box, S):
    from point_sam_amd import ops
    from point_sam_amd.config import get_config
    from point_sam_amd.predictor import PointSAMPredictor
    m, V = box.m, box.ref.V
    cam = _look(_centre((8, 8, 8), H3), (-0.5, 0.6, 0.3), 24, 16)
    view = PointSAMPredictor(model=None).map_view(m, cam, occupied=None)
    want = R.view(box.ref, cam)[0]
    assert torch.equal(view.keys.cpu(), torch.from_numpy(want))
    labels = m.label_image(view)
    ref_label = box.ref.labels()[0]
    assert labels.dtype == torch.int32 and np.array_equal(labels.cpu().numpy(), ref_label[want & 0xffffffff]) and set(ref_label.tolist()) == {0, 1, 2}
    assert torch.equal(ops.view_paint_ids(view.keys, m.bits(3)[0], V), labels), "bits(K) painted through the keys is labels() per pixel"
    assert (m.label_image(view, min_votes=2) == -1).all(), "every voxel has one vote"
    rows = ops.view_paint_rows(view.keys, m.bits(3)[0], V)
    assert torch.equal(rows.to(torch.int32).argmax(0).to(torch.int32), labels) and int(rows.sum()) == 24 * 16
    pixels = torch.tensor([[0, 0], [23, 15], [7, 9], [12, 3]], dtype=torch.int32, device="cuda")
    assert torch.equal(ops.view_pick(view.keys, pixels, 0), view.index[pixels[:, 1].long(), pixels[:, 0].long()]), "a click gives a voxel id"
    rgb = m.cloud()[1]
    img = view.colour(rgb, background=-1.0)
    assert bool((img >= 0).all()) and torch.equal(img, rgb[view.index.long()]), "no background pixel where the reference hits"
    # an empty pixel stays empty in every reader
    out = S.ScanMap(H3, 64)
    out.add(_dev(np.array([_centre((8, 8, 12), H3)], dtype=f32)), torch.zeros(1, 3, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"))
    view = out.view(R.axis_camera(_centre((8, 8, 8), H3), 3, 3, 1.0, 1.5, 1.5))
    assert out.label_image(view).cpu().tolist() == [[-1, -1, -1], [-1, 0, -1], [-1, -1, -1]]
    assert view.depth.cpu()[1, 1] == 4 * H3 and torch.isinf(view.depth.cpu()[0, 0])


def test_a_block_cleared_with_another_voxel_size_shows_nothing(S):
    """The C entry lays the bitmap out for the inv_h it is given; a block whose header holds another one must not be walked with it."""
    from point_sam_amd import ops
    m = S.ScanMap(H3, 64)
    m.add(_dev(np.array([_centre((8, 8, 12), H3)], dtype=f32)), torch.zeros(1, 3, device="cuda"))
    cam = R.axis_camera(_centre((8, 8, 8), H3), 3, 3, 1.0, 1.5, 1.5)
    assert int(m.view(cam).index[1, 1]) == 0
    assert bool((ops.map_view(m._block, m.max_voxels, m.max_pairs, 1, cam, voxel_size=2.0 ** -4) == -1).all())
