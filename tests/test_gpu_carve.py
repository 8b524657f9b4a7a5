"""Scan map carving on the GPU (csrc/carve.hip, ScanMap.carve, predictor.map_carve / map_carve_frames) against tests/carve_reference.py.  Every comparison
is exact.  The carve block lies between guard words, and the map's whole state is compared before and after every carve: a carve never writes it."""
import numpy as np
import pytest
import torch

import carve_reference as CR
import scanmap_reference as SM
from point_sam_amd.config import get_config
from point_sam_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu
f32 = np.float32
H = 2.0 ** -3
GUARD_WORDS = 512            # 4 KiB of int64
GUARD = np.int64(np.uint64(0xA5A5A5A5A5A5A5A5).view(np.int64))


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd import scanmap
    return scanmap


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _scan(M, seed, lo=-0.95, hi=0.95):
    g = np.random.default_rng(seed)
    return g.uniform(lo, hi, (M, 3)).astype(f32)


class Pair:
    """A device map with a guarded carve block beside the reference of both."""

    def __init__(self, S, h, max_voxels):
        from point_sam_amd import ops
        self.m, self.ref = S.ScanMap(h, max_voxels), SM.RefMap(h, max_voxels)
        self.cut = CR.RefCarve(self.ref)
        self.n = ops.carve_bytes(max_voxels) // 8                  # exactly the block: the second guard begins at its last byte's neighbour
        self.buf = torch.full((self.n + 2 * GUARD_WORDS,), int(GUARD), dtype=torch.int64, device="cuda")
        self.m._carve = self.buf[GUARD_WORDS:GUARD_WORDS + self.n]
        ops.carve_clear(self.m._carve, max_voxels)

    def add(self, xyz, pose=None, rgb=None):
        rgb = np.zeros_like(xyz) if rgb is None else rgb
        res = self.m.add(_dev(xyz), _dev(rgb), None, pose)
        want = self.ref.add(xyz, rgb, None, pose)
        assert np.array_equal(res.ids.cpu().numpy(), want[0])
        return res

    def map_state(self):
        return self.m._block.clone()

    def guards_intact(self):
        return bool((self.buf[:GUARD_WORDS] == int(GUARD)).all()) and bool((self.buf[GUARD_WORDS + self.n:] == int(GUARD)).all())

    def carve(self, xyz, origin, pose=None, margin=1):
        """One carve on both sides: the result, the header and every voxel's four words agree; the map's block is bit for bit what it was."""
        from point_sam_amd import ops
        before = self.map_state()
        res = self.m.carve(_dev(xyz), origin, pose, margin)
        rays, acc, rej, hit, missed, crossed, has = self.cut.carve(xyz, origin, pose, margin)
        assert (res.rays, res.accepted, res.rejected, res.hit_voxels, res.missed_voxels, res.crossed) == (rays, acc, rej, hit, missed, crossed)
        h = ops.carve_header(self.m._carve)
        assert h[:10] == [self.m.max_voxels, self.cut.carves, self.cut.stamp, has, rays, acc, rej, hit, missed, 0] and h[10] == crossed and h[12:] == [0] * 4
        assert self.m.num_carves == self.cut.carves
        assert torch.equal(self.map_state(), before), "a carve never writes the map block"
        assert self.guards_intact()
        self.check()
        return res

    def check(self):
        if self.ref.V == 0:
            return
        got = [self.m.hits(), self.m.misses(), self.m.last_hit(), self.m.last_missed()]
        for g, w in zip(got, self.cut.fields()):
            g = g.cpu().numpy()
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)

    def block(self):
        return self.m._carve.clone()


def _cell_centres(cells, h):
    """Points at the centres of cells of size h (a power of two: exact in fp32)."""
    return ((np.asarray(cells, dtype=np.float64) + 0.5) * h - 1.0).astype(f32)


# ------------------------------------------------------------------------------------------------ 1: block and wave edges
@pytest.mark.parametrize("M", [1, 63, 64, 65, 257, 1025, 2049])
def test_block_and_wave_edges(S, M):
    p = Pair(S, H, 4096)
    p.add(_scan(1500, 1))
    p.add(_scan(1200, 2, -0.6, 0.6), SM.rotation_pose())
    origin = [-0.9, -0.85, 0.8]                                    # near a corner
    xyz = _scan(M, 100 + M)
    res = p.carve(xyz, origin)
    assert res.rays > 0 and res.accepted == M and res.missed_voxels > 0 and (M < 63 or res.hit_voxels > 0)
    # the same carve again with the same stamp: no voxel's words change, nor the carve count and the stamp
    from point_sam_amd import ops
    words, carves = p.block()[8:], p.m.num_carves
    h = ops.carve_scan(p.m._block, p.m.max_voxels, p.m.max_pairs, p.m._carve, _dev(xyz), origin, None, 1, carves)
    assert torch.equal(p.block()[8:], words) and h[ops.CARVE_H_CARVES] == carves and h[ops.CARVE_H_STAMP] == carves
    assert (h[ops.CARVE_H_RAYS], h[ops.CARVE_H_CROSSED]) == (res.rays, res.crossed) and h[ops.CARVE_H_HIT] == h[ops.CARVE_H_MISSED] == 0
    want = p.cut.carve(xyz, origin, None, 1, carves)
    assert want[3:5] == (0, 0) and want[0] == res.rays
    # a second carve with a new stamp under a rotated pose
    pose = SM.rotation_pose(-10, 15, (-0.03, 0.04, 0.1))
    res2 = p.carve(_scan(M, 200 + M, -0.6, 0.6), [0.1, -0.2, 0.3], pose)
    assert p.m.num_carves == 2 and res2.rays > 0


# ------------------------------------------------------------------------------------------------ 2: once per carve
def test_a_voxel_crossed_by_hundreds_of_rays_is_missed_once_per_carve(S):
    h = 2.0 ** -5                                                  # fine enough for hundreds of distinct end cells
    p = Pair(S, h, 4096)
    origin = [0.01, 0.01, 0.01]                                    # cell (32, 32, 32)
    beside = _cell_centres([(33, 32, 32)], h)
    p.add(beside)
    g = np.random.default_rng(4)
    xyz = np.stack([g.uniform(0.7, 0.95, 2049), g.uniform(-0.3, 0.4, 2049), g.uniform(-0.3, 0.4, 2049)], 1).astype(f32)      # a wall far along +x
    through = sum(1 for k in {int(k) for k in SM.point_terms(xyz, None, None, p.ref.inv_h)[1]} if (33, 32, 32) in CR.walk((32, 32, 32), CR.cell_of_key(k)))
    assert through >= 300, "hundreds of rays, from every wave of the 2049 points, leave the origin's cell through the voxel beside it"
    for n in (1, 2, 3):
        res = p.carve(xyz[::-1] if n == 2 else xyz, origin)
        assert res.missed_voxels == 1 and res.rays >= through
        assert p.m.misses().tolist() == [n] and p.m.hits().tolist() == [0] and p.m.last_missed().tolist() == [n]
    # many more points than rays: 2049 points of one cell are one ray
    near = np.repeat(_cell_centres([(36, 32, 32)], h), 2049, 0) + g.uniform(-0.012, 0.012, (2049, 3)).astype(f32)
    p.carve(near, origin)
    assert p.m.misses().tolist() == [4]


# ------------------------------------------------------------------------------------------------ 3: ties
def test_ties_pass_through_edges_and_corners_without_missing_the_cells_beside(S):
    o, n = (3, 9, 4), 3
    ends = [(o[0] + n, o[1] + n, o[2] + n), (o[0] + n, o[1] + n, o[2]), (o[0] + 2 * n, o[1] + n, o[2]), (o[0] + n, o[1] - n, o[2] + 2 * n)]
    crossed, touched = set(), set()
    for e in ends:
        w = CR.walk(o, e)
        crossed |= set(w)
        box = {(x, y, z) for x in range(min(o[0], e[0]), max(o[0], e[0]) + 1) for y in range(min(o[1], e[1]), max(o[1], e[1]) + 1)
               for z in range(min(o[2], e[2]), max(o[2], e[2]) + 1)}
        touched |= {c for c in box if any(CR.chebyshev(c, d) == 1 for d in [o] + w + [e])}
    touched -= crossed | set(ends) | {o}
    # the diagonal passes through the corner of (4, 10, 5) with its seven neighbours: (4, 9, 5) and (3, 10, 5) are only touched, by every ray
    assert (4, 10, 5) in crossed and (4, 9, 5) in touched and (3, 10, 5) in touched and len(touched) > 20
    p = Pair(S, H, 4096)
    cells = sorted(crossed) + sorted(touched)
    p.add(_cell_centres(cells, H))                                 # the crossed cells and the corner-touched cells beside them are all in the map
    res = p.carve(_cell_centres(ends, H), _cell_centres([o], H)[0].tolist(), margin=0)
    assert res.rays == 4 and res.missed_voxels == len(crossed) and res.crossed == sum(len(CR.walk(o, e)) for e in ends)
    misses = p.m.misses().cpu().numpy()
    assert misses[:len(crossed)].tolist() == [1] * len(crossed) and misses[len(crossed):].tolist() == [0] * len(touched)


# ------------------------------------------------------------------------------------------------ 4: hit beats miss
def test_a_grazed_near_wall_is_hit_not_missed_until_it_is_gone(S):
    g = np.random.default_rng(6)
    t = np.linspace(-0.9, 0.9, 40)
    yy, zz = np.meshgrid(t, t[t < 0.0], indexing="ij")
    near = np.stack([np.full(yy.size, 0.05), yy.ravel(), zz.ravel()], 1).astype(f32)       # x = 0.05, the lower half: seen over its top
    yy, zz = np.meshgrid(t, t, indexing="ij")
    far = np.stack([np.full(yy.size, 0.9), yy.ravel(), zz.ravel()], 1).astype(f32)
    origin = [-0.9, 0.0, -0.5]
    p = Pair(S, H, 4096)
    both = np.concatenate([far, near])[g.permutation(len(far) + len(near))]
    p.add(both)
    res = p.carve(both, origin)
    near_ids = np.unique(p.ref.locate(near))
    o = CR.origin_cell(origin, None, p.ref.inv_h)
    grazed = {p.ref.id_of[CR.key_of_cell(c)] for k in {int(k) for k in SM.point_terms(far, None, None, p.ref.inv_h)[1]}
              for c in CR.walk(o, CR.cell_of_key(k)) if CR.key_of_cell(c) in p.ref.id_of} & set(near_ids.tolist())
    assert len(grazed) > 5, "rays to the far wall pass through voxels of the near wall"
    hits, misses = p.m.hits().cpu().numpy(), p.m.misses().cpu().numpy()
    assert (hits[near_ids] == 1).all() and (misses[near_ids] == 0).all() and res.missed_voxels == 0
    p.add(far)
    p.carve(far, origin)                                           # the near wall is gone from the next scan
    misses = p.m.misses().cpu().numpy()
    assert (misses[sorted(grazed)] == 1).all() and (p.m.hits().cpu().numpy()[near_ids] == 1).all()


# ------------------------------------------------------------------------------------------------ 5: margins and a voxel size that is no power of two
@pytest.mark.parametrize("h, margin", [(H, 0), (H, 1), (H, 3), (0.3, 0), (0.3, 1), (0.3, 3), (2.0 ** -4, 3)])
def test_margins_and_a_voxel_size_that_is_no_power_of_two(S, h, margin):
    p = Pair(S, h, 8192)
    p.add(_scan(3000, 11))
    res = p.carve(_scan(700, 12), [0.7, -0.6, -0.75], SM.rotation_pose(5, 5, (0.02, 0, 0)), margin)
    assert res.rays > 0 and res.crossed > 0
    wider = Pair(S, h, 8192)
    wider.add(_scan(3000, 11))
    more = wider.carve(_scan(700, 12), [0.7, -0.6, -0.75], SM.rotation_pose(5, 5, (0.02, 0, 0)), margin + 1)
    assert more.crossed < res.crossed and more.rays == res.rays


# ------------------------------------------------------------------------------------------------ 6: a long ray
def test_a_long_ray_whose_differences_pass_2_to_the_32(S):
    h = 2.0 ** -17
    o, e = (10, 20, 30), (70011, 70019, 33)
    w = CR.walk(o, e)
    assert 1.3e5 < len(w) < 1.5e5 and (2 * 70000 + 1) * 69999 > 2 ** 32, "the compared products do not fit 32 bits"
    on = [w[i] for i in np.linspace(50, len(w) - 50, 20).astype(int)]
    on_set = set(w)
    beside = []
    for c in on[:10]:
        for d in ((0, 0, 1), (0, 0, -1), (1, -1, 0), (-1, 1, 0), (0, 1, 1)):
            b = (c[0] + d[0], c[1] + d[1], c[2] + d[2])
            if b not in on_set and b not in beside:
                beside.append(b)
                break
    assert len(beside) == 10 and len(set(on)) == 20
    p = Pair(S, h, 64)
    res_add = p.add(_cell_centres(on + beside, h))
    assert res_add.new_voxels == 30
    res = p.carve(_cell_centres([e], h), _cell_centres([o], h)[0].tolist())
    assert res.rays == 1 and res.crossed == len([c for c in w if CR.chebyshev(c, e) > 1]) and res.missed_voxels == 20
    assert p.m.misses().tolist() == [1] * 20 + [0] * 10 and p.m.hits().tolist() == [0] * 30


# ------------------------------------------------------------------------------------------------ 7: invariance
def test_a_permutation_and_a_second_run_give_identical_blocks(S):
    g = np.random.default_rng(8)
    a, b, xyz = _scan(1500, 21), _scan(1200, 22, -0.6, 0.6), _scan(2049, 23)
    xyz[7, 1], xyz[900, 0] = np.nan, np.inf
    pose, origin = SM.rotation_pose(), [-0.4, 0.3, 0.2]
    blocks = []
    for order in (np.arange(2049), g.permutation(2049), np.arange(2049)):
        p = Pair(S, H, 4096)
        p.add(a)
        p.add(b, pose)
        res = p.carve(xyz[order], origin, pose, 1)
        assert res.rejected >= 2
        p.carve(b, [0.0, 0.0, 0.0], pose, 2)
        blocks.append(p.block())
    assert torch.equal(blocks[0], blocks[1]) and torch.equal(blocks[0], blocks[2])


# ------------------------------------------------------------------------------------------------ 8: lifecycle
def test_lifecycle_clear_an_empty_map_and_a_dead_map(S):
    from point_sam_amd import ops
    p = Pair(S, H, 600)
    res = p.carve(_scan(300, 31), [0.0, 0.0, 0.0])                 # an empty map: rays are walked, nothing is there to hit or miss
    assert res.rays > 0 and res.crossed > 0 and (res.hit_voxels, res.missed_voxels) == (0, 0)
    assert bool((p.block()[8:] == 0).all())
    p.add(_scan(300, 32))
    p.carve(_scan(300, 31), [0.0, 0.0, 0.0])
    assert int(p.m.misses().sum()) > 0 and p.m.num_carves == 2
    p.m.clear()
    p.ref.clear(); p.cut.clear()
    blk = p.block()
    assert p.m.num_carves == 0 and p.m.num_voxels == 0 and blk[0] == 600 and bool((blk[1:] == 0).all()) and p.guards_intact()
    assert ops.map_header(p.m._block)[ops.MAP_H_V] == 0
    p.add(_scan(300, 32))
    p.carve(_scan(300, 33), [0.5, 0.5, 0.5])
    # never carved: no block, everything occupied
    fresh = S.ScanMap(H, 600)
    fresh.add(_dev(_scan(300, 32)), _dev(np.zeros((300, 3), f32)))
    assert fresh._carve is None and bool(fresh.occupied().all()) and fresh.hits().tolist() == [0] * fresh.num_voxels
    # a dead map
    with pytest.raises(S.MapOverflow):
        p.m.add(_dev(_scan(2000, 34)), _dev(np.zeros((2000, 3), f32)))
    before = p.block()
    for call in (lambda: p.m.carve(_dev(_scan(10, 35)), [0.0, 0.0, 0.0]), p.m.occupied, p.m.hits, p.m.misses):
        with pytest.raises(S.MapOverflow):
            call()
    assert torch.equal(p.block(), before)
    with pytest.raises(ValueError, match="no cell"):
        fresh.carve(_dev(_scan(10, 35)), [0.0, 1.5, 0.0])
    assert fresh._carve is None, "refused before any launch and before the block is allocated"


# ------------------------------------------------------------------------------------------------ 9: end to end
def _room(box: bool, seed: int):
    """A room seen from inside: floor and four walls as grids of points, and a box standing on the floor."""
    g = np.random.default_rng(seed)
    t = np.linspace(-0.88, 0.88, 60)
    u, v = (a.ravel() for a in np.meshgrid(t, t, indexing="ij"))
    k = np.full(u.size, 0.9)
    parts = [np.stack([u, v, -k], 1), np.stack([k, u, v], 1), np.stack([-k, u, v], 1), np.stack([u, k, v], 1), np.stack([u, -k, v], 1)]
    if box:
        s = np.linspace(0.26, 0.49, 12)
        a, b = (x.ravel() for x in np.meshgrid(s, s, indexing="ij"))
        parts += [np.stack([a, b, np.full(a.size, -0.3)], 1), np.stack([np.full(a.size, 0.26), a, b - 0.75], 1), np.stack([a, np.full(a.size, 0.26), b - 0.75], 1)]
    xyz = np.concatenate(parts)
    return (xyz + g.uniform(-0.004, 0.004, xyz.shape)).astype(f32)


def test_end_to_end_a_box_that_was_moved_away_is_voted_free(S):
    h = 2.0 ** -3
    origin = [-0.1, -0.2, 0.3]
    p = Pair(S, h, 4096)
    a = _room(True, 41)
    p.add(a)
    p.carve(a, origin)
    box_cells = {CR.cell_of_key(k) for k in SM.point_terms(a[-3 * 144:], None, None, p.ref.inv_h)[1]}
    room_cells = {CR.cell_of_key(k) for k in SM.point_terms(a[:-3 * 144], None, None, p.ref.inv_h)[1]}
    box_ids = sorted(p.ref.id_of[CR.key_of_cell(c)] for c in box_cells - room_cells)
    room_ids = sorted(p.ref.id_of[CR.key_of_cell(c)] for c in room_cells)
    assert len(box_ids) >= 6
    assert bool(p.m.occupied().all())
    for seed in (42, 43):
        scan = _room(False, seed)
        p.add(scan)
        p.carve(scan, origin)
    occ = p.m.occupied()
    want = CR.occupied(*p.cut.fields()[:2])
    assert np.array_equal(occ.cpu().numpy(), want)
    assert not occ[box_ids].any() and bool(occ[room_ids].all())
    cloud = p.m.cloud()[0][occ].cpu().numpy()
    inside_box = (cloud[:, 0] > 0.25) & (cloud[:, 0] < 0.5) & (cloud[:, 1] > 0.25) & (cloud[:, 1] < 0.5) & (cloud[:, 2] > -0.8) & (cloud[:, 2] < -0.25)
    assert not inside_box.any() and len(cloud) == len(room_ids) + int(occ.sum()) - len(room_ids)
    assert bool(p.m.occupied(min_misses=3).all()), "two carves saw through the box: not enough for three"
    assert not p.m.occupied(1, 1, 2)[box_ids].any()


# ------------------------------------------------------------------------------------------------ 10: the predictor
@pytest.fixture(scope="module")
def pred():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd.model import PointCloudSAM
    from point_sam_amd.predictor import PointSAMPredictor
    cfg = get_config("tiny")
    return PointSAMPredictor(PointCloudSAM(cfg, random_state_dict(cfg, 3), "cuda", precision="f16x3"))


def test_predictor_map_carve(S, pred):
    g = np.random.default_rng(12)
    d = g.normal(size=(3000, 3))
    a = (0.8 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)          # a sphere seen from inside
    inner = (0.3 * d[:500] / np.linalg.norm(d[:500], axis=1, keepdims=True)).astype(f32)
    first = np.concatenate([a, inner])
    rgb = g.uniform(0, 1, first.shape).astype(f32)
    h = 2.0 ** -4
    p = Pair(S, h, 1 << 14)
    with pytest.raises(TypeError):
        pred.map_carve("x", [0, 0, 0])
    pred.set_scene(_dev(first), _dev(rgb), max_points=1024)
    assert not pred.scene.identity
    pred.map_add(p.m, None)
    p.ref.add(first, rgb)
    before = p.map_state()
    res = pred.map_carve(p.m, [0.0, 0.01, 0.02])                   # the scan's full-resolution points, not the working cloud
    want = p.cut.carve(first, [0.0, 0.01, 0.02])
    assert (res.rays, res.accepted, res.rejected, res.hit_voxels, res.missed_voxels, res.crossed) == want[:6] and res.hit_voxels == p.ref.V
    pose = SM.rotation_pose(12, -9, (0.02, -0.03, 0.01))
    pred.set_scene(_dev(a), _dev(rgb[:3000]), max_points=1024)
    with pytest.raises(ValueError):
        pred.map_carve(p.m, [0.0, 0.0, 0.0], pose, margin=-1)
    res = pred.map_carve(p.m, [0.0, 0.0, 0.0], pose, margin=2)     # the inner sphere is gone and is seen through
    want = p.cut.carve(a, [0.0, 0.0, 0.0], pose, 2)
    assert (res.rays, res.accepted, res.rejected, res.hit_voxels, res.missed_voxels, res.crossed) == want[:6] and res.missed_voxels > 50
    p.check()
    assert torch.equal(p.map_state(), before) and p.guards_intact()
    pred.set_crop((0.8, 0.0, 0.0), 0.5)
    with pytest.raises(RuntimeError):
        pred.map_carve(p.m, [0.0, 0.0, 0.0])
    pred.clear_crop()


def test_map_carve_frames_is_one_reference_carve_per_frame(S, pred):
    import frames_reference as R
    from point_sam_amd.views import Camera
    depth, rgb, cams, far = R.room_case()
    cameras = [Camera(c.pose_words.reshape(3, 4), c.fx, c.fy, c.cx, c.cy, c.width, c.height, c.near) for c in cams]
    # normalised by the points' own extent the cameras lie outside [-1, 1]^3, where an origin has no cell: twice the automatic scale brings them in
    auto = R.frames(depth, rgb, cams, far, 0.05)
    with pytest.raises(ValueError, match="no cell"):
        pred.map_carve_frames(S.ScanMap(2.0 ** -4, 64), pred.set_frames(depth, rgb, cameras, far, edge=0.05, max_points=2048))
    fs = pred.set_frames(depth, rgb, cameras, far, edge=0.05, center=auto["center"], scale=float(f32(2) * f32(auto["scale"])), max_points=2048)
    xyz, index = fs.xyz.cpu().numpy(), fs.index.cpu().numpy()
    h = 2.0 ** -6
    p = Pair(S, h, 1 << 14)
    col = fs.rgb.cpu().numpy()
    p.m.add(fs.xyz, fs.rgb)
    p.ref.add(xyz, col)
    P0 = fs.views[0].camera.pose.astype(np.float64)
    ghosts = ((xyz[:2000:40].astype(np.float64) + (-P0[:, :3].T @ P0[:, 3])) / 2).astype(f32)      # half way between the first camera and what it saw
    p.add(ghosts)
    out = pred.map_carve_frames(p.m, fs, None, 1)
    assert len(out) == len(cameras) == 2 and out[0].missed_voxels > 0
    for f, res in enumerate(out):
        mine = index[f][index[f] >= 0]
        assert np.array_equal(np.sort(mine), np.arange(mine.min(), mine.max() + 1)), "a frame's points are contiguous"
        P = fs.views[f].camera.pose.astype(np.float64)
        centre = (-P[:, :3].T @ P[:, 3]).astype(f32)
        want = p.cut.carve(xyz[mine.min():mine.max() + 1], centre)
        assert (res.rays, res.accepted, res.rejected, res.hit_voxels, res.missed_voxels, res.crossed) == want[:6] and res.rays > 0 and want[6] == 1
    p.check()
    assert p.m.num_carves == 2 and p.guards_intact()
    with pytest.raises(TypeError):
        pred.map_carve_frames(p.m, [fs.views[0]])
