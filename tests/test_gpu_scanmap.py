"""Scan maps on the GPU (csrc/scanmap.hip, point_sam_amd/scanmap.py, predictor.map_add / map_lookup) against the plain numpy reference
tests/scanmap_reference.py.  Every comparison is exact: integers as integers, floats through an int32 view."""
import ctypes

import numpy as np
import pytest
import torch

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


def _scan(M, seed, lo=-0.95, hi=0.95, labels=(-1, 5)):
    g = np.random.default_rng(seed)
    return g.uniform(lo, hi, (M, 3)).astype(f32), g.uniform(-1, 1, (M, 3)).astype(f32), g.integers(labels[0], labels[1], M).astype(np.int32)


def _add(m, ref, xyz, rgb, lab, pose=None):
    """One add into the device map and the reference; ids and the status counts agree -> the device's AddResult."""
    res = m.add(_dev(xyz), _dev(rgb), _dev(lab), pose)
    ids, new, acc, rej = ref.add(xyz, rgb, lab, pose)
    assert res.ids.dtype == torch.int32 and np.array_equal(res.ids.cpu().numpy(), ids)
    assert (res.new_voxels, res.accepted, res.rejected) == (new, acc, rej)
    assert m.num_voxels == ref.V and m.num_adds == ref.adds
    return res


def _state(m):
    """Every output of a device map as numpy arrays."""
    sq, sc = m.sums()
    out = [m.counts(), m.first_seen(), m.last_seen(), m.keys(), sq, sc, *m.labels(1), *m.labels(2), *m.cloud()]
    return [t.cpu().numpy() for t in out]


def _check_map(m, ref):
    count, first, last, keys, sq, sc = ref.fields()
    xyz, rgb = ref.cloud()
    want = [count, first, last, keys, sq, sc, *ref.labels(1), *ref.labels(2), xyz, rgb]
    got = _state(m)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        assert np.array_equal(g.view(np.int32) if g.dtype == f32 else g, w.view(np.int32) if w.dtype == f32 else w)


def _by_key(state):
    """The per-key part of _state, ordered by key."""
    order = np.argsort(state[3])
    return [a[order] for a in state]


# ------------------------------------------------------------------------------------------------ 1: block edges
@pytest.mark.parametrize("M", [1, 63, 64, 65, 255, 257, 1023, 1025, 2049])
def test_block_edges(S, M):
    m, ref = S.ScanMap(H, 4096), SM.RefMap(H, 4096)
    xyz, rgb, lab = _scan(M, M)
    _add(m, ref, xyz, rgb, lab)
    _check_map(m, ref)
    assert np.array_equal(m.locate(_dev(xyz)).cpu().numpy(), ref.locate(xyz))
    # a second scan of the same width under a pose: old and new voxels at the same edges
    pose = SM.rotation_pose()
    xyz2, rgb2, lab2 = _scan(M, M + 7, -0.6, 0.6)
    _add(m, ref, xyz2, rgb2, lab2, pose)
    _check_map(m, ref)
    assert np.array_equal(m.locate(_dev(xyz2), pose).cpu().numpy(), ref.locate(xyz2, pose))
    assert np.array_equal(m.locate(_dev(xyz)).cpu().numpy(), ref.locate(xyz))
    bits, area = m.bits(5)
    label = ref.labels()[0]
    assert area.cpu().tolist() == [int((label == k).sum()) for k in range(5)] and bits.shape == (5, (ref.V + 63) // 64)


# ------------------------------------------------------------------------------------------------ 2: one voxel
def test_one_voxel_under_full_contention(S):
    g = np.random.default_rng(2)
    xyz = g.uniform(0.01, 0.12, (4096, 3)).astype(f32)
    xyz[:2048] = xyz[0]                                            # half of them identical
    rgb = g.uniform(-1, 1, (4096, 3)).astype(f32)
    lab = g.integers(0, 3, 4096).astype(np.int32)
    m, ref = S.ScanMap(H, 8), SM.RefMap(H, 8)
    res = _add(m, ref, xyz, rgb, lab)
    assert res.new_voxels == 1 and m.num_voxels == 1 and int(m.counts()[0]) == 4096
    _check_map(m, ref)
    assert int(m.labels()[1][0]) == int(np.bincount(lab).max())


# ------------------------------------------------------------------------------------------------ 3: runs across waves
def test_runs_across_waves_and_a_shuffle_of_them(S):
    g = np.random.default_rng(3)
    xyz, rgb, lab = _scan(3000, 33)
    key = SM.point_terms(xyz, rgb, None, SM.inv_h_of(H))[1]
    order = np.argsort(key, kind="stable")                         # runs of equal voxels, crossing lane 63 / 64 and the block boundaries
    xyz, rgb, lab = xyz[order], rgb[order], lab[order]
    singles = np.stack([np.linspace(-0.9, 0.9, 60), np.full(60, -0.97), np.full(60, 0.97)], 1).astype(f32)      # 60 points, then ...
    run = g.uniform(0.51, 0.61, (100, 3)).astype(f32)             # ... one run of 100 in one voxel from lane 60 on: lanes 60 .. 159
    assert len(set(SM.point_terms(run, None, None, SM.inv_h_of(H))[1].tolist())) == 1
    xyz = np.concatenate([singles, run, xyz])
    rgb = np.concatenate([g.uniform(-1, 1, (160, 3)).astype(f32), rgb])
    lab = np.concatenate([g.integers(-1, 5, 160).astype(np.int32), lab])
    m, ref = S.ScanMap(H, 4096), SM.RefMap(H, 4096)
    _add(m, ref, xyz, rgb, lab)
    _check_map(m, ref)
    perm = g.permutation(len(xyz))
    m2, ref2 = S.ScanMap(H, 4096), SM.RefMap(H, 4096)
    _add(m2, ref2, xyz[perm], rgb[perm], lab[perm])
    _check_map(m2, ref2)
    a, b = _by_key(_state(m)), _by_key(_state(m2))
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int32) if x.dtype == f32 else x, y.view(np.int32) if y.dtype == f32 else y)
    assert not np.array_equal(m.keys().cpu().numpy(), m2.keys().cpu().numpy()), "the ids follow the order of the points, the per-key state does not"


# ------------------------------------------------------------------------------------------------ 4: three posed adds
def _unposed(p, pose):
    """Scan-frame points whose pose lands (to fp32 rounding) on p."""
    R, t = pose[:, :3], pose[:, 3]
    return ((np.asarray(p, dtype=np.float64) - t) @ R).astype(f32)


def _three_adds():
    poses = [SM.rotation_pose(20, -35, (0.05, -0.1, 0.02)), SM.rotation_pose(-10, 15, (-0.03, 0.04, 0.1)), SM.rotation_pose(33, 8, (0.0, 0.07, -0.05))]
    centre = np.full((1, 3), 0.9375)                               # the middle of voxel [0.875, 1)^3, the flipping voxel: no other point comes near
    votes = [[1, 1, 1], [2, 2], [2, 2]]                            # 1 leads 3 : 2 after the second add, 2 leads 4 : 3 after the third
    scans = []
    for j, pose in enumerate(poses):
        xyz, rgb, lab = _scan(1500, 40 + j, -0.4, 0.4)             # posed: inside the ball of radius 0.4 sqrt(3) + 0.12 < 0.875
        n = len(votes[j])
        xyz[:n] = _unposed(np.repeat(centre, n, 0) + 0.01 * np.arange(n)[:, None], pose)
        lab[:n] = votes[j]
        scans.append((xyz, rgb, lab, pose))
    return scans


def test_three_posed_adds(S):
    m, ref = S.ScanMap(H, 4096), SM.RefMap(H, 4096)
    scans = _three_adds()
    flip, results = [], []
    for j, (xyz, rgb, lab, pose) in enumerate(scans):
        before = _state(m) if j else None
        V0 = m.num_voxels
        res = _add(m, ref, xyz, rgb, lab, pose)
        results.append(res)
        _check_map(m, ref)
        v = int(res.ids[0])
        lbl, votes = m.labels()
        flip.append((int(lbl[v]), int(votes[v])))
        if before is not None:
            after = _state(m)
            assert np.array_equal(after[3][:V0], before[3]) and np.array_equal(after[1][:V0], before[1]), "earlier ids and first_seen are untouched"
            seen = np.unique(res.ids.cpu().numpy())
            seen = seen[seen >= 0]
            assert (after[2][seen] == j + 1).all() and (after[1][V0:] == j + 1).all()
            untouched = np.setdiff1d(np.arange(V0), seen)
            assert len(untouched) > 0 and np.array_equal(after[2][untouched], before[2][untouched])
    assert flip == [(1, 3), (1, 3), (2, 4)], "the majority flips on the third add"
    for (xyz, rgb, lab, pose), res in zip(scans, results):
        assert torch.equal(m.locate(_dev(xyz), pose), res.ids)


# ------------------------------------------------------------------------------------------------ 5: rejected points
def test_rejected_points(S):
    xyz, rgb, accepted = SM.boundary_case()
    m, ref = S.ScanMap(2.0 ** -4, 64), SM.RefMap(2.0 ** -4, 64)
    res = _add(m, ref, xyz, rgb, np.arange(len(xyz), dtype=np.int32))
    assert np.array_equal(res.ids.cpu().numpy() >= 0, accepted) and res.rejected == int((~accepted).sum())
    _check_map(m, ref)
    assert np.array_equal(m.locate(_dev(xyz)).cpu().numpy(), ref.locate(xyz))
    # a pose that carries part of the scan out of [-1, 1]
    shift = np.array([[1, 0, 0, 0.5], [0, 1, 0, 0], [0, 0, 1, -0.75]], dtype=np.float64)
    xyz2, rgb2, lab2 = _scan(700, 5)
    m, ref = S.ScanMap(H, 4096), SM.RefMap(H, 4096)
    res = _add(m, ref, xyz2, rgb2, lab2, shift)
    assert 100 < res.rejected < 600
    _check_map(m, ref)
    assert np.array_equal(m.locate(_dev(xyz2), shift).cpu().numpy(), ref.locate(xyz2, shift))


# ------------------------------------------------------------------------------------------------ 6: labels
def test_labels_negative_zero_and_int32_max(S):
    p = np.array([[0.1, 0.1, 0.1]] * 7 + [[-0.6, 0.1, 0.1]] * 3 + [[0.1, -0.6, 0.1]], dtype=f32)
    lab = np.array([7, 3, 7, 3, 9, -1, -5, 2 ** 31 - 1, 2 ** 31 - 1, 0, -2 ** 31], dtype=np.int32)
    m, ref = S.ScanMap(0.5, 16), SM.RefMap(0.5, 16)
    _add(m, ref, p, np.zeros_like(p), lab)
    _check_map(m, ref)
    assert m.labels()[0].cpu().tolist() == [3, 2 ** 31 - 1, -1] and m.labels()[1].cpu().tolist() == [2, 2, 0]
    assert m.labels(3)[0].cpu().tolist() == [-1, -1, -1]
    _add(m, ref, p[:1], np.zeros((1, 3), f32), np.array([7], dtype=np.int32))
    _check_map(m, ref)
    assert int(m.labels()[0][0]) == 7
    # without labels nothing is voted
    m, ref = S.ScanMap(0.5, 16), SM.RefMap(0.5, 16)
    _add(m, ref, p, np.zeros_like(p), None)
    _check_map(m, ref)
    assert m.labels()[0].cpu().tolist() == [-1, -1, -1]


# ------------------------------------------------------------------------------------------------ 7: capacities
def _guarded(S, h, max_voxels, max_pairs):
    """A ScanMap whose block lies between two 4 KiB guards of 0xA5 -> (map, the whole buffer, the block's words)."""
    from point_sam_amd import ops
    m = S.ScanMap(h, max_voxels, max_pairs)
    nbytes = ops.map_bytes(m.max_voxels, m.max_pairs)
    assert nbytes % 16 == 0
    n = nbytes // 8                                                # exactly the block: the second guard begins at its last byte's neighbour
    buf = torch.full((n + 2 * GUARD_WORDS,), int(GUARD), dtype=torch.int64, device="cuda")
    m._block = buf[GUARD_WORDS:GUARD_WORDS + n]
    m.clear()
    return m, buf, n


def _guards_intact(buf, n):
    return bool((buf[:GUARD_WORDS] == int(GUARD)).all()) and bool((buf[GUARD_WORDS + n:] == int(GUARD)).all())


def test_capacities_overflow_is_an_error_and_stays_inside_the_block(S):
    xyz, rgb, lab = _scan(1500, 7)
    full = SM.RefMap(H, 4096)
    full.add(xyz, rgb, lab)
    V, pairs = full.V, len(full.pairs)
    assert V > 400 and 400 < pairs <= 4 * V
    for caps, ok in (((V, pairs), True), ((V - 1, 4 * V), False), ((V, pairs - 1), False)):
        m, buf, n = _guarded(S, H, *caps)
        ref = SM.RefMap(H, *caps)
        if ok:
            _add(m, ref, xyz, rgb, lab)
            _check_map(m, ref)
        else:
            with pytest.raises(S.MapOverflow):
                m.add(_dev(xyz), _dev(rgb), _dev(lab))
            for call in (lambda: m.add(_dev(xyz[:10]), _dev(rgb[:10]), _dev(lab[:10])), m.labels, m.cloud, m.counts, lambda: m.locate(_dev(xyz[:10]))):
                with pytest.raises(S.MapOverflow):
                    call()
            assert _guards_intact(buf, n)
            m.clear()                                              # revives the map
            _add(m, ref, xyz[:300], rgb[:300], lab[:300])
            _check_map(m, ref)
        assert _guards_intact(buf, n)


# ------------------------------------------------------------------------------------------------ 8: exact workspace
def test_exact_workspace_through_the_c_abi(S):
    from point_sam_amd import _lib, ops
    lib = _lib.load()
    M = 1500
    xyz, rgb, lab = _scan(M, 8)
    m, ref = S.ScanMap(H, 4096), SM.RefMap(H, 4096)
    first = _add(m, ref, xyz, rgb, lab)
    want = _state(m)
    ws_bytes = lib.psam_map_add_workspace_bytes(M)
    assert ws_bytes % 16 == 0
    for short in (1, 0):
        other = S.ScanMap(H, 4096)
        buf = torch.full((ws_bytes + 2 * 4096,), 0xA5, dtype=torch.uint8, device="cuda")
        ws = buf[4096:4096 + ws_bytes]
        ids = torch.full((M,), -7, dtype=torch.int32, device="cuda")
        dx, dr, dl = _dev(xyz), _dev(rgb), _dev(lab)
        header = ops.map_header(other._block)
        st = lib.psam_map_add(other._block.data_ptr(), other._block.numel() * 8, 4096, 8192, dx.data_ptr(), dr.data_ptr(), dl.data_ptr(), M, None,
                              ids.data_ptr(), ws.data_ptr(), ws_bytes - short, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert bool((buf[:4096] == 0xA5).all()) and bool((buf[4096 + ws_bytes:] == 0xA5).all())
        if short:
            assert st == -3 and "workspace too small" in lib.psam_last_error_string().decode()
            assert bool((buf == 0xA5).all()) and bool((ids == -7).all()) and ops.map_header(other._block) == header, "a refused call touches nothing"
        else:
            assert st == 0
            h = ops.map_header(other._block)
            assert h[ops.MAP_H_FLAGS] == 0 and h[ops.MAP_H_V] == ref.V and h[ops.MAP_H_ADDS] == 1 and h[ops.MAP_H_PAIRS] == len(ref.pairs)
            other._V, other._adds = h[ops.MAP_H_V], h[ops.MAP_H_ADDS]
            assert torch.equal(ids, first.ids)
            for g, w in zip(_state(other), want):
                assert np.array_equal(g.view(np.int32) if g.dtype == f32 else g, w.view(np.int32) if w.dtype == f32 else w)


# ------------------------------------------------------------------------------------------------ 9: second level of the scan
def test_more_than_1024_scan_blocks(S):
    M = 1024 * 1024 + 1025
    xyz, rgb, lab = _scan(M, 9)
    xyz[12345, 1], rgb[777777, 0] = np.nan, np.inf
    h = 2.0 ** -6
    m, ref = S.ScanMap(h, 1 << 20, 1 << 21), SM.FastMap(h, 1 << 20, 1 << 21)      # about 0.8 M of the 2 M voxels, at most M pairs
    res = _add(m, ref, xyz, rgb, lab)
    assert res.rejected == 2 and res.new_voxels > 200000
    _check_map(m, ref)
    assert np.array_equal(m.locate(_dev(xyz)).cpu().numpy(), ref.locate(xyz))


# ------------------------------------------------------------------------------------------------ 10: repeatability
def test_the_same_adds_twice_give_the_same_bits(S):
    runs = []
    for _ in range(2):
        m = S.ScanMap(H, 4096)
        ids = [m.add(_dev(x), _dev(r), _dev(l), pose).ids for x, r, l, pose in _three_adds()]
        sq, sc = m.sums()
        runs.append(ids + [m.counts(), m.first_seen(), m.last_seen(), m.keys(), sq, sc, *m.labels(), *m.cloud()])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


# ------------------------------------------------------------------------------------------------ 11: predictor
def test_predictor_map_add_lookup_and_the_map_as_a_scan(S):
    from point_sam_amd.model import PointCloudSAM
    from point_sam_amd.predictor import PointSAMPredictor
    cfg = get_config("tiny")
    pred = PointSAMPredictor(PointCloudSAM(cfg, random_state_dict(cfg, 3), "cuda", precision="f16x3"))
    g = np.random.default_rng(11)

    def sphere(n, centre, r):
        d = g.normal(size=(n, 3))
        return (np.asarray(centre) + r * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    a = np.concatenate([sphere(2000, (0.2, 0.0, 0.0), 0.3), sphere(2000, (-0.3, 0.1, 0.1), 0.25)])
    pose = SM.rotation_pose(12, -9, (0.02, -0.03, 0.01))
    b = np.concatenate([_unposed(a[::2], pose), _unposed(sphere(1000, (0.0, -0.4, 0.2), 0.2), pose)])      # a posed copy plus new points
    a_rgb, b_rgb = g.uniform(0, 1, a.shape).astype(f32), g.uniform(0, 1, b.shape).astype(f32)
    a_lab = np.where(np.arange(len(a)) < 2000, 0, 1).astype(np.int32)
    b_lab = g.integers(-1, 3, len(b)).astype(np.int32)
    h = 2.0 ** -4
    m, ref = S.ScanMap(h, 1 << 14), SM.RefMap(h, 1 << 14)
    with pytest.raises(RuntimeError):
        pred.map_add(m)
    ax, ar, bx, br = _dev(a), _dev(a_rgb), _dev(b), _dev(b_rgb)
    pred.set_scene(ax, ar, max_points=1024)
    assert not pred.scene.identity
    empty = pred.map_lookup(m)
    assert empty.shape == (len(a),) and empty.dtype == torch.int32 and bool((empty == -1).all()), "an empty map has no voxel anywhere"
    res = pred.map_add(m, _dev(a_lab))                            # the scan's full-resolution points, not the working cloud
    want = ref.add(a, a_rgb, a_lab)
    assert np.array_equal(res.ids.cpu().numpy(), want[0]) and (res.new_voxels, res.accepted, res.rejected) == want[1:]
    pred.set_scene(bx, br, max_points=1024)
    with pytest.raises(ValueError):
        pred.map_add(m, _dev(b_lab[:-1]), pose)
    res = pred.map_add(m, _dev(b_lab), pose)
    want = ref.add(b, b_rgb, b_lab, pose)
    assert np.array_equal(res.ids.cpu().numpy(), want[0]) and (res.new_voxels, res.accepted, res.rejected) == want[1:] and res.new_voxels > 0
    _check_map(m, ref)
    for mv in (1, 3):
        loc, label = ref.locate(b, pose), ref.labels(mv)[0]
        got = pred.map_lookup(m, pose, mv)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), np.where(loc >= 0, label[np.maximum(loc, 0)], -1))
    far = pred.map_lookup(m, np.array([[1, 0, 0, 0.0], [0, 1, 0, 0.9], [0, 0, 1, 0.0]]))
    assert bool((far == -1).any())
    pred.set_crop((0.2, 0.0, 0.0), 0.5)
    with pytest.raises(RuntimeError):
        pred.map_add(m, _dev(b_lab), pose)
    pred.clear_crop()
    # the map is a scan like any other
    mx, mr = m.cloud()
    pred.set_scene(mx, mr, max_points=1024)
    click = mx[:1][None].contiguous()
    masks, scores, logits = pred.predict_masks(click, torch.ones(1, 1, dtype=torch.int64, device="cuda"), None, True)
    assert masks.shape[-1] == m.num_voxels == ref.V and logits.shape[-1] == ref.V
    # without a scene the cloud as encoded is the scan
    pred.set_pointcloud(ax[None, :1024].contiguous(), ar[None, :1024].contiguous())
    m2, ref2 = S.ScanMap(h, 1 << 12), SM.RefMap(h, 1 << 12)
    res = pred.map_add(m2, _dev(a_lab[:1024]))
    want = ref2.add(a[:1024], a_rgb[:1024], a_lab[:1024])
    assert np.array_equal(res.ids.cpu().numpy(), want[0])
    _check_map(m2, ref2)
