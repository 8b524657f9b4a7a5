"""Multi-view label fusion on the device (csrc/fusion.hip, point_sam_amd/fusion.py) against the numpy reference (tests/fusion_reference.py).  Every
comparison is exact: bits as int64 words, everything else as integers."""
import numpy as np
import pytest
import torch

import frames_reference as R
import fusion_reference as FR
import view_reference as V
from point_sam_amd import _lib
from point_sam_amd.config import get_config
from point_sam_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu
I32 = np.iinfo(np.int32)
VOTE_KEYS = ("label", "votes", "seen", "labelled", "dropped")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd import ops
    return ops


def _camera(ref):
    from point_sam_amd.views import Camera
    return Camera(ref.pose_words.reshape(3, 4), ref.fx, ref.fy, ref.cx, ref.cy, ref.width, ref.height, ref.near)


def _dev(a):
    a = np.array(a)                                                # a writable, contiguous copy: the shared inputs are read-only
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def _check_all(ops, xyz, cams, keys, labels, rb, tau, seed=0):
    """Region bits, the vote (with a remap, with row_base alone, with consistent ids) and label bits of one input against the reference."""
    cameras = [_camera(c) for c in cams]
    dx, dk, dl = _dev(xyz), _dev(keys), _dev(labels)
    N, Rn, Vn = len(xyz), int(rb[-1]), len(cams)
    want_bits, want_area = FR.region_bits(xyz, cams, keys, labels, rb, tau)
    bits, area = ops.fuse_region_bits(dx, cameras, dk, dl, rb, tau)
    assert tuple(bits.shape) == (Rn + Vn, (N + 63) // 64) and np.array_equal(bits.cpu().numpy(), want_bits)
    assert np.array_equal(area.cpu().numpy(), want_area)
    remap = np.random.default_rng(seed).integers(-1, 5, Rn).astype(np.int32)          # a remap that holds -1
    for kw_ref, kw_dev in ((dict(row_base=rb, remap=remap), dict(row_base=rb, remap=_dev(remap))), (dict(row_base=rb), dict(row_base=rb)), ({}, {})):
        for min_votes in (1, 2):
            want = FR.vote(xyz, cams, keys, labels, tau, min_votes=min_votes, **kw_ref)
            got = ops.fuse_vote(dx, cameras, dk, dl, tau, min_votes=min_votes, **kw_dev)
            for k, g in zip(VOTE_KEYS, got):
                assert np.array_equal(g.cpu().numpy(), want[k]), (k, sorted(kw_ref), min_votes)
    K = 5
    lb, la = ops.label_bits(got[0], K)
    want_lb, want_la = FR.label_bits(want["label"], K)
    assert np.array_equal(lb.cpu().numpy(), want_lb) and np.array_equal(la.cpu().numpy(), want_la)
    return want_area


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.fixture(scope="module")
def ten_frames():
    """Ten patterned frames of 24 x 43 and their scan, computed once and never modified."""
    depth, rgb, cams, far = R.pattern_case(10, 24, 43)
    xyz, ncams, keys = FR.frames_case(depth, rgb, cams, far)
    labels = FR.pattern_labels(depth.shape, 3)
    for a in (xyz, keys, labels):
        a.setflags(write=False)
    return xyz, ncams, keys, labels


@pytest.mark.parametrize("Vn", [1, 2, 10])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 1025])
def test_sizes_against_the_reference(ops, ten_frames, N, Vn):
    """N: a wave's tail (63, 65), no tail bits (64), a block's tail (257 = one block of four words and one wave), more than one block (1025)."""
    xyz, ncams, keys, labels = ten_frames
    pick = np.linspace(0, len(xyz) - 1, N).astype(np.int64) if N > 1 else np.array([len(xyz) // 3])      # points of every frame
    counts = np.array([3, 0, 4, 2, 3, 3, 1, 3, 0, 5][:Vn])          # views with no region, with fewer and with more regions than labels
    rb = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    _check_all(ops, np.ascontiguousarray(xyz[pick]), ncams[:Vn], keys[:Vn], labels[:Vn], rb, 0.01, seed=N + Vn)


@pytest.mark.parametrize("shape, dead", [((3, 5, 13), None), ((2, 24, 43), None), ((3, 5, 13), 1)])
def test_pattern_shapes_and_a_dead_frame(ops, shape, dead):
    depth, rgb, cams, far = R.pattern_case(*shape, dead_frame=dead)
    xyz, ncams, keys = FR.frames_case(depth, rgb, cams, far)
    if dead is not None:
        assert (keys[dead] == V.EMPTY).all()
    labels = FR.pattern_labels(shape, 4)
    rb = np.arange(shape[0] + 1, dtype=np.int32) * 4
    area = _check_all(ops, xyz, ncams, keys, labels, rb, 0.0)
    assert area[int(rb[-1]):].sum() > 0 and (dead is None or area[int(rb[-1]) + dead] == 0)


@pytest.mark.parametrize("tau", [0.0, 0.05])
def test_room_fixture(ops, tau):
    depth, rgb, cams, far = R.room_case()
    xyz, ncams, keys = FR.frames_case(depth, rgb, cams, far)
    labels = FR.pattern_labels(depth.shape, 6)
    area = _check_all(ops, xyz, ncams, keys, labels, np.array([0, 6, 12], dtype=np.int32), tau)
    assert (area[12:] >= R.ROOM_KEPT // 2 - 200).all()              # every frame sees (nearly all of) its own points


def test_nan_and_infinite_coordinates(ops):
    pts, expected = V.hand_points()
    cams = [V.Cam(), V.Cam(pose=V.ROTATED)]
    keys = np.stack([V.splat(pts, c, 1) for c in cams])
    labels = FR.pattern_labels((2, 96, 128), 3)
    area = _check_all(ops, pts, cams, keys, labels, np.array([0, 3, 6], dtype=np.int32), 0.0)
    assert 1 <= area[6] <= sum(e is not None for e in expected)    # no point that is out of view is visible


# ------------------------------------------------------------------------------------------------ vote edge cases
def _one_point_views(labels):
    cam = V.Cam()
    xyz = np.array([[0.0, 0.0, -2.0]], dtype=np.float32)
    keys = np.stack([V.splat(xyz, cam, 0)] * len(labels))
    lab = np.stack([np.full((cam.height, cam.width), l, dtype=np.int32) for l in labels])
    return xyz, [cam] * len(labels), keys, lab


def _vote1(ops, case, **kw):
    xyz, cams, keys, lab = case
    return tuple(int(t.item()) for t in ops.fuse_vote(_dev(xyz), [_camera(c) for c in cams], _dev(keys), _dev(lab), 0.0, **kw))


def test_vote_ties_min_votes_and_unlabelled_observations(ops):
    case = _one_point_views([7, 3, 7, 3])
    assert _vote1(ops, case) == (3, 2, 4, 4, 0)                     # the lower label, though 7 was seen first
    assert _vote1(ops, case, min_votes=3) == (-1, 0, 4, 4, 0)
    assert _vote1(ops, _one_point_views([7, 3, 7])) == (7, 2, 3, 3, 0)
    case = _one_point_views([-1, 2, I32.max, I32.min, 1])
    rb = [0, 2, 4, 6, 8, 10]
    assert _vote1(ops, case, row_base=rb) == (1, 1, 5, 1, 0)        # -1, count_v, INT32_MAX, INT32_MIN: seen, not labelled
    assert _vote1(ops, case) == (1, 1, 5, 3, 0)                     # consistent ids: 2 and INT32_MAX are labels too
    assert _vote1(ops, case, row_base=rb, remap=_dev(np.array([5, -1] * 5, dtype=np.int32))) == (-1, 0, 5, 0, 0)
    assert _vote1(ops, case, row_base=rb, remap=_dev(np.array([5, 9] * 5, dtype=np.int32))) == (9, 1, 5, 1, 0)
    assert _vote1(ops, case, row_base=[0, 0, 0, 0, 0, 2]) == (1, 1, 5, 1, 0)      # views without a region


def test_vote_overflow_ten_identical_frames(ops):
    depth, rgb, cams, far = FR.tiled_room(10)
    xyz, ncams, keys = FR.frames_case(depth, rgb, cams, far)
    lab = np.stack([np.full(depth.shape[1:], v, dtype=np.int32) for v in range(10)])
    label, votes, seen, labelled, dropped = ops.fuse_vote(_dev(xyz), [_camera(c) for c in ncams], _dev(keys), _dev(lab), 0.0)
    assert len(xyz) == 10 * (R.ROOM_KEPT // 2)
    assert (seen == 10).all() and (labelled == 10).all() and (dropped == 2).all() and (label == 0).all() and (votes == 1).all()
    label, votes, _, _, dropped = ops.fuse_vote(_dev(xyz), [_camera(c) for c in ncams], _dev(keys), _dev(lab[::-1]), 0.0)      # 9 first: 9 .. 2 stay
    assert (label == 2).all() and (votes == 1).all() and (dropped == 2).all()


# ------------------------------------------------------------------------------------------------ the ring fixture, end to end
@pytest.fixture(scope="module")
def ring():
    case = FR.ring_case()
    case["want"] = FR.fuse(case["xyz"], case["cams"], case["keys"], case["labels"], FR.RING_TAU, 0.5, 20)
    for v in list(case.values()) + list(case["want"].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@pytest.fixture(scope="module")
def predictor(ops):
    from point_sam_amd.model import PointCloudSAM
    from point_sam_amd.predictor import PointSAMPredictor
    cfg = get_config("tiny")
    return PointSAMPredictor(PointCloudSAM(cfg, random_state_dict(cfg, 3), "cuda", precision="f16x3"))


@pytest.mark.parametrize("working", [None, 4096], ids=["scan", "working4096"])
def test_ring_fixture_through_the_predictor(ops, predictor, ring, working):
    """Links on the scan itself (max_points >= M), and links on a voxel working cloud of at most 4096 points (3130 here) with the vote on every point of
    the scan.  Both equal the reference on the same link cloud in every output, and both meet the fixture's conditions: 4 instances, at most 0.1 % of
    the 30493 points with an instance other than their object's (the reference has 8 such points either way)."""
    import scene_reference as S
    from point_sam_amd.fusion import FusionConfig
    M = len(ring["xyz"])
    # the reference's own centre and scale: with them passed in, the scan equals the reference's word for word
    fs = predictor.set_frames(ring["depth"].copy(), ring["rgb"].copy(), [_camera(c) for c in ring["cameras"]], ring["far"], edge=ring["edge"],
                              center=ring["center"].copy(), scale=float(ring["scale"]), max_points=working or M)
    assert fs.num_points == M and np.array_equal(fs.xyz.cpu().numpy(), ring["xyz"]) and np.array_equal(fs.keys.cpu().numpy().view(np.uint64), ring["keys"])
    sc = predictor.scene
    assert sc.identity == (working is None) and sc.num_working <= (working or M)
    if working is None:
        want = ring["want"]
    else:
        keep = S.downsample(ring["xyz"], sc.voxel_size)[0]
        assert np.array_equal(sc.keep_idx.cpu().numpy(), keep) and len(keep) < M // 4
        want = FR.fuse(ring["xyz"], ring["cams"], ring["keys"], ring["labels"], FR.RING_TAU, 0.5, 20, link_xyz=ring["xyz"][keep])
    fused = predictor.fuse_labels(fs, ring["labels"].copy(), FusionConfig(FR.RING_TAU))
    label, remap = fused.labels.cpu().numpy(), fused.remap.cpu().numpy()
    wrong = FR.ring_disagreement(label, remap, fused.row_base, ring["perm"], ring["obj"])
    print(f"ring, working cloud {sc.num_working}: instances {fused.num_instances}, disagree {wrong} of {M}")
    assert fused.num_instances == 4 and tuple(label.shape) == (M,)
    assert wrong <= 0.001 * M
    assert np.array_equal(remap, want["remap"]) and np.array_equal(fused.row_base, want["row_base"])
    for k, t in zip(VOTE_KEYS, (fused.labels, fused.votes, fused.seen, fused.labelled, fused.dropped)):
        assert np.array_equal(t.cpu().numpy(), want[k]), k
    # the fused instances as packed rows: their popcounts are the labels' histogram, and mask_geometry takes them
    bits, area = fused.bits()
    hist = np.bincount(label[label >= 0], minlength=4)
    assert tuple(bits.shape) == (4, (M + 63) // 64) and np.array_equal(area.cpu().numpy(), hist)
    assert np.array_equal(ops.mask_unpack(bits, M).sum(1).cpu().numpy(), hist)
    geo = predictor.mask_geometry(bits)
    assert np.array_equal(geo.count.cpu().numpy(), hist) and bool(geo.valid.all())
    one, a1 = fused.bits([2])
    assert torch.equal(one, bits[2:3]) and torch.equal(a1, area[2:3])
    # a list of the frames' views is the FrameSet; consistent ids vote without links
    again = predictor.fuse_labels(list(fs.views), _dev(ring["labels"]), FusionConfig(FR.RING_TAU))
    assert torch.equal(again.labels, fused.labels) and torch.equal(again.remap, fused.remap)
    if working is None:
        glob = np.where(ring["labels"] >= 0, np.take_along_axis(np.argsort(ring["perm"], 1), np.maximum(ring["labels"], 0).reshape(6, -1), 1).reshape(6, 96, 128), -1)
        cons = predictor.fuse_labels(fs, glob.astype(np.int32), FusionConfig(FR.RING_TAU), consistent=True)
        ref = FR.vote(ring["xyz"], ring["cams"], ring["keys"], glob.astype(np.int32), FR.RING_TAU)
        assert cons.num_instances == 4 and cons.remap is None and np.array_equal(cons.labels.cpu().numpy(), ref["label"])
        assert (cons.labels.cpu().numpy() != ring["obj"]).sum() <= 0.001 * M


# ------------------------------------------------------------------------------------------------ reproducibility and refusals
def test_two_runs_and_another_stream_give_the_same_bits(ops):
    depth, rgb, cams, far = R.room_case()
    xyz, ncams, keys = FR.frames_case(depth, rgb, cams, far)
    labels = FR.pattern_labels(depth.shape, 6)
    cameras, rb = [_camera(c) for c in ncams], [0, 6, 12]
    dx, dk, dl = _dev(xyz), _dev(keys), _dev(labels)

    def run():
        bits, area = ops.fuse_region_bits(dx, cameras, dk, dl, rb, 0.02)
        return (bits, area) + ops.fuse_vote(dx, cameras, dk, dl, 0.02, rb) + ops.label_bits(dl.reshape(-1)[:len(xyz)].contiguous(), 6)
    first, second = run(), run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    for a, b, c in zip(first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_entry_points_refuse_bad_arguments_and_launch_nothing(ops):
    lib = _lib.load()
    buf = torch.full((1 << 13,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert buf.data_ptr() % 16 == 0
    FR.entry_point_refusals(lib, buf.data_ptr())
    torch.cuda.synchronize()
    assert bool((buf == 0x5A5A5A5A5A5A5A5A).all())                  # device memory every refused call was handed: untouched
