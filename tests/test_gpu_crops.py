"""Scene crops on the GPU (csrc/crops.hip, point_sam_amd/scene.py: build_crop, predictor.set_crop, multi-crop proposals).  Every output is an integer, a
bit, a bit-for-bit copy or an fp32 value of individually rounded operations, so every comparison is equality -- against the plain numpy reference in
tests/crop_reference.py and against the existing set_pointcloud / predict_masks / generate_masks on the reference-built crop cloud."""
import numpy as np
import pytest
import torch

import crop_reference as C
import scene_reference as R
from oracle import pointsam_oracle as O
from point_sam_amd.config import get_config
from point_sam_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu
f32 = np.float32
NEG_INF = f32(-np.inf)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd import ops
    return ops


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_crop(ops, xyz, rgb, center, radius, h):
    want_keep, want_inv, want_xyz, want_rgb, want_members = C.crop_downsample(xyz, rgb, center, radius, h)
    dx, dr = torch.from_numpy(np.ascontiguousarray(xyz, dtype=f32)).cuda(), torch.from_numpy(np.ascontiguousarray(rgb, dtype=f32)).cuda()
    keep_idx, inv, wxyz, wrgb, members = ops.crop_downsample(dx, dr, center, radius, h)
    assert keep_idx.dtype == torch.int64 and inv.dtype == torch.int64 and keep_idx.is_contiguous() and wxyz.is_contiguous() and wrgb.is_contiguous()
    assert members == want_members and keep_idx.numel() == len(want_keep), (members, want_members, keep_idx.numel(), len(want_keep))
    assert np.array_equal(keep_idx.cpu().numpy(), want_keep)
    assert np.array_equal(inv.cpu().numpy(), want_inv)
    assert tuple(wxyz.shape) == (len(want_keep), 3) and tuple(wrgb.shape) == (len(want_keep), 3)
    assert np.array_equal(_bits(wxyz.cpu().numpy()), _bits(want_xyz))
    assert np.array_equal(_bits(wrgb.cpu().numpy()), _bits(want_rgb))
    assert ops.crop_count(dx, center, radius, h) == (len(want_keep), want_members)      # the count-only mode agrees with the full mode
    return keep_idx, inv, wxyz, wrgb, members


# ------------------------------------------------------------------------------------------------ 1. downsample against the reference
BALL = ((0.1, -0.2, 0.05), 0.6)


@pytest.mark.parametrize("h", [0.2, None])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 1025, 4097])
def test_crop_downsample_sizes_around_wave_block_and_second_level(ops, M, h):
    """One point; one short of, exactly and one past a wave; one past a scan block of 1024; five blocks (second-level offsets).  About a tenth of the
    uniform points lie in the ball; at h = 0.2 (crop units, no power of two) many members share a voxel with an earlier one.  h None: every member
    is a point of the crop cloud."""
    rng = np.random.default_rng(100 + M)
    xyz = rng.uniform(-1, 1, (M, 3)).astype(f32)
    if M == 1:
        xyz[0] = (0.2, -0.1, 0.0)                         # the single point is a member
    rgb = rng.uniform(-1, 1, (M, 3)).astype(f32)
    keep_idx, inv, _, _, members = _check_crop(ops, xyz, rgb, *BALL, h)
    assert M < 65 or 0 < members < M
    if h is None:
        assert keep_idx.numel() == members
    else:
        assert M < 1025 or keep_idx.numel() < members


@pytest.mark.parametrize("h", [0.05, 2.0])
@pytest.mark.parametrize("M", [65, 1025])
def test_crop_downsample_of_the_unit_ball_equals_voxel_downsample(ops, M, h):
    """The two downsamples share the table and the scan (csrc/voxel_table.h), so they agree where their definitions coincide: centre 0 and radius 1
    make x - 0 and x * 1 exact, points of [-0.55, 0.55]^3 have q <= 0.9075 (all members, the clamp idle), and both grids start at -1.  Then
    keep_idx and inv are voxel_downsample's, wxyz = xyz[keep_idx] and wrgb = rgb[keep_idx] bit for bit.  M = 65: a wave and one lane; 1025: two
    scan blocks.  h = 2: one voxel.  Point 5 repeats point 2 and one coordinate is -0.0.  (tests/scene_reference.py and tests/crop_reference.py
    agree bit for bit on these inputs: the statement holds for the definitions, not only for the kernels.)"""
    rng = np.random.default_rng(700 + M)
    xyz = rng.uniform(-0.55, 0.55, (M, 3)).astype(f32)
    xyz[5] = xyz[2]
    xyz[7, 1] = f32(-0.0)
    rgb = rng.uniform(-1, 1, (M, 3)).astype(f32)
    assert float(((xyz.astype(np.float64)) ** 2).sum(1).max()) <= 0.9075 and np.signbit(xyz[7, 1])
    dx, dr = torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda()
    want_keep, want_inv = ops.voxel_downsample(dx, h)
    keep_idx, inv, wxyz, wrgb, members = ops.crop_downsample(dx, dr, (0.0, 0.0, 0.0), 1.0, h)
    assert members == M
    assert torch.equal(keep_idx, want_keep) and torch.equal(inv, want_inv)
    assert int(inv[5]) == int(inv[2]) and (h < 2.0 or keep_idx.tolist() == [0])
    keep = keep_idx.cpu().numpy()
    assert np.array_equal(_bits(wxyz.cpu().numpy()), _bits(xyz[keep]))
    assert np.array_equal(_bits(wrgb.cpu().numpy()), _bits(rgb[keep]))


# ------------------------------------------------------------------------------------------------ 2. boundary and ordering cases
def test_membership_is_exact_on_the_sphere_and_non_finite_points_are_outside(ops):
    """c = 0, r = 0.5: every operation is exact, so (0.5, 0, 0) and (0, -0.5, 0) lie ON the sphere and are members (q == r2), and the next float
    after 0.5 on an axis is not.  A NaN and an inf point are non-members, not errors."""
    up = np.nextafter(f32(0.5), f32(1))
    xyz = np.array([[0.5, 0, 0], [0, -0.5, 0], [up, 0, 0], [0, 0, -up], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, 0], [-np.inf, np.nan, 0.1]], dtype=f32)
    rgb = np.arange(24, dtype=f32).reshape(8, 3)
    for h in (None, 0.25):
        keep_idx, inv, wxyz, _, members = _check_crop(ops, xyz, rgb, (0.0, 0.0, 0.0), 0.5, h)
        assert members == 3 and keep_idx.tolist() == [0, 1, 6] and inv.tolist() == [0, 1, -1, -1, -1, -1, 2, -1]
        assert wxyz.cpu().numpy().tolist() == [[1, 0, 0], [0, -1, 0], [0, 0, 0]]


def test_the_representative_of_a_voxel_is_a_member(ops):
    """Points 0 and 1 share a voxel of the crop grid; point 0 (the lowest index in that cell) lies outside the ball, point 1 inside: the
    representative is point 1.  An implementation that voxelises before it selects keeps point 0 and loses the voxel."""
    center, r, h = (0.0, 0.0, 0.0), 0.5, 0.5              # crop cells of half a unit: scan cells of 0.25 from -0.5
    xyz = np.array([[0.49, 0.49, 0.01], [0.26, 0.26, 0.01], [0.27, 0.3, 0.2], [-0.1, 0.0, 0.0]], dtype=f32)
    rgb = np.zeros((4, 3), dtype=f32)
    _, q, member = C.ball(xyz, center, r)
    assert member.tolist() == [False, True, True, True]
    u = C.normalise(C.ball(xyz, center, r)[0], r)
    cells = np.floor((u + 1) / 0.5)
    assert np.array_equal(cells[0], cells[1]) and np.array_equal(cells[1], cells[2])      # one voxel, first entered by a non-member
    keep_idx, inv, _, _, _ = _check_crop(ops, xyz, rgb, center, r, h)
    assert keep_idx.tolist() == [1, 3] and inv.tolist() == [-1, 0, 0, 1]


def test_one_point_4096_times(ops):
    xyz = np.tile(np.array([[0.3, -0.1, 0.1]], dtype=f32), (4096, 1))
    rgb = np.random.default_rng(1).uniform(-1, 1, (4096, 3)).astype(f32)
    keep_idx, inv, _, wrgb, members = _check_crop(ops, xyz, rgb, *BALL, 0.05)
    assert members == 4096 and keep_idx.tolist() == [0] and int(inv.max()) == 0 and int(inv.min()) == 0
    assert np.array_equal(_bits(wrgb.cpu().numpy()), _bits(rgb[:1]))
    keep_idx, inv, _, _, _ = _check_crop(ops, xyz, rgb, *BALL, None)
    assert torch.equal(keep_idx, torch.arange(4096, device="cuda")) and torch.equal(inv, keep_idx)


def test_a_ball_with_every_point_and_a_ball_with_none(ops):
    from point_sam_amd.scene import build_crop
    rng = np.random.default_rng(5)
    xyz = rng.uniform(-0.5, 0.5, (3000, 3)).astype(f32)
    rgb = rng.uniform(-1, 1, (3000, 3)).astype(f32)
    _, inv, _, _, members = _check_crop(ops, xyz, rgb, (0.0, 0.0, 0.0), 1.0, 0.1)
    assert members == 3000 and int(inv.min()) >= 0
    keep_idx, inv, wxyz, wrgb, members = _check_crop(ops, xyz, rgb, (3.0, 0.0, 0.0), 0.25, 0.1)
    assert members == 0 and keep_idx.numel() == 0 and wxyz.shape[0] == 0 and wrgb.shape[0] == 0 and int(inv.max()) == -1
    dx, dr = torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda()
    with pytest.raises(ValueError, match="no point"):
        build_crop(dx, dr, (3.0, 0.0, 0.0), 0.25, voxel_size=0.1)
    with pytest.raises(ValueError, match="no point"):
        build_crop(dx, dr, (3.0, 0.0, 0.0), 0.25, max_points=100)
    for bad in ((float("nan"), 0.0, 0.0), (0.0, float("inf"), 0.0)):
        with pytest.raises(ValueError, match="center"):
            ops.crop_downsample(dx, dr, bad, 0.5)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="radius"):
            ops.crop_count(dx, (0.0, 0.0, 0.0), bad)
    with pytest.raises(ValueError, match="2\\^21"):      # (u + 1) / 2^-21 = 2^21 at u = 0: one past the last cell
        ops.crop_downsample(dx, dr, (float(xyz[0, 0]), float(xyz[0, 1]), float(xyz[0, 2])), 0.5, 2.0 ** -21)
    _check_crop(ops, xyz, rgb, (0.0, 0.0, 0.0), 1.0, 0.1)      # the flag was cleared


def test_a_member_whose_normalised_coordinate_rounds_above_one_is_clamped(ops):
    """With inv_r = fl32(1) / fl32(r), as ops computes it, r * inv_r never rounds above 1 (tests/test_crops_cpu.py checks every fp32 mantissa), and a
    member has |d| <= r on every axis.  The C entry takes inv_r from its caller, though: one ulp above the quotient, the member (r, 0, 0) (q == r2
    exactly) has d * inv_r = the float after 1, and the clamp returns exactly 1 -- the crop cloud never trips the model's coordinate-range check."""
    import ctypes
    from point_sam_amd import _lib
    r = f32(0.75)
    inv_r = np.nextafter(f32(1) / r, f32(np.inf))
    assert f32(r * inv_r) > f32(1)
    xyz = np.array([[r, 0, 0], [0, -r, 0], [0.1, 0.1, -0.2], [0, 0, np.nextafter(r, f32(1))]], dtype=f32)
    dx, dr = torch.from_numpy(xyz).cuda(), torch.zeros(4, 3, device="cuda")
    lib = _lib.load()
    ws = torch.empty(lib.psam_crop_downsample_workspace_bytes(4) // 8 + 2, dtype=torch.int64, device="cuda")
    keep_idx, inv = torch.full((4,), -7, dtype=torch.int64, device="cuda"), torch.full((4,), -7, dtype=torch.int64, device="cuda")
    wxyz, wrgb, res = torch.full((4, 3), 9.0, device="cuda"), torch.full((4, 3), 9.0, device="cuda"), torch.full((3,), 9, dtype=torch.int32, device="cuda")
    center = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    st = lib.psam_crop_downsample(dx.data_ptr(), dr.data_ptr(), 4, ctypes.addressof(center), float(r * r), float(inv_r), 0.0, keep_idx.data_ptr(),
                                  inv.data_ptr(), wxyz.data_ptr(), wrgb.data_ptr(), res.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                  torch.cuda.current_stream().cuda_stream)
    assert st == 0
    assert res.tolist() == [3, 3, 0] and keep_idx.tolist() == [0, 1, 2, -7] and inv.tolist() == [0, 1, 2, -1]
    got = wxyz.cpu().numpy()
    assert got[0].tolist() == [1, 0, 0] and got[1].tolist() == [0, -1, 0] and (got[3] == 9).all()
    assert np.array_equal(_bits(got[2]), _bits((xyz[2] * inv_r).astype(f32)))
    # and through ops (inv_r the quotient): the same member sits at exactly 1 without the clamp's help
    _, _, wxyz, _, _ = _check_crop(ops, xyz, np.zeros((4, 3), dtype=f32), (0.0, 0.0, 0.0), float(r), None)
    assert np.abs(wxyz.cpu().numpy()).max() == f32(1)


# ------------------------------------------------------------------------------------------------ 3. expand rows / bits
def _inv_cases(M, Nw, rng):
    """inv [M] with whole 64-point words of -1, mixed words, and all -1."""
    mixed = rng.integers(0, Nw, M)
    mixed[rng.random(M) < 0.5] = -1
    words_off = rng.integers(0, Nw, M)
    for w in range(0, (M + 63) // 64, 2):                 # every other 64-point word entirely off the ball
        words_off[w * 64:(w + 1) * 64] = -1
    if M > 64:
        words_off[64:72] = -1                             # and a mixed word next to them
    return {"mixed": mixed, "words": words_off, "none": np.full(M, -1, dtype=np.int64)}


@pytest.mark.parametrize("Nw", [1, 65])
@pytest.mark.parametrize("M", [1, 64, 65, 4097])
def test_crop_expand_rows_and_bits_equal_numpy(ops, M, Nw):
    rng = np.random.default_rng(M * 131 + Nw)
    for name, inv in _inv_cases(M, Nw, rng).items():
        inv = inv.astype(np.int64)
        dinv = torch.from_numpy(inv).cuda()
        for K in (1, 3):
            # rows: f32 with fill -inf, int32 with fill -1; source and destination with row strides wider than the rows
            src = rng.normal(0, 1, (K, Nw)).astype(f32)
            src[0, 0] = np.nan
            lab = rng.integers(-1, 9, (K, Nw)).astype(np.int32)
            want = C.expand_rows(src, inv, NEG_INF)
            got = ops.crop_expand_rows(torch.from_numpy(src).cuda(), dinv, float("-inf"))
            assert got.dtype == torch.float32 and tuple(got.shape) == (K, M), name
            assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), name
            assert np.isneginf(got.cpu().numpy()[:, inv < 0]).all()
            got = ops.crop_expand_rows(torch.from_numpy(lab).cuda(), dinv, -1)
            assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), C.expand_rows(lab, inv, np.int32(-1))), name
            wide = torch.full((K + 2, Nw + 11), 7.5, device="cuda")
            wide[1:1 + K, 3:3 + Nw] = torch.from_numpy(src).cuda()
            buf = torch.full((K + 2, M + 5), -3.0, device="cuda")
            out = buf[1:1 + K, 2:2 + M]
            assert ops.crop_expand_rows(wide[1:1 + K, 3:3 + Nw], dinv, float("-inf"), out=out) is out
            full = buf.cpu().numpy()
            assert np.array_equal(_bits(full[1:1 + K, 2:2 + M]), _bits(want)), name
            full[1:1 + K, 2:2 + M] = -3.0
            assert (full == -3.0).all(), "words outside the destination range were written"
            # bits
            masks = rng.random((K, Nw)) < 0.6
            masks[0] = True
            ww = R.words(masks)
            want_bits, want_area = C.expand_bits(ww, inv, Nw)
            bits, area = ops.crop_expand_bits(torch.from_numpy(ww.view(np.int64)).cuda(), dinv, Nw)
            got = bits.cpu().numpy().view(np.uint64)
            assert got.shape == (K, (M + 63) // 64) and np.array_equal(got, want_bits), name
            if M % 64:
                assert (got[:, -1] >> np.uint64(M % 64)).max() == 0, "bits past M must be zero"
            assert area.dtype == torch.int32 and np.array_equal(area.cpu().numpy(), want_area), name
            assert int(area[0]) == int((inv >= 0).sum())                     # the areas are the popcounts: row 0 is the whole ball
            assert np.array_equal(area.cpu().numpy(), R.unwords(got, M).sum(1))
            bits2, none = ops.crop_expand_bits(torch.from_numpy(ww.view(np.int64)).cuda(), dinv, Nw, area=False)
            assert none is None and torch.equal(bits2, bits)


# ------------------------------------------------------------------------------------------------ 4. the predictor under a crop
M_SCAN = 20000
SCENE_POINTS = 2048
CENTER, RADIUS, CROP_VOXEL = (0.1, -0.1, 0.05), 0.38, 0.1      # about 3 000 of the 20 000 points; cells of a tenth of the ball's radius


@pytest.fixture(scope="module")
def scan(ops):
    from point_sam_amd.model import PointCloudSAM
    cfg = get_config("tiny")
    model = PointCloudSAM(cfg, random_state_dict(cfg, 3), "cuda", precision="f16x3")
    xyz, rgb, _, _ = O.synthetic_batch(1, M_SCAN, seed=8)
    xyz_np, rgb_np = xyz[0].numpy(), rgb[0].numpy()
    ref = C.crop_downsample(xyz_np, rgb_np, CENTER, RADIUS, CROP_VOXEL)
    assert 2500 <= ref[4] <= 3500 and 400 <= len(ref[0]) < ref[4], (ref[4], len(ref[0]))
    inside = np.nonzero(ref[1] >= 0)[0]
    clicks = xyz[0, [int(inside[5]), int(inside[1200])]].cuda()[None]      # [1, 2, 3]: two points of the scan inside the ball
    outside = xyz[0, int(np.nonzero(ref[1] < 0)[0][0])].cuda()[None, None]
    return model, xyz[0].cuda().contiguous(), rgb[0].cuda().contiguous(), xyz_np, ref, clicks, outside


def _two_clicks(pred, clicks, pick=lambda full: full, transform=lambda p: p):
    """The demo's loop: click 1 multimask, click 2 with the best mask's logits as the dense prompt."""
    one = torch.ones(1, 1, dtype=torch.int64, device="cuda")
    clicks = transform(clicks)
    m1, s1, l1 = pred.predict_masks(clicks[:, :1], one, None, True)
    best = torch.argmax(s1[0])
    m2, s2, l2 = pred.predict_masks(clicks, torch.cat([one, 1 - one], 1), pick(l1[0][best][None]), False)
    return (l1, s1), (l2, s2)


def _ref_cloud(ref):
    return torch.from_numpy(ref[2]).cuda()[None].contiguous(), torch.from_numpy(ref[3]).cuda()[None].contiguous()


def test_predict_masks_under_a_crop_is_the_crop_clouds_expanded(ops, scan):
    from point_sam_amd.predictor import PointSAMPredictor
    model, xyz, rgb, xyz_np, ref, clicks, outside = scan
    keep, inv = ref[0], ref[1]
    pred = PointSAMPredictor(model)
    pred.set_scene(xyz, rgb, max_points=SCENE_POINTS)
    before = _two_clicks(pred, clicks)
    scene_state = pred._state
    pred.set_crop(CENTER, RADIUS, voxel_size=CROP_VOXEL)
    crop = pred.crop
    assert (crop.num_points, crop.num_members, crop.num_working, crop.voxel_size) == (M_SCAN, ref[4], len(keep), CROP_VOXEL)
    assert crop.center == tuple(float(f32(v)) for v in CENTER) and crop.radius == float(f32(RADIUS))
    assert np.array_equal(crop.keep_idx.cpu().numpy(), keep) and np.array_equal(crop.inv.cpu().numpy(), inv)
    assert np.array_equal(_bits(pred._crop_state.coords[0].cpu().numpy()), _bits(ref[2]))      # the crop cloud is the reference's, bit for bit
    assert pred._state is scene_state
    work = PointSAMPredictor(model)
    work.set_pointcloud(*_ref_cloud(ref))
    to_crop = lambda p: torch.from_numpy(C.crop_prompts(p.cpu().numpy(), CENTER, RADIUS)).cuda()
    want = _two_clicks(work, clicks, transform=to_crop)
    got = _two_clicks(pred, clicks)                        # click 2 hands the scan-width logits back, as the demo does: they round-trip
    off = torch.from_numpy(inv < 0).cuda()
    for (gl, gs), (wl, ws) in zip(got, want):
        assert tuple(gl.shape) == (1, wl.shape[1], M_SCAN)
        full = C.expand_rows(wl[0].cpu().numpy(), inv, NEG_INF)
        assert np.array_equal(_bits(gl[0].cpu().numpy()), _bits(full)) and torch.equal(gs, ws)
        assert bool(torch.isneginf(gl[0][:, off]).all()) and bool(torch.isfinite(gl[0][:, ~off]).all())
    narrow = _two_clicks(pred, clicks, pick=lambda full: full[:, torch.from_numpy(keep).cuda()])      # a prompt mask of the crop's width is taken as it is
    assert torch.equal(narrow[1][0], got[1][0])
    with pytest.raises(ValueError, match="outside the crop"):
        pred.predict_masks(outside, torch.ones(1, 1, dtype=torch.int64, device="cuda"), None, True)
    with pytest.raises(ValueError, match="width"):
        pred.predict_masks(clicks, torch.ones(1, 2, dtype=torch.int64, device="cuda"), torch.zeros(1, M_SCAN - 1, device="cuda"), False)
    # back to the whole scene: nothing is encoded, and the answers are the earlier ones bit for bit
    calls = []
    encode = model.encode
    model.encode = lambda *a, **k: calls.append(1) or encode(*a, **k)
    try:
        pred.clear_crop()
        assert pred.crop is None and pred._state is scene_state
        after = _two_clicks(pred, clicks)
        pred.set_crop(CENTER, RADIUS, voxel_size=CROP_VOXEL)      # the last crop is cached
        again = _two_clicks(pred, clicks)
    finally:
        model.encode = encode
    assert calls == []
    for (al, as_), (bl, bs) in zip(after, before):
        assert torch.equal(al, bl) and torch.equal(as_, bs)
    for (al, as_), (bl, bs) in zip(again, got):
        assert torch.equal(al, bl) and torch.equal(as_, bs)
    pred.set_scene(xyz, rgb, max_points=SCENE_POINTS)      # set_scene drops the crop
    assert pred.crop is None


def _proposal_config(work, clicks_crop):
    from point_sam_amd.proposals import ProposalConfig
    logits, _, _ = work.predict_masks(clicks_crop[:, :1], torch.ones(1, 1, dtype=torch.int64, device="cuda"), None, True)
    return ProposalConfig(num_prompts=32, prompt_chunk=16, mask_threshold=float(logits.median()), pred_iou_thresh=float("-inf"), stability_thresh=0.0,
                          min_points=1, max_area_frac=1.0001)


def test_generate_and_clean_masks_under_a_crop_are_the_crop_clouds_expanded(ops, scan):
    from point_sam_amd.predictor import PointSAMPredictor
    from point_sam_amd.regions import RegionConfig
    model, xyz, rgb, xyz_np, ref, clicks, outside = scan
    keep, inv = ref[0], ref[1]
    work = PointSAMPredictor(model)
    work.set_pointcloud(*_ref_cloud(ref))
    clicks_crop = torch.from_numpy(C.crop_prompts(clicks.cpu().numpy(), CENTER, RADIUS)).cuda()
    pc = _proposal_config(work, clicks_crop)
    want = work.generate_masks(pc)[0]
    assert len(want) >= 1 and want.n_points == len(keep)
    pred = PointSAMPredictor(model)
    pred.set_scene(xyz, rgb, max_points=SCENE_POINTS)
    pred.set_crop(CENTER, RADIUS, voxel_size=CROP_VOXEL)
    got = pred.generate_masks(pc)
    assert len(got) == 1
    got = got[0]
    bits, area = C.expand_bits(want.bits.cpu().numpy().view(np.uint64), inv, len(keep))
    assert got.n_points == M_SCAN and len(got) == len(want) and got.crop_index is None
    assert got.labels.dtype == torch.int32 and np.array_equal(got.labels.cpu().numpy(), C.expand_rows(want.labels.cpu().numpy()[None], inv, np.int32(-1))[0])
    assert (got.labels.cpu().numpy()[inv < 0] == -1).all()
    assert np.array_equal(got.bits.cpu().numpy().view(np.uint64), bits)
    assert not R.unwords(got.bits.cpu().numpy().view(np.uint64), M_SCAN)[:, inv < 0].any()
    assert np.array_equal(got.area.cpu().numpy(), area) and got.area.dtype == torch.int32
    for name in ("score", "candidate", "prompt_index", "stability"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    # clean_masks: scan-width logits are reduced to the crop cloud, cleaned there (with the clicks moved into the crop) and expanded
    one = torch.ones(1, 2, dtype=torch.int64, device="cuda")
    rc = RegionConfig(min_island=5, min_hole=5, keep_clicked=True)
    wl, _, _ = work.predict_masks(clicks_crop, one, None, True)
    gl, _, _ = pred.predict_masks(clicks, one, None, True)
    thr = float(wl.median())
    wb, wa, wc = work.clean_masks(wl, rc, clicks_crop, one, threshold=thr)
    gb, ga, gc = pred.clean_masks(gl, rc, clicks, one, threshold=thr)
    eb, ea = C.expand_bits(wb.cpu().numpy().view(np.uint64), inv, len(keep))
    assert np.array_equal(gb.cpu().numpy().view(np.uint64), eb) and np.array_equal(ga.cpu().numpy(), ea) and torch.equal(gc, wc)
    pred.clear_crop()                                      # the graph cache is keyed on the crop: the scene's own clean-up builds its own graph
    sl, _, _ = pred.predict_masks(clicks, one, None, True)
    sb, _, _ = pred.clean_masks(sl, rc, clicks, one, threshold=thr)
    assert tuple(sb.shape) == (sl.shape[1], (M_SCAN + 63) // 64)


# ------------------------------------------------------------------------------------------------ 5. multi-crop proposals
def test_shell_rule_on_hand_made_bits(ops):
    """One mask with a single point in the shell is dropped; its copy without that point is kept."""
    from point_sam_amd.scene import Crop, crop_shell_bits
    rng = np.random.default_rng(9)
    r, edge = 0.5, 0.1
    dirs = rng.normal(0, 1, (200, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    xyz = (dirs * rng.uniform(0.05, 0.40, (200, 1))).astype(f32)      # well inside (1 - edge) r = 0.45 ...
    xyz[77] = (dirs[77] * 0.47).astype(f32)                            # ... except one point in the shell
    shell_row = C.shell(xyz, (0.0, 0.0, 0.0), r, edge)
    assert shell_row.sum() == 1 and shell_row[77]
    masks = np.zeros((3, 200), dtype=bool)
    masks[0, [3, 77, 150]] = True
    masks[1, [3, 150]] = True
    masks[2, 77] = True
    assert C.drop_shell_masks(masks, shell_row).tolist() == [False, True, False]
    ar = torch.arange(200, device="cuda")
    crop = Crop((0.0, 0.0, 0.0), r, 200, 200, 200, ar, ar, None)
    sb = crop_shell_bits(crop, torch.from_numpy(xyz).cuda(), edge)
    assert np.array_equal(sb.cpu().numpy().view(np.uint64), R.words(shell_row[None]))
    touches = ops.mask_intersections(torch.from_numpy(R.words(masks).view(np.int64)).cuda(), sb)[:, 0] > 0
    assert touches.tolist() == [True, False, True]


def test_multi_crop_proposals_equal_the_composition_by_hand(ops, scan, capsys):
    from point_sam_amd import scene as S
    from point_sam_amd.predictor import PointSAMPredictor
    from point_sam_amd.proposals import CropLayerConfig, ProposalConfig
    model, xyz, rgb, xyz_np, ref, clicks, outside = scan
    pred = PointSAMPredictor(model)
    pred.set_scene(xyz, rgb, max_points=SCENE_POINTS)
    logits, _, _ = pred.predict_masks(clicks[:, :1], torch.ones(1, 1, dtype=torch.int64, device="cuda"), None, True)
    thr = float(torch.quantile(logits[0, :, ::7].flatten(), 0.97))      # small masks: some of a crop's stay clear of its shell
    pc = ProposalConfig(num_prompts=16, prompt_chunk=16, mask_threshold=thr, pred_iou_thresh=0.0, stability_thresh=0.0, min_points=1, max_area_frac=1.0001)
    cl = CropLayerConfig(num_crops=2, radius=0.4, max_points=256, edge_frac=0.05, nms_thresh=0.7)
    got = pred.generate_masks(pc, crops=cl)
    assert len(got) == 1 and pred.crop is None
    got = got[0]
    # by hand, from public pieces
    base = pred.generate_masks(pc)[0]
    sc = pred.scene
    _, centers = ops.fps(xyz.index_select(0, sc.keep_idx)[None].contiguous(), 2)
    rows, score, area, origin = [base.bits.cpu().numpy().view(np.uint64)], [base.score.cpu().numpy()], [base.area.cpu().numpy()], [np.full(len(base), -1)]
    work = PointSAMPredictor(model)
    dropped = 0
    for ci, center in enumerate(centers[0].cpu().tolist()):
        assert (xyz_np == np.asarray(center, dtype=f32)).all(1).any()      # every centre is a real point
        crop, wxyz, wrgb = S.build_crop(xyz, rgb, center, cl.radius, max_points=cl.max_points)
        assert crop.num_members > cl.max_points >= crop.num_working and crop.voxel_size is not None      # the ladder was searched
        keep, inv, rxyz, rrgb, _ = C.crop_downsample(xyz_np, rgb.cpu().numpy(), center, cl.radius, crop.voxel_size)
        assert np.array_equal(crop.keep_idx.cpu().numpy(), keep) and np.array_equal(_bits(wxyz.cpu().numpy()), _bits(rxyz))
        k = round(4 * (1 - np.log2(crop.voxel_size)))
        assert S.ladder(k) == crop.voxel_size and ops.crop_count(xyz, center, cl.radius, S.ladder(k + 1))[0] > cl.max_points      # the next finer step would not fit
        work.set_pointcloud(torch.from_numpy(rxyz).cuda()[None].contiguous(), torch.from_numpy(rrgb).cuda()[None].contiguous())
        p = work.generate_masks(pc)[0]
        masks = p.masks().cpu().numpy()
        ok = C.drop_shell_masks(masks, C.shell(xyz_np[keep], center, cl.radius, cl.edge_frac))
        dropped += int((~ok).sum())
        b, a = C.expand_bits(R.words(masks[ok]), inv, len(keep)) if ok.any() else (np.zeros((0, (M_SCAN + 63) // 64), dtype=np.uint64), np.zeros(0, dtype=np.int32))
        rows.append(b); score.append(p.score.cpu().numpy()[ok]); area.append(a); origin.append(np.full(int(ok.sum()), ci))
    rows, score, area, origin = np.concatenate(rows), np.concatenate(score), np.concatenate(area), np.concatenate(origin)
    K = len(score)
    order = torch.sort(torch.from_numpy(score).cuda(), descending=True, stable=True).indices.to(torch.int32)
    bits = torch.from_numpy(rows.view(np.int64)).cuda().contiguous()
    darea = torch.from_numpy(area.astype(np.int32)).cuda()
    keepm = ops.mask_nms(order, torch.ones(K, dtype=torch.uint8, device="cuda"), darea, ops.mask_intersections(bits), cl.nms_thresh)
    labels = ops.mask_paint(bits, order, keepm, M_SCAN)
    sel = order.long()[keepm[order.long()].bool()].cpu().numpy()
    with capsys.disabled():
        print(f"\nmulti-crop: base {len(base)}, per-crop kept {[int((origin == c).sum()) for c in range(2)]}, dropped at the shell {dropped}, "
              f"merged {len(sel)} with origins {np.bincount(origin[sel] + 1, minlength=3).tolist()}")
    assert got.n_points == M_SCAN and len(got) == len(sel) >= 1
    assert np.array_equal(got.bits.cpu().numpy().view(np.uint64), rows[sel])
    assert np.array_equal(_bits(got.score.cpu().numpy()), _bits(score[sel]))
    assert got.crop_index.dtype == torch.int64 and np.array_equal(got.crop_index.cpu().numpy(), origin[sel])
    assert np.array_equal(got.area.cpu().numpy(), area[sel])
    assert torch.equal(got.labels, labels) and got.labels.dtype == torch.int32
    # the scores come out best first, and a tie keeps the earlier layer first
    s = got.score.cpu().numpy()
    assert (s[:-1] >= s[1:]).all()
    pred.set_crop(CENTER, RADIUS, voxel_size=CROP_VOXEL)
    with pytest.raises(RuntimeError, match="clear_crop"):
        pred.generate_masks(pc, crops=cl)
    plain = PointSAMPredictor(model)
    plain.set_pointcloud(xyz[None, :2000].contiguous(), rgb[None, :2000].contiguous())
    with pytest.raises(RuntimeError, match="set_scene"):
        plain.generate_masks(pc, crops=cl)
    with pytest.raises(RuntimeError, match="set_scene"):
        plain.set_crop(CENTER, RADIUS)


# ------------------------------------------------------------------------------------------------ 6. the C entry points
def test_crop_entry_points_resolve_and_reject_bad_arguments(ops):
    from point_sam_amd import _lib
    lib = _lib.load()
    for name in ("psam_crop_downsample_workspace_bytes", "psam_crop_downsample", "psam_crop_expand_rows", "psam_crop_expand_bits"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.psam_crop_downsample_workspace_bytes(0) == 0 and lib.psam_crop_downsample_workspace_bytes((1 << 28) + 1) == 0
    assert lib.psam_crop_downsample(None, None, 1, None, 1.0, 1.0, 0.0, None, None, None, None, None, None, 0, None) == -1
    assert b"null" in lib.psam_last_error_string()
    assert lib.psam_crop_expand_rows(None, 1, None, 1, 1, 1, 0, None, 1, None) == -1
    assert lib.psam_crop_expand_bits(None, None, 1, 1, 1, None, None, None) == -1


# ------------------------------------------------------------------------------------------------ 7. second-level scan with several blocks per thread
@pytest.mark.parametrize("h", [0.025, None])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_crop_downsample_with_one_two_and_three_blocks_per_offsets_thread(ops, which, h):
    """M = T^2, T^2 + 1 and 2 T^2 + T + 1 points for T = SCAN_THREADS read from voxel_table.h (the one constant behind both keys of scan_constants):
    crop_offsets_kernel -- the shared scan_block_offsets and the members' sum over the same spans -- gives each thread 1, 2 and 3 block counts
    (the last with a ragged final span and threads with none).  Uniform points of the cube; two stretches of 4 T consecutive points
    (the middle and the end) are copies of point 0, a member, so whole blocks count zero representatives with a voxel size (and T members).  The
    ball holds between a quarter and three quarters of the points (a condition on the inputs)."""
    import kernel_sizes as KS
    T = KS.scan_constants()["CROP_SCAN_THREADS"]
    M = KS.scan_sizes(T)[which]
    assert -(-(-(-M // T)) // T) == which + 1
    rng = np.random.default_rng(30 + which)
    xyz = rng.uniform(-1, 1, (M, 3)).astype(f32)
    xyz[0] = (0.3, -0.2, 0.1)
    xyz[M // 2:M // 2 + 4 * T] = xyz[0]
    xyz[M - 4 * T:] = xyz[0]
    rgb = rng.uniform(-1, 1, (M, 3)).astype(f32)
    center, radius = (0.05, -0.1, 0.02), 1.0
    want_keep, want_inv, want_xyz, want_rgb, want_members = C.crop_downsample(xyz, rgb, center, radius, h)
    print(f"M={M} h={h}: {which + 1} blocks per thread, {want_members} members, reference keeps {len(want_keep)}")
    assert M / 4 <= want_members <= 3 * M / 4 and want_inv[0] == 0
    if h is not None:
        own = np.zeros(M, dtype=bool)
        own[want_keep] = True
        per_block = np.add.reduceat(own, np.arange(0, M, T))
        assert (per_block[(M // 2) // T + 1:(M // 2) // T + 4] == 0).all() and (per_block[-3:] == 0).all() and len(want_keep) < want_members
    dx, dr = torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda()
    assert ops.crop_count(dx, center, radius, h) == (len(want_keep), want_members)
    keep_idx, inv, wxyz, wrgb, members = ops.crop_downsample(dx, dr, center, radius, h)
    assert members == want_members and keep_idx.numel() == len(want_keep)
    assert np.array_equal(keep_idx.cpu().numpy(), want_keep)
    assert np.array_equal(inv.cpu().numpy(), want_inv)
    assert np.array_equal(_bits(wxyz.cpu().numpy()), _bits(want_xyz))
    assert np.array_equal(_bits(wrgb.cpu().numpy()), _bits(want_rgb))
