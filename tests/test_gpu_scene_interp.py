"""Interpolated scene masks on the GPU (csrc/scene_interp.hip, scene.build_interp_plan, the predictor's smooth edges) against the plain numpy reference
in tests/interp_reference.py.  Every operation of the definition is a single rounded fp32 operation, so every comparison is equality of the bits:
idx3 as int32, w3 and the rows through a 32-bit integer view.

One exception, with its reason: where a BLEND (two or three sources) meets a NaN or inf - inf, the result is a NaN whose sign and payload IEEE 754 leaves
to the implementation (numpy on the host and the GPU differ); `_same_words` maps the NaNs of blended points -- and only those -- to one pattern before
it compares.  Copied words (single source, the representatives among them) and fills are compared as they are, NaN payloads included."""
import numpy as np
import pytest
import torch

import crop_reference as C
import interp_reference as I
import scene_reference as R
from oracle import pointsam_oracle as O
from point_sam_amd.config import get_config
from point_sam_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _words(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _same_words(got, want, idx3, Nw):
    """got, want [R, M] float32: equal bit for bit; NaNs that a blend computed are compared as NaNs (module docstring)."""
    got, want = np.ascontiguousarray(got, dtype=f32).copy(), np.ascontiguousarray(want, dtype=f32).copy()
    b = I.blended(idx3, Nw)[None] & np.ones(got.shape, dtype=bool)
    for a in (got, want):
        a.view(np.uint32)[b & np.isnan(a)] = 0x7FC00000
    return np.array_equal(got.view(np.int32), want.view(np.int32))


def _check_scene_plan(ops, xyz, h):
    """Downsample, neighbours and plan on the device against the references.  -> (reference (keep_idx, inv, wxyz, nbr, idx3, w3), device (idx3, w3))."""
    xyz = np.ascontiguousarray(xyz, dtype=f32)
    keep_idx, inv = R.downsample(xyz, h)
    wxyz = xyz[keep_idx]
    nbr = I.neighbors(wxyz, h)
    idx3, w3 = I.plan(xyz, inv, wxyz, nbr)
    dx = _dev(xyz)
    dk, di = ops.voxel_downsample(dx, h)
    assert np.array_equal(dk.cpu().numpy(), keep_idx) and np.array_equal(di.cpu().numpy(), inv)
    dn = ops.region_neighbors(dx, dk, h)
    assert np.array_equal(dn.cpu().numpy(), nbr)
    gi, gw = ops.scene_interp_plan(dx, di, dx.index_select(0, dk), dn)
    assert gi.dtype == torch.int32 and gw.dtype == torch.float32 and tuple(gi.shape) == tuple(gw.shape) == (len(xyz), 3)
    assert np.array_equal(gi.cpu().numpy(), idx3), np.nonzero((gi.cpu().numpy() != idx3).any(1))[0][:10]
    assert np.array_equal(_words(gw), w3.view(np.int32)), np.nonzero((_words(gw) != w3.view(np.int32)).any(1))[0][:10]
    return (keep_idx, inv, wxyz, nbr, idx3, w3), (gi, gw)


# ------------------------------------------------------------------------------------------------ 1. the plan
M_LATTICE = 1061


def _lattice():
    """5 x 5 x 5 cells of h = 0.25 from origin -1 (cells 0 .. 4: cell 0's neighbours fall outside the grid), 0 - 6 distinct positions per cell on the
    1 / 64 grid (sixteen steps per cell and axis, step 0 on the cell's lower face), some cells empty.  125 cells x 6 positions are fewer than the
    1061 points the case has, so the remainder repeats earlier points: exact duplicates, a tie in every comparison they enter."""
    rng = np.random.default_rng(12)
    pts = []
    for cell in range(125):
        c = np.array([cell % 5, cell // 5 % 5, cell // 25])
        for _ in range(int(rng.integers(0, 7)) if cell % 7 else 0):
            pts.append(-1 + (c * 16 + rng.integers(0, 16, 3)) / 64)
    pts = np.array(pts, dtype=f32)
    assert 250 < len(pts) < 750
    extra = pts[rng.integers(0, len(pts), M_LATTICE - len(pts))]
    xyz = np.concatenate([pts, extra])[rng.permutation(M_LATTICE)]
    return np.ascontiguousarray(xyz, dtype=f32)


@pytest.fixture(scope="module")
def lattice(ops):
    xyz = _lattice()
    ref, dev = _check_scene_plan(ops, xyz, 0.25)
    return xyz, ref, dev


def test_plan_lattice_with_ties_faces_and_empty_cells(ops, lattice):
    xyz, (keep_idx, inv, wxyz, nbr, idx3, w3), _ = lattice
    c, _ = R.cells(xyz, 0.25)
    assert c.min() == 0 and c.max() == 4 and len(keep_idx) < 125 and (nbr[inv] == -1).any()
    on_face = (np.round((xyz + 1) * 64) % 16 == 0).any(1)
    assert on_face.sum() > 100
    d = ((xyz[:, None, :].astype(np.float64) - wxyz[None].astype(np.float64)) ** 2).sum(-1)      # exact: the coordinates are multiples of 1 / 64
    cand = np.concatenate([inv[:, None], nbr[inv]], 1)
    tied = 0
    for i in range(len(xyz)):
        q = d[i, cand[i][cand[i] >= 0]]
        tied += len(np.unique(q)) < len(q)
    assert tied > 100, tied                                # distance ties among a point's candidates are frequent
    assert (idx3[:, 0] == inv).mean() < 0.9                # and the voxel's representative is often not the nearest


def test_plan_isolated_voxels_have_one_and_two_candidates(ops):
    rng = np.random.default_rng(13)
    cells = {"a": (0, 0, 0), "b": (7, 0, 0), "c": (0, 7, 7), "p0": (4, 4, 4), "p1": (5, 4, 4)}
    xyz, tag = [], []
    for name, cell in cells.items():
        n = 40
        xyz.append(-1 + (np.array(cell) + rng.uniform(0.05, 0.95, (n, 3))) * 0.25)
        tag += [name] * n
    order = rng.permutation(len(tag))
    xyz, tag = np.concatenate(xyz).astype(f32)[order], np.array(tag)[order]
    (keep_idx, inv, _, nbr, idx3, w3), _ = _check_scene_plan(ops, xyz, 0.25)
    assert len(keep_idx) == 5 and (nbr >= 0).sum() == 2
    single = np.isin(tag, ["a", "b", "c"])
    assert (idx3[single, 1:] == -1).all() and (idx3[single, 0] == inv[single]).all() and (w3[single] == np.array([1, 0, 0], dtype=f32)).all()
    pair = ~single
    pair[keep_idx] = False                                 # the two representatives are exact hits
    assert (idx3[pair, 1] >= 0).all() and (idx3[pair, 2] == -1).all() and (w3[pair, 2] == 0).all() and (w3[pair, :2] > 0).all()


def test_plan_exact_duplicates_and_negative_zero(ops):
    rng = np.random.default_rng(14)
    xyz = rng.uniform(-1, 1, (2000, 3)).astype(f32)
    xyz[:40, 0] = 0.0                                      # points on the plane x = 0, half of them written as -0.0
    xyz[:40:2, 0] = -0.0
    first, _ = R.downsample(xyz, 0.2)
    srcs = np.concatenate([first[first < 40][:20], first[(first >= 40) & (first < 1500)][-40:]])      # representatives: the lowest index of their voxels
    assert len(srcs) == 60
    dup = np.arange(1900, 1960)
    flip = xyz[srcs].copy()                                # exact duplicates of representatives, behind them: never representatives themselves
    assert (flip == 0).sum() == 20
    flip[flip == 0] *= -1                                  # twenty differ from their representative in the sign of a zero: still q = 0
    xyz[dup] = flip
    (keep_idx, inv, _, _, idx3, w3), _ = _check_scene_plan(ops, xyz, 0.2)
    assert np.isin(srcs, keep_idx).all() and not np.isin(dup, keep_idx).any() and np.signbit(xyz[:40, 0]).sum() == 20
    assert (np.signbit(xyz[dup[:20], 0]) != np.signbit(xyz[srcs[:20], 0])).all()
    assert (idx3[dup, 0] == inv[srcs]).all() and (idx3[dup, 1:] == -1).all() and (w3[dup] == np.array([1, 0, 0], dtype=f32)).all()
    assert (idx3[keep_idx, 1] == -1).all() and (idx3[:, 1] >= 0).sum() > 1000


@pytest.mark.parametrize("M", [1, 63, 64, 65, 1025, 3000])
def test_plan_sizes_around_wave_and_block(ops, M):
    xyz = np.random.default_rng(M).uniform(-1, 1, (M, 3)).astype(f32)
    _check_scene_plan(ops, xyz, 0.25)


@pytest.fixture(scope="module")
def cloud20k(ops):
    xyz = np.random.default_rng(15).uniform(-1, 1, (20000, 3)).astype(f32)
    ref, dev = _check_scene_plan(ops, xyz, 2.0 ** -3)
    return xyz, ref, dev


def test_plan_random_cloud(ops, cloud20k):
    xyz, (keep_idx, inv, wxyz, nbr, idx3, w3), _ = cloud20k
    assert 3000 < len(keep_idx) <= 4096 and (idx3[:, 2] >= 0).mean() > 0.75
    d = ((xyz[:2000, None, :].astype(np.float64) - wxyz[None].astype(np.float64)) ** 2).sum(-1)
    assert (idx3[:2000, 0] == d.argmin(1)).mean() > 0.99   # the 27 cells hold the true nearest working point


CROP_CENTER, CROP_RADIUS, CROP_VOXEL = (0.02, -0.03, 0.01), 0.98, 2.0 ** -3


@pytest.fixture(scope="module")
def crop5k(ops):
    """A ball holding about half of a 5000-point cloud, voxel size 2^-3 in crop units, one non-finite point (off the ball by definition)."""
    rng = np.random.default_rng(16)
    xyz = rng.uniform(-1, 1, (5000, 3)).astype(f32)
    xyz[777] = (np.nan, 0.1, np.inf)
    rgb = rng.uniform(0, 1, (5000, 3)).astype(f32)
    keep_idx, inv, wxyz, _, members = C.crop_downsample(xyz, rgb, CROP_CENTER, CROP_RADIUS, CROP_VOXEL)
    assert 2000 < members < 3000 and inv[777] == -1
    nbr = I.neighbors(wxyz, CROP_VOXEL)
    idx3, w3 = I.plan(I.crop_coordinate(xyz, CROP_CENTER, CROP_RADIUS), inv, wxyz, nbr)
    dx = _dev(xyz)
    dk, di, dw, _, dm = ops.crop_downsample(dx, _dev(rgb), CROP_CENTER, CROP_RADIUS, CROP_VOXEL)
    assert dm == members and np.array_equal(dk.cpu().numpy(), keep_idx) and np.array_equal(di.cpu().numpy(), inv) and np.array_equal(_words(dw), wxyz.view(np.int32))
    dn = ops.region_neighbors(dw, torch.arange(len(keep_idx), device="cuda"), CROP_VOXEL)
    assert np.array_equal(dn.cpu().numpy(), nbr)
    gi, gw = ops.scene_interp_plan(dx, di, dw, dn, center=CROP_CENTER, radius=CROP_RADIUS)
    return xyz, (keep_idx, inv, wxyz, nbr, idx3, w3), (gi, gw)


def test_plan_crop(ops, crop5k):
    _, (keep_idx, inv, _, _, idx3, w3), (gi, gw) = crop5k
    assert np.array_equal(gi.cpu().numpy(), idx3) and np.array_equal(_words(gw), w3.view(np.int32))
    off = inv < 0
    assert (idx3[off] == -1).all() and (w3[off] == 0).all() and (idx3[~off, 0] >= 0).all()
    assert (idx3[keep_idx, 0] == np.arange(len(keep_idx))).all() and (idx3[keep_idx, 1] == -1).all()


# ------------------------------------------------------------------------------------------------ 2. rows
def _special_source(rng, R_rows, Nw):
    src = rng.normal(0, 1, (R_rows, Nw)).astype(f32)
    special = np.array([0x7FC12345, 0xFFA00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001], dtype=np.uint32).view(f32)      # NaN payloads, +-inf, -0, a denormal
    for r in range(R_rows):
        src[r, 6 * r:6 * r + 6] = special                  # working points 0 .. 6 R: representatives and blend sources of their neighbourhoods
    return src


@pytest.mark.parametrize("R_rows", [1, 3, 4, 7])
def test_rows_strided_with_fill_specials_and_a_corrupt_index(ops, crop5k, R_rows):
    """Unroll tails (4 rows at a time), src_ld > Nw, dst_ld > M, -inf off the ball, special values at representatives, and an idx3 entry of value Nw
    that must be ignored: the source's column Nw (inside the wider buffer) holds a value that would show."""
    _, (keep_idx, inv, _, _, idx3, w3), (gi, gw) = crop5k
    Nw, M = len(keep_idx), len(inv)
    rng = np.random.default_rng(R_rows)
    src = _special_source(rng, R_rows, Nw)
    bad = idx3.copy()
    three = np.nonzero(idx3[:, 2] >= 0)[0]
    bad[three[0], 2], bad[three[1], 1], bad[three[2], 0] = Nw, Nw, Nw      # third dropped; second dropped: a copy; first dropped: off
    want = I.apply_rows(src, bad, w3, -np.inf)
    assert np.isneginf(want[:, three[2]]).all() and np.array_equal(want[:, three[1]].view(np.int32), src[:, bad[three[1], 0]].view(np.int32))
    wide = torch.full((R_rows + 2, Nw + 11), 7.5e30, device="cuda")
    wide[1:1 + R_rows, 3:3 + Nw] = _dev(src)
    view = wide[1:1 + R_rows, 3:3 + Nw]
    buf = torch.full((R_rows + 2, M + 5), -3.0, device="cuda")
    out = buf[1:1 + R_rows, 2:2 + M]
    ret = ops.scene_interp_rows(view, _dev(bad), gw, float("-inf"), out=out)
    assert ret is out
    full = buf.cpu().numpy()
    assert _same_words(full[1:1 + R_rows, 2:2 + M], want, bad, Nw)
    assert np.array_equal(np.ascontiguousarray(full[1:1 + R_rows, 2:2 + M][:, keep_idx]).view(np.int32), src.view(np.int32))      # the representatives, bit for bit
    assert np.isneginf(full[1:1 + R_rows, 2:2 + M][:, inv < 0]).all()
    full[1:1 + R_rows, 2:2 + M] = -3.0
    assert (full == -3.0).all(), "words outside the destination range were written"
    # the allocating form, leading dimensions kept, default fill 0
    got = ops.scene_interp_rows(_dev(src)[None], gi, gw)
    assert tuple(got.shape) == (1, R_rows, M) and _same_words(got[0].cpu().numpy(), I.apply_rows(src, idx3, w3, 0.0), idx3, Nw)


def test_rows_finite_sources_are_exactly_the_reference(ops, cloud20k):
    _, (keep_idx, _, _, _, idx3, w3), (gi, gw) = cloud20k
    src = np.random.default_rng(17).normal(0, 3, (3, len(keep_idx))).astype(f32)
    got = ops.scene_interp_rows(_dev(src), gi, gw)
    assert np.array_equal(_words(got), I.apply_rows(src, idx3, w3).view(np.int32))
    assert np.array_equal(_words(got[:, _dev(keep_idx)]), src.view(np.int32))


# ------------------------------------------------------------------------------------------------ 3. bits
@pytest.mark.parametrize("thr", [0.0, 0.37])
def test_bits_equal_mask_pack_of_the_rows(ops, lattice, thr):
    xyz, (keep_idx, _, _, _, idx3, w3), (gi, gw) = lattice
    Nw, M = len(keep_idx), M_LATTICE
    src = _special_source(np.random.default_rng(18), 5, Nw)
    dsrc = _dev(src)
    rows = ops.scene_interp_rows(dsrc, gi, gw)
    want_bits, want_area, _, _ = ops.mask_pack(rows.contiguous(), thr, 0.0)
    bits, area = ops.scene_interp_bits(dsrc, gi, gw, thr)
    assert bits.dtype == torch.int64 and tuple(bits.shape) == (5, (M + 63) // 64) and torch.equal(bits, want_bits)
    assert area.dtype == torch.int32 and torch.equal(area, want_area)
    got = bits.cpu().numpy().view(np.uint64)
    ref_bits, ref_area = I.apply_bits(src, idx3, w3, thr)
    assert np.array_equal(got, ref_bits) and np.array_equal(area.cpu().numpy(), ref_area)
    assert np.array_equal(area.cpu().numpy(), R.unwords(got, M).sum(1))                  # the areas are the popcounts
    assert M % 64 and (got[:, -1] >> np.uint64(M % 64)).max() == 0, "bits past M must be zero"
    nan_cols = np.isnan(rows.cpu().numpy())
    assert nan_cols.any() and not R.unwords(got, M)[nan_cols].any()                      # a NaN value is no member
    bits2, none = ops.scene_interp_bits(dsrc, gi, gw, thr, area=False)
    assert none is None and torch.equal(bits2, bits)


def test_bits_of_a_crop_are_zero_off_the_ball(ops, crop5k):
    _, (keep_idx, inv, _, _, idx3, w3), (gi, gw) = crop5k
    src = np.random.default_rng(19).normal(0, 1, (3, len(keep_idx))).astype(f32)
    rows = ops.scene_interp_rows(_dev(src), gi, gw, float("-inf"))
    bits, area = ops.scene_interp_bits(_dev(src), gi, gw, -1e30)      # every finite value passes: the ball's points, and nothing else
    want_bits, want_area, _, _ = ops.mask_pack(rows.contiguous(), -1e30, 0.0)
    assert torch.equal(bits, want_bits) and torch.equal(area, want_area) and area.tolist() == [int((inv >= 0).sum())] * 3
    assert np.array_equal(R.unwords(bits.cpu().numpy().view(np.uint64), len(inv)), np.tile(inv >= 0, (3, 1)))


# ------------------------------------------------------------------------------------------------ 4. determinism
def test_two_runs_and_a_side_stream_give_identical_bits(ops, cloud20k):
    xyz, (keep_idx, inv, wxyz, nbr, _, _), (gi, gw) = cloud20k
    dx, di, dw, dn = _dev(xyz), _dev(inv), _dev(wxyz), _dev(nbr)
    src = _dev(np.random.default_rng(20).normal(0, 1, (3, len(keep_idx))).astype(f32))
    rows, (bits, area) = ops.scene_interp_rows(src, gi, gw), ops.scene_interp_bits(src, gi, gw, 0.1)
    i2, w2 = ops.scene_interp_plan(dx, di, dw, dn)
    assert torch.equal(i2, gi) and torch.equal(w2.view(torch.int32), gw.view(torch.int32))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        i3, w3s = ops.scene_interp_plan(dx, di, dw, dn)
        rows3 = ops.scene_interp_rows(src, i3, w3s)
        bits3, area3 = ops.scene_interp_bits(src, i3, w3s, 0.1)
    side.synchronize()
    assert torch.equal(i3, gi) and torch.equal(w3s.view(torch.int32), gw.view(torch.int32))
    assert torch.equal(rows3.view(torch.int32), rows.view(torch.int32)) and torch.equal(bits3, bits) and torch.equal(area3, area)


# ------------------------------------------------------------------------------------------------ 5. the predictor
M_SCAN = 2000
VOXEL = 0.15            # 649 occupied voxels on the seeded scan below (tests/test_gpu_scene.py's scan)


@pytest.fixture(scope="module")
def scan(ops):
    from point_sam_amd.model import PointCloudSAM
    cfg = get_config("tiny")
    model = PointCloudSAM(cfg, random_state_dict(cfg, 3), "cuda", precision="f16x3")
    xyz, rgb, _, _ = O.synthetic_batch(1, M_SCAN, seed=8)
    xyz_np = np.ascontiguousarray(xyz[0].numpy(), dtype=f32)
    keep_idx, inv = R.downsample(xyz_np, VOXEL)
    wxyz = xyz_np[keep_idx]
    idx3, w3 = I.plan(xyz_np, inv, wxyz, I.neighbors(wxyz, VOXEL))
    clicks = xyz[0, [5, 1200]].cuda()[None]               # [1, 2, 3]: two points of the scan
    return model, xyz[0].cuda().contiguous(), rgb[0].cuda().contiguous(), keep_idx, inv, idx3, w3, clicks


def _one():
    return torch.ones(1, 1, dtype=torch.int64, device="cuda")


def test_predictor_smooth_scene_is_the_reference_blend_of_the_working_logits(ops, scan):
    from point_sam_amd.predictor import PointSAMPredictor
    model, xyz, rgb, keep_idx, inv, idx3, w3, clicks = scan
    dk, di = _dev(keep_idx), _dev(inv)
    Nw = len(keep_idx)
    work = PointSAMPredictor(model)
    work.set_pointcloud(xyz[dk][None].contiguous(), rgb[dk][None].contiguous())
    w1, ws1, _ = work.predict_masks(clicks[:, :1], _one(), None, True)
    pred = PointSAMPredictor(model)
    pred.set_scene(xyz, rgb, voxel_size=VOXEL, smooth=True)
    state = pred._state
    s1, ss1, _ = pred.predict_masks(clicks[:, :1], _one(), None, True)
    assert tuple(s1.shape) == (1, w1.shape[1], M_SCAN) and torch.equal(ss1, ws1)
    assert np.array_equal(_words(s1[0]), I.apply_rows(w1[0].cpu().numpy(), idx3, w3).view(np.int32))
    assert torch.equal(s1[..., dk], w1)                    # reduce_prompt_mask's round trip stays exact
    # smooth=False: the exact voxel transfer, as before; toggling encodes nothing
    pred.set_scene(xyz, rgb, voxel_size=VOXEL)
    assert pred._state is state
    h1, _, _ = pred.predict_masks(clicks[:, :1], _one(), None, True)
    assert torch.equal(h1, ops.scene_expand_rows(w1, di)) and torch.equal(h1, w1[:, :, di]) and not torch.equal(h1, s1)
    pred.set_scene(xyz, rgb, voxel_size=VOXEL, smooth=True)
    assert pred._state is state
    # click 2: the scan-width smooth logits as the mask prompt give what the working-width logits give
    best = torch.argmax(ss1[0])
    two = torch.cat([_one(), 1 - _one()], 1)
    a, sa, _ = pred.predict_masks(clicks, two, s1[0][best][None], False)
    b, sb, _ = pred.predict_masks(clicks, two, w1[0][best][None], False)
    w2, ws2, _ = work.predict_masks(clicks, two, w1[0][best][None], False)
    assert torch.equal(a, b) and torch.equal(sa, sb) and torch.equal(sa, ws2)
    assert np.array_equal(_words(a[0]), I.apply_rows(w2[0].cpu().numpy(), idx3, w3).view(np.int32))
    # the bits: mask_pack of the logits, smooth and not
    for smooth in (True, False):
        pred.set_scene(xyz, rgb, voxel_size=VOXEL, smooth=smooth)
        logits, scores, _ = pred.predict_masks(clicks[:, :1], _one(), None, True)
        thr = float(logits[0, 0].median())                 # about half of the first mask
        want_bits, want_area, _, _ = ops.mask_pack(logits.contiguous(), thr, 0.0)
        bits, area, sc2 = pred.predict_mask_bits(clicks[:, :1], _one(), None, True, threshold=thr)
        assert torch.equal(bits, want_bits) and torch.equal(area, want_area) and torch.equal(sc2, scores) and 0 < int(area[0]) < M_SCAN
    assert pred._state is state
    # after set_pointcloud: mask_pack alone
    bits, area, _ = work.predict_mask_bits(clicks[:, :1], _one(), None, True, threshold=0.0)
    want_bits, want_area, _, _ = ops.mask_pack(w1.contiguous(), 0.0, 0.0)
    assert torch.equal(bits, want_bits) and torch.equal(area, want_area) and tuple(bits.shape) == (w1.shape[1], (Nw + 63) // 64)


def test_predictor_smooth_crop(ops, scan):
    from point_sam_amd.predictor import PointSAMPredictor
    model, xyz, rgb, _, _, _, _, clicks = scan
    center, radius, h = tuple(float(v) for v in clicks[0, 0].cpu()), 0.8, 0.2
    xyz_np, rgb_np = xyz.cpu().numpy(), rgb.cpu().numpy()
    ck, ci, cw, cr, members = C.crop_downsample(xyz_np, rgb_np, center, radius, h)
    assert 100 < len(ck) < members < M_SCAN
    idx3, w3 = I.plan(I.crop_coordinate(xyz_np, center, radius), ci, cw, I.neighbors(cw, h))
    work = PointSAMPredictor(model)
    work.set_pointcloud(_dev(cw)[None], _dev(cr)[None])
    click_u = _dev(C.crop_prompts(clicks[:, :1].cpu().numpy(), center, radius))
    w1, ws1, _ = work.predict_masks(click_u, _one(), None, True)
    pred = PointSAMPredictor(model)
    pred.set_scene(xyz, rgb, voxel_size=VOXEL, smooth=True)
    pred.set_crop(center, radius, voxel_size=h)            # smooth=None: the scene's setting
    crop_state = pred._crop_state
    assert np.array_equal(pred.crop.keep_idx.cpu().numpy(), ck) and np.array_equal(_words(crop_state.coords[0]), cw.view(np.int32))
    s1, ss1, _ = pred.predict_masks(clicks[:, :1], _one(), None, True)
    assert torch.equal(ss1, ws1)
    assert np.array_equal(_words(s1[0]), I.apply_rows(w1[0].cpu().numpy(), idx3, w3, -np.inf).view(np.int32))
    assert torch.isneginf(s1[0][:, _dev(ci < 0)]).all() and torch.equal(s1[..., _dev(ck)], w1)
    best = torch.argmax(ss1[0])
    a, _, _ = pred.predict_masks(clicks[:, :1], _one(), s1[0][best][None], False)
    b, _, _ = pred.predict_masks(clicks[:, :1], _one(), w1[0][best][None], False)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    bits, area, _ = pred.predict_mask_bits(clicks[:, :1], _one(), None, True)
    want_bits, want_area, _, _ = ops.mask_pack(s1.contiguous(), 0.0, 0.0)
    assert torch.equal(bits, want_bits) and torch.equal(area, want_area)
    # not smooth: the voxel transfer of the same crop, nothing encoded again; and back, after clear_crop
    pred.set_crop(center, radius, voxel_size=h, smooth=False)
    assert pred._crop_state is crop_state
    h1, _, _ = pred.predict_masks(clicks[:, :1], _one(), None, True)
    assert torch.equal(h1.view(torch.int32), ops.crop_expand_rows(w1, _dev(ci), float("-inf")).view(torch.int32))
    bits, area, _ = pred.predict_mask_bits(clicks[:, :1], _one(), None, True)
    want_bits, want_area, _, _ = ops.mask_pack(h1.contiguous(), 0.0, 0.0)
    assert torch.equal(bits, want_bits) and torch.equal(area, want_area)
    pred.clear_crop()
    pred.set_crop(center, radius, voxel_size=h, smooth=True)
    assert pred._crop_state is crop_state
    again, _, _ = pred.predict_masks(clicks[:, :1], _one(), None, True)
    assert torch.equal(again.view(torch.int32), s1.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 6. quality
def test_smooth_bits_follow_an_analytic_sphere_better_than_the_voxel_transfer(ops):
    """A uniform scan of 200 000 points at h = 1 / 8; the working logits are the signed distance to a sphere, evaluated at the working points.  The
    numpy reference counts 671 (voxel transfer) against 317 (blend) wrong signs in a 30 000-point sample of this set-up."""
    rng = np.random.default_rng(21)
    M, h = 200000, 0.125
    xyz = rng.uniform(-1, 1, (M, 3)).astype(f32)
    field = 0.7 - np.linalg.norm(xyz.astype(np.float64) - np.array([0.05, -0.02, 0.03]), axis=1)
    dx = _dev(xyz)
    dk, di = ops.voxel_downsample(dx, h)
    Nw = dk.numel()
    logits = _dev(field.astype(f32))[dk][None].contiguous()
    idx3, w3 = ops.scene_interp_plan(dx, di, dx.index_select(0, dk), ops.region_neighbors(dx, dk, h))
    smooth, _ = ops.scene_interp_bits(logits, idx3, w3, 0.0)
    hard, _ = ops.scene_expand_bits(ops.mask_pack(logits, 0.0, 0.0)[0], di, Nw)
    truth = field > 0
    wrong_smooth = int((R.unwords(smooth.cpu().numpy().view(np.uint64), M)[0] != truth).sum())
    wrong_hard = int((R.unwords(hard.cpu().numpy().view(np.uint64), M)[0] != truth).sum())
    print(f"wrong signs of {M}: voxel transfer {wrong_hard}, blend {wrong_smooth}")
    assert wrong_smooth < wrong_hard, (wrong_smooth, wrong_hard)
