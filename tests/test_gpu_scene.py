"""Full-resolution scenes on the GPU (csrc/scene.hip, point_sam_amd/scene.py): every output is an integer, a bit or a bit-for-bit copy, so every comparison
is equality -- against the plain numpy reference in tests/scene_reference.py and against the existing set_pointcloud / predict_masks / generate_masks."""
import http.client
import json
import threading

import numpy as np
import pytest
import torch

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


def _check_downsample(ops, xyz, h, origin=(-1.0, -1.0, -1.0)):
    want_keep, want_inv = R.downsample(xyz, h, origin)
    dev = torch.from_numpy(np.ascontiguousarray(xyz, dtype=f32)).cuda()
    keep_idx, inv = ops.voxel_downsample(dev, h, origin)
    assert keep_idx.dtype == torch.int64 and inv.dtype == torch.int64 and keep_idx.is_contiguous()
    assert keep_idx.numel() == len(want_keep), (keep_idx.numel(), len(want_keep))
    assert np.array_equal(keep_idx.cpu().numpy(), want_keep)
    assert np.array_equal(inv.cpu().numpy(), want_inv)
    assert ops.voxel_count(dev, h, origin) == len(want_keep)          # count-only mode agrees with the full mode
    return dev, keep_idx, inv


# ------------------------------------------------------------------------------------------------ 1. downsample
@pytest.mark.parametrize("M", [1, 63, 64, 65, 1025, 4097])
def test_downsample_sizes_around_wave_block_and_second_level(ops, M):
    """One point; one short of, exactly and one past a wave (a ballot); one past a scan block of 1024; five blocks (second-level offsets).  h = 0.2 is
    no power of two (the product with fl32(1 / h) rounds), and about a third to all of the points share a voxel with an earlier one."""
    rng = np.random.default_rng(M)
    xyz = rng.uniform(-1, 1, (M, 3)).astype(f32)
    _, keep_idx, _ = _check_downsample(ops, xyz, 0.2)
    assert M < 1025 or keep_idx.numel() < M


def test_downsample_one_point_4096_times(ops):
    xyz = np.tile(np.array([[0.3, -0.7, 0.1]], dtype=f32), (4096, 1))
    _, keep_idx, inv = _check_downsample(ops, xyz, 0.05)
    assert keep_idx.tolist() == [0] and int(inv.max()) == 0


def test_downsample_every_point_in_its_own_voxel(ops):
    rng = np.random.default_rng(3)
    cells = rng.permutation(20 ** 3)[:5000]
    ijk = np.stack([cells % 20, cells // 20 % 20, cells // 400], 1)
    xyz = (-1 + (ijk + rng.uniform(0.1, 0.9, ijk.shape)) * 0.1).astype(f32)
    _, keep_idx, inv = _check_downsample(ops, xyz, 0.1)
    assert np.array_equal(keep_idx.cpu().numpy(), np.arange(5000)) and np.array_equal(inv.cpu().numpy(), np.arange(5000))


def test_downsample_lattice_pins_floor_and_edge_cell(ops):
    """Coordinates exactly origin + k h, h = 2^-3: every product is exact, so a point on a cell's lower face belongs to that cell; -1.0 is cell 0, 1.0 is
    cell 16, and -0.0 is cell 8 like 0.0.  Each lattice point appears twice (the second copy never a representative)."""
    h = 0.125
    g = (-1 + np.arange(17) * h).astype(f32)
    assert g[0] == -1.0 and g[16] == 1.0 and g[8] == 0.0
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(4)
    xyz = np.concatenate([lat[rng.permutation(len(lat))], lat[rng.permutation(len(lat))]]).astype(f32)
    zero = xyz == 0.0
    xyz[zero & (rng.random(xyz.shape) < 0.5)] = -0.0
    assert np.signbit(xyz[zero]).any() and not np.signbit(xyz[zero]).all()
    c, bad = R.cells(xyz, h)
    assert not bad.any() and c.min() == 0 and c.max() == 16 and np.array_equal(c, (xyz.astype(np.float64) + 1) * 8)
    _, keep_idx, inv = _check_downsample(ops, xyz, h)
    assert keep_idx.numel() == 17 ** 3 and np.array_equal(keep_idx.cpu().numpy(), np.arange(17 ** 3))
    # another origin and size: the same lattice seen from (-2, -1.5, -1) at h = 0.25
    _check_downsample(ops, xyz, 0.25, (-2.0, -1.5, -1.0))


def test_downsample_200k_uniform_points_and_a_second_stream(ops):
    """h = 0.037: 113 556 occupied voxels, half of them with more than one point -- a table of 2^19 slots holds them at load 0.22 with many probe
    collisions.  The same call on another stream gives identical tensors (slot positions depend on arrival order; no output may)."""
    rng = np.random.default_rng(7)
    xyz = rng.uniform(-1, 1, (200000, 3)).astype(f32)
    want_keep, want_inv = R.downsample(xyz, 0.037)
    shared = (np.bincount(want_inv) > 1).mean()
    assert 0.4 < shared < 0.6, shared
    dev, keep_idx, inv = _check_downsample(ops, xyz, 0.037)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        keep2, inv2 = ops.voxel_downsample(dev, 0.037)
    side.synchronize()
    assert torch.equal(keep2, keep_idx) and torch.equal(inv2, inv)


# ------------------------------------------------------------------------------------------------ 2. the flag
def _valid_cloud():
    return np.random.default_rng(11).uniform(-1, 1, (300, 3)).astype(f32)


@pytest.mark.parametrize("bad", ["nan", "inf", "cell_2^21"])
def test_flag_raises_value_error_and_is_cleared_by_the_next_call(ops, bad):
    xyz = _valid_cloud()
    h = 0.2
    if bad == "nan":
        xyz[17, 1] = np.nan
    elif bad == "inf":
        xyz[299, 2] = np.inf
    else:                                                 # (1 - (-1)) * 2^20 = 2^21: one past the last cell; 1 - 2^-20 is the last cell and passes
        h = 2.0 ** -20
        xyz[5, 0] = 1.0
        ok = xyz.copy(); ok[5, 0] = f32(1 - 2.0 ** -20)
        _check_downsample(ops, ok, h)
    dev = torch.from_numpy(xyz).cuda()
    with pytest.raises(ValueError):
        R.downsample(xyz, h)
    with pytest.raises(ValueError):
        ops.voxel_downsample(dev, h)
    with pytest.raises(ValueError):
        ops.voxel_count(dev, h)
    _check_downsample(ops, _valid_cloud(), 0.2)           # a following valid call succeeds: the flag was cleared


# ------------------------------------------------------------------------------------------------ 3. expand rows
@pytest.mark.parametrize("R_rows", [1, 3])
def test_expand_rows_bit_for_bit(ops, R_rows):
    rng = np.random.default_rng(R_rows)
    Nw, M = 517, 2000 + 37
    inv = rng.integers(0, Nw, M)
    inv[:3] = (0, Nw - 1, Nw - 1)
    src = rng.normal(0, 1, (R_rows, Nw)).astype(f32)
    src.reshape(-1)[:6 if R_rows > 1 else 5] = [np.nan, -0.0, np.inf, -np.inf, 0.0, 1e-45][:6 if R_rows > 1 else 5]
    inv[3:8] = np.arange(5)                               # the special values are certainly gathered
    dinv = torch.from_numpy(inv).cuda()
    want = R.expand_rows(src, inv)
    got = ops.scene_expand_rows(torch.from_numpy(src).cuda(), dinv)
    assert got.dtype == torch.float32 and tuple(got.shape) == (R_rows, M)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # int32 rows with -1; a 1-D source gives a 1-D result; a [2, R, Nw] source a [2, R, M] result
    lab = rng.integers(-1, 9, (R_rows, Nw)).astype(np.int32)
    lab[:, 0] = -1
    got = ops.scene_expand_rows(torch.from_numpy(lab).cuda(), dinv)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), R.expand_rows(lab, inv)) and (got[:, 3] == -1).all()
    one = ops.scene_expand_rows(torch.from_numpy(lab[0]).cuda(), dinv)
    assert tuple(one.shape) == (M,) and np.array_equal(one.cpu().numpy(), lab[0][inv])
    both = ops.scene_expand_rows(torch.from_numpy(np.stack([src, -src])).cuda(), dinv)
    assert tuple(both.shape) == (2, R_rows, M) and np.array_equal(both.cpu().numpy().view(np.uint32), np.stack([want, R.expand_rows(-src, inv)]).view(np.uint32))
    # source and destination with row strides larger than the row; the destination rows sit inside a larger buffer that is otherwise untouched
    wide = torch.full((R_rows + 2, Nw + 11), 7.5, device="cuda")
    wide[1:1 + R_rows, 3:3 + Nw] = torch.from_numpy(src).cuda()
    view = wide[1:1 + R_rows, 3:3 + Nw]
    assert R_rows == 1 or view.stride(0) == Nw + 11
    buf = torch.full((R_rows + 2, M + 5), -3.0, device="cuda")
    out = buf[1:1 + R_rows, 2:2 + M]
    ret = ops.scene_expand_rows(view, dinv, out=out)
    assert ret is out
    full = buf.cpu().numpy()
    assert np.array_equal(full[1:1 + R_rows, 2:2 + M].view(np.uint32), want.view(np.uint32))
    full[1:1 + R_rows, 2:2 + M] = -3.0
    assert (full == -3.0).all(), "words outside the destination range were written"


# ------------------------------------------------------------------------------------------------ 4. expand bits
@pytest.mark.parametrize("K,Nw,M", [(1, 1, 1), (5, 130, 1000), (64, 2048 + 37, 8192 + 5), (300, 4096, 70001)])
def test_expand_bits_equal_numpy(ops, K, Nw, M):
    rng = np.random.default_rng(K + Nw)
    masks = rng.random((K, Nw)) < rng.uniform(0.02, 0.9, (K, 1))
    masks[0] = True
    masks[-1] = K == 1
    inv = rng.integers(0, Nw, M)
    inv[0], inv[-1] = Nw - 1, Nw - 1
    ww = R.words(masks)
    want, want_area = R.expand_bits(ww, inv, Nw)
    dw, dinv = torch.from_numpy(ww.view(np.int64)).cuda(), torch.from_numpy(inv).cuda()
    bits, area = ops.scene_expand_bits(dw, dinv, Nw)
    got = bits.cpu().numpy().view(np.uint64)
    assert got.shape == (K, (M + 63) // 64) and np.array_equal(got, want)
    if M % 64:
        assert (got[:, -1] >> np.uint64(M % 64)).max() == 0, "bits past M must be zero"
    assert area.dtype == torch.int32 and np.array_equal(area.cpu().numpy(), want_area)
    assert int(area[0]) == M
    bits2, none = ops.scene_expand_bits(dw, dinv, Nw, area=False)      # area_f = NULL is accepted
    assert none is None and torch.equal(bits2, bits)


# ------------------------------------------------------------------------------------------------ 5. the predictor on a scene
M_SCAN = 2000
VOXEL = 0.15            # 649 occupied voxels on the seeded scan below (the numpy reference's count)


@pytest.fixture(scope="module")
def scan(ops):
    from point_sam_amd.model import PointCloudSAM
    cfg = get_config("tiny")
    model = PointCloudSAM(cfg, random_state_dict(cfg, 3), "cuda", precision="f16x3")
    xyz, rgb, _, _ = O.synthetic_batch(1, M_SCAN, seed=8)
    keep_idx, inv = R.downsample(xyz[0].numpy(), VOXEL)
    assert 400 <= len(keep_idx) <= 800
    clicks = xyz[0, [5, 1200]].cuda()[None]               # [1, 2, 3]: two points of the scan
    return model, xyz[0].cuda().contiguous(), rgb[0].cuda().contiguous(), keep_idx, inv, clicks


def _two_clicks(pred, clicks, pick=lambda full: full):
    """The demo's loop: click 1 multimask, click 2 with the best mask's logits as the dense prompt.  pick: what of the returned logits is handed back."""
    one = torch.ones(1, 1, dtype=torch.int64, device="cuda")
    m1, s1, l1 = pred.predict_masks(clicks[:, :1], one, None, True)
    best = torch.argmax(s1[0])
    m2, s2, l2 = pred.predict_masks(clicks, torch.cat([one, 1 - one], 1), pick(l1[0][best][None]), False)
    return (l1, s1), (l2, s2)


def test_scene_that_fits_is_its_own_working_cloud(ops, scan):
    from point_sam_amd.predictor import PointSAMPredictor
    model, xyz, rgb, _, _, clicks = scan
    plain = PointSAMPredictor(model)
    plain.set_pointcloud(xyz[None], rgb[None])
    want = _two_clicks(plain, clicks)
    assert plain.scene is None
    for max_points in (M_SCAN, M_SCAN + 1):
        pred = PointSAMPredictor(model)
        pred.set_scene(xyz, rgb, max_points=max_points)
        sc = pred.scene
        assert sc.num_working == M_SCAN and sc.identity
        assert torch.equal(sc.keep_idx, torch.arange(M_SCAN, device="cuda")) and torch.equal(sc.inv, sc.keep_idx)
        for (gl, gs), (wl, ws) in zip(_two_clicks(pred, clicks), want):
            assert torch.equal(gl, wl) and torch.equal(gs, ws)
    # back to a plain cloud: the scene is gone and nothing changed
    pred.set_pointcloud(xyz[None], rgb[None])
    assert pred.scene is None
    for (gl, gs), (wl, ws) in zip(_two_clicks(pred, clicks), want):
        assert torch.equal(gl, wl) and torch.equal(gs, ws)


def test_scene_logits_are_the_working_clouds_indexed_by_inv(ops, scan):
    from point_sam_amd.predictor import PointSAMPredictor
    model, xyz, rgb, keep_idx, inv, clicks = scan
    pred = PointSAMPredictor(model)
    pred.set_scene(xyz, rgb, voxel_size=VOXEL)
    sc = pred.scene
    assert sc.num_working == len(keep_idx) and not sc.identity and sc.num_points == M_SCAN
    assert np.array_equal(sc.keep_idx.cpu().numpy(), keep_idx) and np.array_equal(sc.inv.cpu().numpy(), inv)
    state = pred._state
    pred.set_scene(xyz, rgb, voxel_size=VOXEL)             # cached under the same kind of key as set_pointcloud
    assert pred._state is state
    dk, di = torch.from_numpy(keep_idx).cuda(), torch.from_numpy(inv).cuda()
    assert torch.equal(state.coords[0], xyz[dk])           # the working cloud consists of real points of the scan
    work = PointSAMPredictor(model)
    work.set_pointcloud(xyz[dk][None].contiguous(), rgb[dk][None].contiguous())
    want = _two_clicks(work, clicks)
    got = _two_clicks(pred, clicks)                        # click 2 hands the full-width logits back, as the demo does
    for (gl, gs), (wl, ws) in zip(got, want):
        assert tuple(gl.shape) == (1, wl.shape[1], M_SCAN)
        assert torch.equal(gl, wl[:, :, di]) and torch.equal(gs, ws)
    # a prompt mask of the working cloud's width is taken as it is
    narrow = _two_clicks(pred, clicks, pick=lambda full: full[:, dk])
    assert torch.equal(narrow[1][0], got[1][0])
    with pytest.raises(ValueError, match="width"):
        pred.predict_masks(clicks, torch.ones(1, 2, dtype=torch.int64, device="cuda"), torch.zeros(1, M_SCAN - 1, device="cuda"), False)


def test_scene_proposals_are_the_working_clouds_expanded(ops, scan):
    from point_sam_amd.predictor import PointSAMPredictor
    from point_sam_amd.proposals import ProposalConfig
    model, xyz, rgb, keep_idx, inv, clicks = scan
    dk = torch.from_numpy(keep_idx).cuda()
    work = PointSAMPredictor(model)
    work.set_pointcloud(xyz[dk][None].contiguous(), rgb[dk][None].contiguous())
    logits, _, _ = work.predict_masks(clicks[:, :1], torch.ones(1, 1, dtype=torch.int64, device="cuda"), None, True)
    pc = ProposalConfig(num_prompts=32, prompt_chunk=16, mask_threshold=float(logits.median()), pred_iou_thresh=float("-inf"), stability_thresh=0.0,
                        min_points=1, max_area_frac=1.0001)
    want = work.generate_masks(pc)[0]
    assert len(want) >= 1 and want.n_points == len(keep_idx)
    pred = PointSAMPredictor(model)
    pred.set_scene(xyz, rgb, voxel_size=VOXEL)
    got = pred.generate_masks(pc)
    assert len(got) == 1
    got = got[0]
    bits, area = R.expand_bits(want.bits.cpu().numpy().view(np.uint64), inv, len(keep_idx))
    assert got.n_points == M_SCAN and len(got) == len(want)
    assert np.array_equal(got.labels.cpu().numpy(), want.labels.cpu().numpy()[inv]) and got.labels.dtype == torch.int32
    assert np.array_equal(got.bits.cpu().numpy().view(np.uint64), bits)
    assert np.array_equal(got.area.cpu().numpy(), area) and got.area.dtype == torch.int32
    for name in ("score", "candidate", "prompt_index", "stability"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    assert np.array_equal(got.masks().cpu().numpy(), want.masks().cpu().numpy()[:, inv])


def test_segment_route_with_working_points_answers_per_loaded_point(ops, scan):
    from point_sam_amd.demo_server import DemoSession, serve
    from point_sam_amd.predictor import PointSAMPredictor
    model, xyz, rgb, _, _, _ = scan
    pred = PointSAMPredictor(model)
    sess = DemoSession(pred, working_points=700)
    srv = serve(sess, "127.0.0.1", 0)
    threading.Thread(target=srv.serve_forever, daemon=True).start()

    def req(path, body):
        c = http.client.HTTPConnection("127.0.0.1", srv.server_address[1], timeout=120)
        c.request("POST", path, json.dumps(body), {"Content-Type": "application/json"})
        r = c.getresponse()
        return r.status, json.loads(r.read())

    try:
        st, _ = req("/sampled_pointcloud", {"points": {str(i): float(v) for i, v in enumerate(xyz.flatten().tolist())},
                                            "colors": {str(i): float(v) for i, v in enumerate(rgb.flatten().tolist())}})
        assert st == 200
        for click in range(2):
            st, out = req("/segment", {"prompt_point": xyz[5 + click].tolist(), "prompt_label": 1})
            assert st == 200, out
            assert len(out["seg"]) == M_SCAN and all(isinstance(v, bool) for v in out["seg"])
        sc = pred.scene
        assert sc is not None and 0 < sc.num_working <= 700 and sc.num_points == M_SCAN
        # the working size is the ladder's answer: the next finer step would exceed 700
        from point_sam_amd.scene import ladder
        k = round(4 * (1 - np.log2(sc.voxel_size)))
        assert ladder(k) == sc.voxel_size and ops.voxel_count(sess.pc_xyz, ladder(k)) == sc.num_working and ops.voxel_count(sess.pc_xyz, ladder(k + 1)) > 700
        st, out = req("/segment_all", {"num_prompts": 16, "prompt_chunk": 16, "mask_threshold": 0.0, "pred_iou_thresh": -1e30, "stability_thresh": 0.0,
                                       "min_points": 1, "max_area_frac": 1.0001})
        assert st == 200 and len(out["labels"]) == M_SCAN, out
    finally:
        srv.shutdown()


# ------------------------------------------------------------------------------------------------ 6. second-level scan with several blocks per thread
def _scan_cloud(M, T, seed):
    """Uniform points of the cube; two stretches of 4 T consecutive points (the middle and the end) are copies of point 0, so whole blocks of the
    look-up kernel count zero representatives inside a thread's span of the offsets kernel."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-1, 1, (M, 3)).astype(f32)
    xyz[M // 2:M // 2 + 4 * T] = xyz[0]
    xyz[M - 4 * T:] = xyz[0]
    return xyz


@pytest.mark.parametrize("which", [0, 1, 2])
def test_downsample_with_one_two_and_three_blocks_per_offsets_thread(ops, which):
    """M = T^2, T^2 + 1 and 2 T^2 + T + 1 points for T = SCAN_THREADS read from voxel_table.h: scan_block_offsets (voxel_offsets_kernel) gives each
    thread 1, 2 and 3 block counts (the last with a ragged final span and threads with none): the serial span sum, the in-place rewrite of the span,
    the empty spans.
    h = 0.025: the reference keeps between M / 8 and M / 2 points (a condition on the inputs)."""
    import kernel_sizes as KS
    T = KS.scan_constants()["SCAN_THREADS"]
    M = KS.scan_sizes(T)[which]
    blocks = -(-M // T)
    assert -(-blocks // T) == which + 1
    xyz = _scan_cloud(M, T, 20 + which)
    want_keep, want_inv = R.downsample(xyz, 0.025)
    print(f"M={M}: {blocks} blocks, {which + 1} per thread, reference keeps {len(want_keep)}")
    assert M / 8 <= len(want_keep) <= M / 2
    own = np.zeros(M, dtype=bool)
    own[want_keep] = True
    per_block = np.add.reduceat(own, np.arange(0, M, T))
    assert (per_block[(M // 2) // T + 1:(M // 2) // T + 4] == 0).all() and (per_block[-3:] == 0).all() and per_block.max() > 0
    dev = torch.from_numpy(xyz).cuda()
    assert ops.voxel_count(dev, 0.025) == len(want_keep)                  # the count-only call
    keep_idx, inv = ops.voxel_downsample(dev, 0.025)
    assert keep_idx.numel() == len(want_keep)
    assert np.array_equal(keep_idx.cpu().numpy(), want_keep)
    assert np.array_equal(inv.cpu().numpy(), want_inv)
