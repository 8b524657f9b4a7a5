"""Scan map tracking on the GPU (csrc/track.hip, ops.track_step, ScanMap.track_step / track, predictor.map_align / map_nearest) against the plain numpy
reference tests/track_reference.py.  `nearest` and the two counts are always exact.  The other sums are exact on the lattice case and otherwise
within M * 2^-53 * sum |term| of the exactly rounded value, the bound tests/test_gpu_align.py uses.  Every step goes through the C entry with the
workspace and `sums` between guard words, and the map's block is compared bit for bit before and after: a step only reads it."""
import ctypes

import numpy as np
import pytest
import torch

import align_reference as AR
import scanmap_reference as SM
import track_reference as TR
from point_sam_amd.config import get_config
from point_sam_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu
f32 = np.float32
U = 2.0 ** -53
GUARD_WORDS = 512            # 4 KiB of float64
GUARD = -7.25                # the sentinel of `sums` and the guards: no sum of a case takes this value
CASES = TR.cases()


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd import ops
    return ops


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pack(take, garbage=True):
    """[n] bool -> [ceil(n / 64)] int64 words in mask_pack's layout; with garbage the bits past n are SET (the entry must ignore them)."""
    n = len(take)
    pad = np.ones(-(-n // 64) * 64, dtype=bool) if garbage else np.zeros(-(-n // 64) * 64, dtype=bool)
    pad[:n] = take
    return (pad.reshape(-1, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(1, dtype=np.uint64).view(np.int64)


def _device_map(case):
    """-> (ScanMap on the device, RefMap): the case's adds in order; the ids of every add agree."""
    from point_sam_amd.scanmap import ScanMap
    m, ref = ScanMap(case["h"], case["max_voxels"]), SM.RefMap(case["h"], case["max_voxels"])
    for pts in case["adds"]:
        got = m.add(_dev(pts), _dev(np.zeros_like(pts)))
        assert np.array_equal(got.ids.cpu().numpy(), ref.add(pts, np.zeros_like(pts))[0])
    assert m.num_voxels == ref.V
    return m, ref


_maps = {}


def _shared_map(case):
    """One device map per distinct list of adds: the cases of the step share it, and no step changes it."""
    key = (case["h"], case["max_voxels"]) + tuple(a.tobytes() for a in case["adds"])
    if key not in _maps:
        _maps[key] = _device_map(case)
    return _maps[key]


def _raw_step(m, qry, r2, reach, pose=None, take=None, V=None, skip=None, min_count=1, nearest=True, garbage=True):
    """psam_track_step itself: `sums` and the workspace lie between guard words that stay intact, and the map's block is bit for bit what it was.
    -> (nearest [M] int32 or None, sums [20])."""
    from point_sam_amd import _lib, ops
    lib = _lib.load()
    q = _dev(np.ascontiguousarray(qry, dtype=f32))
    M = len(qry)
    V = m.num_voxels if V is None else V
    n_ws = lib.psam_track_workspace_bytes(M) // 8
    assert n_ws == -(-M // 64) * 20
    buf = torch.full((3 * GUARD_WORDS + 20 + n_ws,), GUARD, dtype=torch.float64, device="cuda")
    sums = buf[GUARD_WORDS:GUARD_WORDS + 20]
    ws = buf[2 * GUARD_WORDS + 20:2 * GUARD_WORDS + 20 + n_ws]
    near = torch.full((M + 2 * GUARD_WORDS,), -99, dtype=torch.int32, device="cuda") if nearest else None
    bits = None if take is None else _dev(_pack(take, garbage))
    skipw = None if skip is None else _dev(_pack(np.asarray(skip, dtype=bool)[:V], garbage=False))
    words = ops.transfer_pose(pose)
    P = None if words is None else (ctypes.c_float * 12)(*[float(w) for w in words])
    before = m._block.clone()
    st = lib.psam_track_step(m._block.data_ptr(), m._block.numel() * 8, m.max_voxels, m.max_pairs, V, None if skipw is None else skipw.data_ptr(), min_count,
                             reach, float(r2), q.data_ptr(), M, None if bits is None else bits.data_ptr(), None if P is None else ctypes.addressof(P),
                             None if near is None else near[GUARD_WORDS:].data_ptr(), sums.data_ptr(), ws.data_ptr(), n_ws * 8,
                             torch.cuda.current_stream().cuda_stream)
    assert st == 0, lib.psam_last_error_string()
    torch.cuda.synchronize()
    assert torch.equal(m._block, before), "the map block is only read"
    host = buf.cpu().numpy()
    guards = np.concatenate([host[:GUARD_WORDS], host[GUARD_WORDS + 20:2 * GUARD_WORDS + 20], host[2 * GUARD_WORDS + 20 + n_ws:]])
    assert (guards == GUARD).all(), "a guard word around sums or the workspace was written"
    if near is not None:
        n = near.cpu().numpy()
        assert (n[:GUARD_WORDS] == -99).all() and (n[GUARD_WORDS + M:] == -99).all()
        near = n[GUARD_WORDS:GUARD_WORDS + M]
    return near, host[GUARD_WORDS:GUARD_WORDS + 20].copy()


def _check_case(case, exact=False):
    """The device's step equals the reference's -> (nearest, sums) of the reference."""
    m, ref = _shared_map(case)
    want_near, want, mass = TR.reference(case, ref)
    radius = case.get("radius", case["h"])
    reach = case.get("reach") or TR.reach_of(radius, case["h"])
    near, got = _raw_step(m, case["qry"], TR.r2_of(radius), reach, case.get("pose"), case.get("take"), case.get("V"), case.get("skip"), case.get("min_count", 1))
    bad = np.nonzero(near != want_near)[0]
    assert len(bad) == 0, (len(bad), bad[:5], near[bad[:5]], want_near[bad[:5]])
    assert got[0] == want[0] == (want_near >= 0).sum() and got[19] == want[19], (got[[0, 19]], want[[0, 19]])
    err = np.abs(got - want)
    bound = np.zeros(20) if exact else len(case["qry"]) * U * mass
    print(f"{case['name']}: M = {len(case['qry'])}, V = {ref.V}, reach {reach}: pairs {int(got[0])}, with a cell {int(got[19])}, max |error| / bound = "
          f"{'exact' if exact else float(np.max(err[1:19] / np.maximum(bound[1:19], 1e-300)))}")
    assert (err <= bound).all(), (np.nonzero(err > bound)[0], got, want, bound)
    return want_near, want


# ------------------------------------------------------------------------------------------------ the step
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_step_equals_the_reference(ops, case):
    near, sums = _check_case(case)
    if case["name"] == "tie and q == r2":
        assert near.tolist() == [0, 2, 4, 6, 8, 10, -1]
    if case["name"] == "skip hands on":
        assert near.tolist() == [-1, 2] and sums[0] == 1 and sums[19] == 2
    if case["name"] == "full table":
        assert _shared_map(case)[0].num_voxels == 32 == case["max_voxels"]


def test_lattice_case_is_exact(ops):
    near, sums = _check_case(TR.lattice_case(), exact=True)
    assert (near >= 0).sum() > 300 and (near < 0).sum() > 100 and sums[19] == 700


def test_a_wider_cube_with_the_same_r2_gives_the_same_words(ops):
    by = {c["name"]: c for c in CASES}
    case = by["reach 1"]
    m, _ = _shared_map(case)
    runs = [_raw_step(m, case["qry"], TR.r2_of(case["h"]), reach, case["pose"]) for reach in (1, 2, 4)]
    for near, sums in runs[1:]:
        assert np.array_equal(near, runs[0][0]) and np.array_equal(sums.view(np.int64), runs[0][1].view(np.int64))


def test_counts_above_one_pair_with_the_clouds_bits(ops):
    case = {c["name"]: c for c in CASES}["sizes M=257"]
    m, ref = _shared_map(case)
    assert int(m.counts().max()) > 1
    cloud = m.cloud()[0].cpu().numpy()
    assert np.array_equal(cloud.view(np.int32), TR.means(ref).view(np.int32))
    near, sums = _raw_step(m, case["qry"], TR.r2_of(case["h"]), 1, case["pose"])
    several = (near >= 0) & (np.asarray(ref.count)[np.maximum(near, 0)] > 1)
    assert several.sum() > 20
    s = cloud[near[near >= 0]].astype(np.float64)
    assert abs(sums[5] - s[:, 0].sum()) <= 257 * U * np.abs(s[:, 0]).sum()


def test_two_calls_and_no_nearest_give_the_same_words_and_all_bits_are_no_bits(ops):
    case = {c["name"]: c for c in CASES}["sizes M=2113"]
    m, _ = _shared_map(case)
    r2 = TR.r2_of(case["h"])
    runs = [_raw_step(m, case["qry"], r2, 1, case["pose"], nearest=n)[1].view(np.int64) for n in (True, True, False)]
    runs.append(_raw_step(m, case["qry"], r2, 1, case["pose"], take=np.ones(2113, dtype=bool))[1].view(np.int64))
    for other in runs[1:]:
        assert np.array_equal(runs[0], other)


def test_wrappers_give_the_entrys_words(ops):
    case = {c["name"]: c for c in CASES}["skip"]
    m, ref = _shared_map(case)
    take = np.random.default_rng(5).uniform(size=300) < 0.7
    want = _raw_step(m, case["qry"], TR.r2_of(2 * case["h"]), 2, case["pose"], take, None, case["skip"], 2)
    skip = _dev(_pack(case["skip"][:ref.V], garbage=False))
    sums, near = m.track_step(_dev(case["qry"]), case["pose"], 2 * case["h"], _dev(_pack(take)), skip, 2, return_nearest=True)
    assert sums.dtype == torch.float64 and sums.shape == (20,) and near.dtype == torch.int32 and near.shape == (300,)
    assert np.array_equal(near.cpu().numpy(), want[0]) and np.array_equal(sums.cpu().numpy().view(np.int64), want[1].view(np.int64))
    alone = m.track_step(_dev(case["qry"]), case["pose"], 2 * case["h"], _dev(_pack(take)), skip, 2)
    assert torch.equal(alone, sums)
    default = m.track_step(_dev(case["qry"]))                    # radius None: the voxel size
    assert np.array_equal(default.cpu().numpy().view(np.int64), _raw_step(m, case["qry"], TR.r2_of(case["h"]), 1)[1].view(np.int64))
    with pytest.raises(ValueError, match="at most 4"):
        m.track_step(_dev(case["qry"]), None, 4.5 * case["h"])


def test_a_dead_map_and_an_empty_map_raise(ops):
    from point_sam_amd.align import AlignConfig
    from point_sam_amd.scanmap import MapOverflow, ScanMap
    q = _dev(np.zeros((10, 3), dtype=f32))
    cfg = AlignConfig(radius=0.25)
    m = ScanMap(0.125, 4)
    for call in (lambda: m.track_step(q), lambda: m.track(q, cfg)):
        with pytest.raises(ValueError, match="empty"):
            call()
    pts = np.random.default_rng(0).uniform(-0.9, 0.9, (50, 3)).astype(f32)
    with pytest.raises(MapOverflow):
        m.add(_dev(pts), _dev(np.zeros_like(pts)))
    for call in (lambda: m.track_step(q), lambda: m.track(q, cfg)):
        with pytest.raises(MapOverflow):
            call()


def test_nearest_equals_align_step_on_the_maps_cloud(ops):
    """The seed at which the two numpy references agree on every query (tests/test_track_cpu.py asserts it): the cloud's row is the voxel id and the
    tie rule is the same, so the two kernels must agree on every query too."""
    case = TR.random_case(0)
    (m, ref), q, r = _shared_map(case), case["qry"], case["h"]
    assert np.array_equal(m.cloud()[0].cpu().numpy().view(np.int32), TR.means(ref).view(np.int32))
    near = _raw_step(m, q, TR.r2_of(r), 1)[0]
    other = ops.align_step(ops.transfer_index(m.cloud()[0].contiguous(), r), _dev(q), return_nearest=True)[1].cpu().numpy()
    assert (near != other).sum() == 0 and np.array_equal(near, TR.step(ref, q, r)[0])


def test_entry_refusals_leave_sums_and_nearest_untouched(ops):
    from point_sam_amd import _lib
    lib = _lib.load()
    case = TR.lattice_case()
    m, ref = _shared_map(case)
    q = _dev(case["qry"])
    M = len(case["qry"])
    sums = torch.full((20,), GUARD, dtype=torch.float64, device="cuda")
    near = torch.full((M,), -99, dtype=torch.int32, device="cuda")
    ws = torch.zeros(lib.psam_track_workspace_bytes(M) // 8, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    good = dict(map=m._block.data_ptr(), map_bytes=m._block.numel() * 8, max_voxels=m.max_voxels, max_pairs=m.max_pairs, V=ref.V, skip=None, min_count=1, reach=1,
                r2=float(TR.r2_of(case["h"])), qry=q.data_ptr(), M=M, qry_bits=None, pose=None, nearest=near.data_ptr(), sums=sums.data_ptr(), ws=ws.data_ptr(),
                ws_bytes=ws.numel() * 8)
    call = lambda **kw: lib.psam_track_step(*{**good, **kw}.values(), stream)
    nan_pose = (ctypes.c_float * 12)(*([1.0] * 11 + [float("nan")]))
    for code, kw in ((-1, dict(map=None)), (-1, dict(M=0)), (-1, dict(V=m.max_voxels + 1)), (-1, dict(max_pairs=0)), (-1, dict(reach=5)), (-1, dict(reach=0)),
                     (-1, dict(min_count=0)), (-1, dict(r2=float("nan"))), (-1, dict(pose=ctypes.addressof(nan_pose))),
                     (-2, dict(map=m._block.data_ptr() + 8)), (-2, dict(sums=sums.data_ptr() + 4)), (-2, dict(skip=ws.data_ptr() + 4)),
                     (-2, dict(qry=q.data_ptr() + 2)), (-2, dict(nearest=near.data_ptr() + 1)),
                     (-3, dict(ws_bytes=ws.numel() * 8 - 1)), (-3, dict(map_bytes=lib.psam_map_bytes(m.max_voxels, m.max_pairs) - 1))):
        assert call(**kw) == code, (kw, lib.psam_last_error_string())
        assert lib.psam_last_error_string().decode().startswith("psam_track_step")
    torch.cuda.synchronize()
    assert bool((sums == GUARD).all()) and bool((near == -99).all())
    assert call() == 0
    want_near, want, _ = TR.reference(case, ref)
    assert np.array_equal(sums.cpu().numpy(), want) and np.array_equal(near.cpu().numpy(), want_near)


# ------------------------------------------------------------------------------------------------ the loop, on the fixture tests/test_track_cpu.py verifies
ROTATION_MARGIN = max(10 * TR.REF_ROTATION_ERROR, 1e-6)       # ten times the reference loop's recorded error against the truth: 6.3695e-2 rad
TRANSLATION_MARGIN = max(10 * TR.REF_TRANSLATION_ERROR, 1e-6)  # 2.3991e-2


def _same_alignment(a, b):
    return (np.array_equal(a.pose.view(np.int64), b.pose.view(np.int64)) and (a.pairs, a.coverage, a.rms, a.iterations, a.converged, a.reason) ==
            (b.pairs, b.coverage, b.rms, b.iterations, b.converged, b.reason) and a.history == b.history)


@pytest.fixture(scope="module")
def loop(ops):
    from point_sam_amd.scanmap import ScanMap
    ref, a, b = TR.loop_case()
    m = ScanMap(TR.LOOP_H, TR.LOOP_MAX_VOXELS)
    m.add(_dev(a), _dev(np.zeros_like(a)))
    assert m.num_voxels == ref.V == TR.REF_LOOP_VOXELS
    return m, ref, _dev(b), b


def _config():
    from point_sam_amd.align import AlignConfig
    return AlignConfig(radius=TR.LOOP_RADIUS, final_radius=TR.LOOP_FINAL, shrink=TR.LOOP_SHRINK)


def test_track_on_the_device_converges_to_the_truth(ops, loop):
    m, ref, qry, b = loop
    before = m._block.clone()
    out = m.track(qry, _config(), TR.LOOP_INIT)
    rot, tr = AR.pose_error(out.pose)
    print(f"device track: {out.iterations} steps (reference {TR.REF_LOOP_ITERATIONS}), {out.pairs} pairs, coverage {out.coverage:.4f}, rms {out.rms:.6f}, "
          f"rotation error {rot:.4e} rad (margin {ROTATION_MARGIN:.4e}), translation error {tr:.4e} (margin {TRANSLATION_MARGIN:.4e}), {out.reason}")
    assert out.converged and out.reason == "fixed point" and out.iterations == len(out.history)
    assert rot <= ROTATION_MARGIN and tr <= TRANSLATION_MARGIN
    assert out.pairs == TR.REF_LOOP_PAIRS and out.coverage == 1.0 and out.history[0][2] == TR.LOOP_RADIUS and out.history[-1][2] == TR.LOOP_FINAL
    assert _same_alignment(out, m.track(qry, _config(), TR.LOOP_INIT)), "run to run"
    assert torch.equal(m._block, before)
    with pytest.raises(ValueError, match="at most 4"):
        from point_sam_amd.align import AlignConfig
        m.track(qry, AlignConfig(radius=4.5 * TR.LOOP_H))


def test_track_pairs_no_freed_voxel(ops, loop):
    """occupied= a mask that frees a slab of voxels (the floor's cells and the ones above): no pair of the final step lies in the slab."""
    m, ref, qry, b = loop
    cloud = m.cloud()[0]
    slab = cloud[:, 2] < -0.25
    assert 50 < int(slab.sum()) < ref.V - 50
    out = m.track(qry, _config(), TR.LOOP_INIT, occupied=~slab)
    assert out.pairs >= 16 and out.pairs < TR.REF_LOOP_PAIRS
    skip = _pack(slab.cpu().numpy(), garbage=False)
    radius = out.history[-1][2]
    # the pairs of the last step were found under the pose before its solve; at a fixed point that pose has the same fp32 words
    near = m.track_step(qry, out.pose, radius, None, _dev(skip), 1, return_nearest=True)[1]
    hit = near[near >= 0].long()
    assert hit.numel() > 0 and not bool(slab[hit].any())
    if out.converged:
        assert hit.numel() == out.pairs
    plain = m.track_step(qry, out.pose, radius, return_nearest=True)[1]
    assert bool(slab[plain[plain >= 0].long()].any()), "without the mask the same pose does pair into the slab"
    with pytest.raises(ValueError, match="occupied"):
        m.track(qry, _config(), occupied=slab[:-1])
    assert _same_alignment(m.track(qry, _config(), TR.LOOP_INIT, occupied=True), m.track(qry, _config(), TR.LOOP_INIT)), "never carved: everything is occupied"


# ------------------------------------------------------------------------------------------------ the predictor
@pytest.fixture(scope="module")
def pred():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd.model import PointCloudSAM
    from point_sam_amd.predictor import PointSAMPredictor
    cfg = get_config("tiny")
    return PointSAMPredictor(PointCloudSAM(cfg, random_state_dict(cfg, 3), "cuda", precision="f16x3"))


def test_predictor_map_align_and_map_nearest(ops, pred, loop):
    from point_sam_amd.scanmap import ScanMap
    _, _, _, b = loop
    ref, a, _ = TR.loop_case()
    g = np.random.default_rng(4)
    labels = g.integers(-1, 5, size=len(a)).astype(np.int32)
    m, lab_ref = ScanMap(TR.LOOP_H, TR.LOOP_MAX_VOXELS), SM.RefMap(TR.LOOP_H, TR.LOOP_MAX_VOXELS)
    pred.set_scene(_dev(a), torch.zeros(len(a), 3, device="cuda"), max_points=1024)
    assert not pred.scene.identity
    pred.map_add(m, _dev(labels))
    lab_ref.add(a, np.zeros_like(a), labels)
    # under the identity every point of the scan has a voxel of its own; where that voxel's mean is the nearest, map_nearest is map_lookup
    near_ref = TR.step(lab_ref, a, TR.LOOP_H)[0]
    own = lab_ref.locate(a)
    vote = lab_ref.labels()[0]
    got, looked = pred.map_nearest(m).cpu().numpy(), pred.map_lookup(m).cpu().numpy()
    assert np.array_equal(got, np.where(near_ref >= 0, vote[np.maximum(near_ref, 0)], -1))
    same = near_ref == own
    assert same.sum() > 1000 and np.array_equal(got[same], looked[same])
    # the next scan: map_align is m.track on the coordinates map_add would add -- the full-resolution points, not the working cloud
    xyz = _dev(b)
    pred.set_scene(xyz, torch.zeros(len(b), 3, device="cuda"), max_points=1024)
    cfg = _config()
    out = pred.map_align(m, cfg, TR.LOOP_INIT)
    assert _same_alignment(out, m.track(xyz, cfg, TR.LOOP_INIT)) and out.converged
    mask = g.uniform(size=len(b)) < 0.5
    part = pred.map_align(m, cfg, TR.LOOP_INIT, _dev(_pack(mask, garbage=False)), min_count=2)
    assert _same_alignment(part, m.track(xyz, cfg, TR.LOOP_INIT, _dev(_pack(mask, garbage=False)), None, 2)) and part.pairs <= mask.sum()
    pose = out.pose
    want = TR.step(lab_ref, b, 2 * TR.LOOP_H, pose.astype(f32))[0]
    got = pred.map_nearest(m, pose, 2 * TR.LOOP_H, min_votes=2).cpu().numpy()
    assert np.array_equal(got, np.where(want >= 0, lab_ref.labels(2)[0][np.maximum(want, 0)], -1)) and (got >= 0).sum() > 1000
    for bad in (0, True, 1.5):
        with pytest.raises(ValueError, match="min_votes"):
            pred.map_nearest(m, min_votes=bad)
    with pytest.raises(ValueError, match="empty"):
        pred.map_nearest(ScanMap(TR.LOOP_H, 64))
    pred.set_crop((0.0, 0.0, 0.0), 0.5)
    with pytest.raises(RuntimeError):
        pred.map_align(m, cfg)
    pred.clear_crop()
