"""One ICP step and the ICP loop on the GPU (csrc/align.hip, ops.align_step, point_sam_amd/align.py, predictor.align) against the plain numpy reference
tests/align_reference.py.  `nearest` and the two counts are always exact.  The other sums are exact where every term is a small multiple of a power of
two (the lattice inputs: no addition rounds in any order) and otherwise within M * 2^-53 * sum |term| of the exactly rounded value: the first-order
bound of M rounded additions, while a term of the device's sum passes through at most 2 + 6 + ceil(ceil(M / 64) / 32) + 32 of them."""
import ctypes

import numpy as np
import pytest
import torch

import align_reference as A
import transfer_reference as T
from point_sam_amd.config import get_config
from point_sam_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu
f32 = np.float32
U = 2.0 ** -53


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd import ops
    return ops


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _pack(take, garbage=True):
    """[M] bool -> [ceil(M / 64)] int64 words in mask_pack's layout; the bits past M are SET (the entry must ignore them)."""
    M = len(take)
    pad = np.ones(-(-M // 64) * 64, dtype=bool) if garbage else np.zeros(-(-M // 64) * 64, dtype=bool)
    pad[:M] = take
    return (pad.reshape(-1, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(1, dtype=np.uint64).view(np.int64)


def _device_step(ops, index, qry, pose=None, radius=None, take=None, nearest=True):
    out = ops.align_step(index, _dev(qry), pose, radius, None if take is None else _dev(_pack(take)), return_nearest=nearest)
    sums, near = out if nearest else (out, None)
    assert sums.dtype == torch.float64 and sums.shape == (20,) and sums.is_cuda
    if nearest:
        assert near.dtype == torch.int32 and near.shape == (len(qry),)
    return (None if near is None else near.cpu().numpy()), sums.cpu().numpy()


def _check_step(ops, src, r, qry, pose=None, radius=None, take=None, exact=False):
    """The device's step equals the reference's -> (nearest, sums) of the reference."""
    src, qry = np.ascontiguousarray(src, dtype=f32), np.ascontiguousarray(qry, dtype=f32)
    want_near, want, mass = A.step(src, r, qry, pose, radius, take)
    near, got = _device_step(ops, ops.transfer_index(_dev(src), r), qry, pose, radius, take)
    bad = np.nonzero(near != want_near)[0]
    assert len(bad) == 0, (len(bad), bad[:5], near[bad[:5]], want_near[bad[:5]])
    assert got[0] == want[0] == (want_near >= 0).sum() and got[19] == want[19], (got[[0, 19]], want[[0, 19]])
    err = np.abs(got - want)
    bound = np.zeros(20) if exact else len(qry) * U * mass
    print(f"M = {len(qry)}: pairs {int(got[0])}, with a cell {int(got[19])}, max |error| / bound = "
          f"{'exact' if exact else float(np.max(err[1:19] / np.maximum(bound[1:19], 1e-300)))}")
    assert (err <= bound).all(), (np.nonzero(err > bound)[0], got, want, bound)
    return want_near, want


# ------------------------------------------------------------------------------------------------ the step
@pytest.mark.parametrize("radius", [None, 0.125])
def test_lattice_case_is_exact(ops, radius):
    """901 sources, 1543 queries, r = 0.25, no pose: every term is a small multiple of a power of two, so all 20 sums are exact in any order; then
    the same index searched at half the radius."""
    src, qry, r = T.lattice_case()
    near, sums = _check_step(ops, src, r, qry, None, radius, exact=True)
    assert (near >= 0).sum() > 300 and (near < 0).sum() > 300 and sums[19] > sums[0]
    assert (sums[0] == 611) if radius is None else (sums[0] == 373)                     # fewer of the same candidates


def test_lattice_case_posed(ops):
    src, qry, r = T.lattice_case()
    near, _ = _check_step(ops, src, r, qry, T.POSE)
    assert (near >= 0).sum() > 100


@pytest.mark.parametrize("r", [0.05, 0.11])
@pytest.mark.parametrize("posed", [False, True])
def test_uniform_cases(ops, r, posed):
    src, qry = T.uniform_case()
    near, sums = _check_step(ops, src, r, qry, T.POSE if posed else None)
    assert (near >= 0).mean() > 0.3 and sums[19] <= len(qry)


def test_a_smaller_search_radius_on_a_coarser_index(ops):
    src, qry = T.uniform_case()
    near, _ = _check_step(ops, src, 0.11, qry, T.POSE, 0.05)
    same, _, _ = A.step(src, 0.05, qry, T.POSE)                                        # here the 27 cells of either index hold the radius-0.05 search
    assert np.array_equal(near, same)


@pytest.mark.parametrize("N,M", [(1, 1543), (901, 1), (901, 257), (901, 1025)])
def test_single_source_single_query_one_past_a_block_one_past_a_wave(ops, N, M):
    src, qry, r = T.lattice_case()
    src = src[:N]
    if N == 1:
        qry = np.concatenate([src, src + f32(0.125), qry], 0)                          # an exact hit and a lone candidate among them
    if M == 1:
        qry = src[5:6]                                                                 # the one query has a pair
    near, sums = _check_step(ops, src, r, qry[:M], exact=True)
    assert near.shape == (M,) and sums[0] >= (2 if N == 1 else 1)


def test_queries_out_of_reach(ops):
    """Beyond the cell range: no query has a cell, all 20 sums are zero.  In range but far from every source: 19 zeros and the count of queries with a cell."""
    src, qry, r = T.lattice_case()
    index = ops.transfer_index(_dev(src), r)
    near, sums = _device_step(ops, index, (qry + f32(1e6)).astype(f32))
    assert (near == -1).all() and np.array_equal(sums, np.zeros(20)) and not np.signbit(sums).any()
    near, sums = _device_step(ops, index, (qry + f32(100)).astype(f32))
    assert (near == -1).all() and np.array_equal(sums[:19], np.zeros(19)) and sums[19] == len(qry)
    _check_step(ops, src, r, (qry + f32(100)).astype(f32), exact=True)


def test_queries_without_a_cell_are_neither_paired_nor_counted(ops):
    src, qry, r = T.lattice_case()
    odd = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e6, 0, 0], [-1e6, -1e6, 1e6], [np.nan, np.nan, np.nan]], dtype=f32)
    mixed = np.concatenate([odd[:3], qry[:700], odd[3:], qry[700:]], 0).astype(f32)
    near, sums = _check_step(ops, src, r, mixed, exact=True)
    plain_near, plain = A.step(src, r, qry)[:2]
    assert np.array_equal(sums, plain) and np.isfinite(sums).all()                     # the six add nothing, not even to sums[19]
    assert (near[:3] == -1).all() and (near[703:706] == -1).all() and np.array_equal(np.delete(near, [0, 1, 2, 703, 704, 705]), plain_near)


def test_one_long_chain_with_duplicates_a_tie_goes_to_the_lower_index(ops):
    g = np.random.default_rng(3)
    src = (g.integers(0, 16, size=(300, 3)).astype(f32) / f32(64)).astype(f32)      # one cell of 0.25: a chain of 300, many exact duplicates
    src[0] = 0                                                                      # pins the origin: the cell is [0, 0.25)^3
    src[200:] = src[100:200]                                                        # every one of these twice
    assert len(T.index(src, 0.25, T.parameters(src, 0.25)[0])) == 1
    qry = np.concatenate([(g.integers(-16, 32, size=(700, 3)).astype(f32) / f32(64)).astype(f32), src[200:]], 0)
    near, _ = _check_step(ops, src, 0.25, qry, exact=True)
    first = np.array([np.nonzero((src == p).all(1))[0][0] for p in src[200:]])
    assert np.array_equal(near[700:], first) and (near[700:] < 200).all()             # q = 0 at both copies (or more): the lowest index


def test_bits_select_an_irregular_subset(ops):
    """M = 1543 is no multiple of 64 and the bits past M are set: the result is the reference's restricted to the subset."""
    src, qry, r = T.lattice_case()
    g = np.random.default_rng(8)
    take = g.uniform(size=len(qry)) < 0.37
    take[64:128] = False                                                               # a whole word, hence a whole wave, without a participant
    take[1536:] = [True, False, True, True, False, False, True]
    near, sums = _check_step(ops, src, r, qry, None, None, take, exact=True)
    assert (near[~take] == -1).all() and 0 < sums[0] < sums[19] <= take.sum()
    sub_near, sub, _ = A.step(src, r, qry[take])
    assert np.array_equal(sums, sub) and np.array_equal(near[take], sub_near)
    # posed, rounded sums: the bound; and all bits set is no bits at all
    usrc, uqry = T.uniform_case()
    utake = g.uniform(size=len(uqry)) < 0.5
    _check_step(ops, usrc, 0.11, uqry, T.POSE, 0.07, utake)
    index = ops.transfer_index(_dev(usrc), 0.11)
    every = _device_step(ops, index, uqry, T.POSE, take=np.ones(len(uqry), dtype=bool))
    none = _device_step(ops, index, uqry, T.POSE)
    assert np.array_equal(every[0], none[0]) and np.array_equal(every[1].view(np.int64), none[1].view(np.int64))


def test_without_nearest_the_sums_are_the_same_words_and_two_calls_agree(ops):
    src, qry = T.uniform_case()
    a = ops.transfer_index(_dev(src), 0.11)
    b = ops.transfer_index(_dev(src), 0.11)                                            # another arrival order inside the chains
    runs = [_device_step(ops, ix, qry, T.POSE, nearest=n)[1].view(np.int64) for ix, n in ((a, True), (a, True), (a, False), (b, False))]
    for other in runs[1:]:
        assert np.array_equal(runs[0], other)


def test_entry_refusals_leave_the_sums_untouched(ops):
    from point_sam_amd import _lib
    lib = _lib.load()
    src, qry, r = T.lattice_case()
    index = ops.transfer_index(_dev(src), r)
    q = _dev(qry)
    sums = torch.full((20,), -7.25, dtype=torch.float64, device="cuda")
    ws = torch.zeros(lib.psam_align_workspace_bytes(len(qry)) // 8, dtype=torch.float64, device="cuda")
    org = (ctypes.c_float * 3)(*index.origin)
    stream = torch.cuda.current_stream().cuda_stream
    good = dict(src=index.src_xyz.data_ptr(), N=len(src), index_ws=index.ws.data_ptr(), index_ws_bytes=index.ws.numel() * 8, origin=ctypes.addressof(org),
                inv_h=float(index.inv_h), r2=float(index.r2), qry=q.data_ptr(), M=len(qry), qry_bits=None, pose=None, nearest=None, sums=sums.data_ptr(),
                ws=ws.data_ptr(), ws_bytes=ws.numel() * 8)
    call = lambda **kw: lib.psam_align_step(*{**good, **kw}.values(), stream)
    nan_pose = (ctypes.c_float * 12)(*([1.0] * 11 + [float("nan")]))
    for code, kw in ((-1, dict(r2=float("nan"))), (-1, dict(M=0)), (-1, dict(ws=None)), (-1, dict(pose=ctypes.addressof(nan_pose))),
                     (-2, dict(qry=q.data_ptr() + 2)), (-2, dict(sums=sums.data_ptr() + 4)), (-2, dict(index_ws=index.ws.data_ptr() + 8)),
                     (-3, dict(ws_bytes=ws.numel() * 8 - 1)), (-3, dict(index_ws_bytes=lib.psam_transfer_index_workspace_bytes(len(src)) - 1))):
        assert call(**kw) == code, (kw, lib.psam_last_error_string())
    torch.cuda.synchronize()
    assert bool((sums == -7.25).all())
    assert call() == 0
    want = A.step(src, r, qry)[1]
    assert np.array_equal(sums.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ the loop, on the fixture tests/test_align_cpu.py verifies
ROTATION_MARGIN = max(10 * A.REF_ROTATION_ERROR, 1e-6)        # ten times the reference ICP's recorded error against the truth: 1.4141e-2 rad
TRANSLATION_MARGIN = max(10 * A.REF_TRANSLATION_ERROR, 1e-6)  # 2.9329e-3


def _config():
    from point_sam_amd.align import AlignConfig
    return AlignConfig(A.ICP_RADIUS, A.ICP_FINAL, A.ICP_SHRINK, A.ICP_ITERATIONS)


def _share(bits_a, bits_b, M):
    """Per row the share of the M points whose bit is the same in both."""
    x = (bits_a ^ bits_b).cpu().numpy().view(np.uint64)
    return 1 - np.array([sum(bin(int(w)).count("1") for w in row) for row in x]) / M


def _same_alignment(a, b):
    return (np.array_equal(a.pose.view(np.int64), b.pose.view(np.int64)) and (a.pairs, a.coverage, a.rms, a.iterations, a.converged, a.reason) ==
            (b.pairs, b.coverage, b.rms, b.iterations, b.converged, b.reason) and a.history == b.history)


def test_icp_on_the_device_converges_to_the_truth(ops):
    """The device's pose may differ from the reference's by an fp32 ulp on the way, which can change a handful of pairs: it is held against the
    TRUTH, within ten times the reference ICP's own error (tests/align_reference.py: REF_*), and by what it does to the carried masks: the same
    packed bits as under the true pose on at least the share of points the reference ICP's pose achieves (6097 of 6100, measured on the CPU)."""
    from point_sam_amd import align as X, transfer as S
    a, b = A.icp_case()
    src, qry = _dev(a), _dev(b)
    out = X.icp(ops.transfer_index(src, A.ICP_RADIUS), qry, _config())
    rot, tr = A.pose_error(out.pose)
    print(f"device ICP: {out.iterations} steps, {out.pairs} pairs, coverage {out.coverage:.4f}, rms {out.rms:.6f}, rotation error {rot:.4e} rad "
          f"(margin {ROTATION_MARGIN:.4e}), translation error {tr:.4e} (margin {TRANSLATION_MARGIN:.4e}), {out.reason}")
    assert out.converged and out.reason == "fixed point" and out.iterations == len(out.history) < A.ICP_ITERATIONS
    assert rot <= ROTATION_MARGIN and tr <= TRANSLATION_MARGIN
    assert out.pairs > 6000 and out.coverage > 0.98 and 0.005 < out.rms < 0.02 and out.history[0][2] == A.ICP_RADIUS and out.history[-1][2] == A.ICP_FINAL
    assert _same_alignment(out, X.icp(ops.transfer_index(src, A.ICP_RADIUS), qry, _config()))      # run to run
    rows = _dev(A.mask_rows(a))
    same = _share(*[S.transfer_bits(S.build_plan(src, qry, A.TRANSFER_RADIUS, pose), rows)[0] for pose in (A.TRUE_POSE, out.pose)], len(b))
    print(f"share of points with the same bit as under the true pose: {same.tolist()} (the reference ICP's pose: {A.REF_MASK_SHARE})")
    assert same.min() >= A.REF_MASK_SHARE
    # an object alone: the sphere's queries against the whole source cloud
    sphere = np.abs(np.linalg.norm(b.astype(np.float64) @ A.TRUE_POSE[:, :3].T + A.TRUE_POSE[:, 3] - np.array([0.15, 0.1, -0.05]), axis=1) - 0.2) < 1e-3
    part = X.icp(ops.transfer_index(src, A.ICP_RADIUS), qry, _config(), bits=_dev(_pack(sphere, garbage=False)))
    assert part.pairs <= sphere.sum() < 2000 and part.pairs > 0.9 * sphere.sum() and part.coverage > 0.9


# ------------------------------------------------------------------------------------------------ the predictor
@pytest.fixture(scope="module")
def scans(ops):
    """The fixture's cloud A as a scene with a snapshot of two objects, then cloud B as the current scene; both are their own working clouds."""
    from point_sam_amd.model import PointCloudSAM
    from point_sam_amd.predictor import PointSAMPredictor
    cfg = get_config("tiny")
    pred = PointSAMPredictor(PointCloudSAM(cfg, random_state_dict(cfg, 3), "cuda", precision="f16x3"))
    a, b = A.icp_case()
    axyz, bxyz = _dev(a), _dev(b)
    pred.set_scene(axyz, torch.full_like(axyz, 0.5), max_points=8192)
    snap = pred.snapshot(_dev(A.mask_rows(a)))
    assert torch.equal(snap.coords, axyz)
    pred.set_scene(bxyz, torch.full_like(bxyz, 0.5), max_points=8192)
    assert torch.equal(pred._state.coords[0], bxyz)
    return pred, snap, bxyz


def test_predictor_align_equals_icp_composed_from_public_calls(ops, scans):
    from point_sam_amd import align as X
    pred, snap, bxyz = scans
    init = np.concatenate([A.rotation([0, 0, 1], 1.0), [[0.01], [0.0], [0.0]]], 1)
    take = torch.zeros(ops.mask_words(len(bxyz)), dtype=torch.int64, device="cuda")
    take[:40] = -1                                                                     # the first 2560 working points
    for kw in (dict(), dict(init=init), dict(mask=take)):
        got = pred.align(snap, _config(), **kw)
        want = X.icp(ops.transfer_index(snap.coords, A.ICP_RADIUS), pred._state.coords[0].contiguous(), _config(), kw.get("init"), kw.get("mask"))
        assert _same_alignment(got, want), kw
        assert got.pose.shape == (3, 4) and got.pose.dtype == np.float64
    full = pred.align(snap, _config())
    rot, tr = A.pose_error(full.pose)
    assert full.converged and rot <= ROTATION_MARGIN and tr <= TRANSLATION_MARGIN
    # the pose passes straight to transfer_masks
    est, _, covered = pred.transfer_masks(snap, A.TRANSFER_RADIUS, full.pose)
    true, _, _ = pred.transfer_masks(snap, A.TRANSFER_RADIUS, A.TRUE_POSE)
    assert _share(est, true, len(bxyz)).min() >= A.REF_MASK_SHARE and int(covered) > 0.99 * len(bxyz)


def test_predictor_align_refuses_a_crop_and_a_non_snapshot(ops, scans):
    pred, snap, _ = scans
    with pytest.raises(TypeError, match="Snapshot"):
        pred.align((snap.coords, snap.logits), _config())
    with pytest.raises(TypeError, match="AlignConfig"):
        pred.align(snap, A.ICP_RADIUS)
    pred.set_crop((0.0, 0.0, 0.0), 0.9, max_points=2048)
    try:
        with pytest.raises(RuntimeError, match="crop"):
            pred.align(snap, _config())
    finally:
        pred.clear_crop()
    assert pred.align(snap, _config()).converged


# ------------------------------------------------------------------------------------------------ the demo
def _write_ply(path, pts):
    with open(path, "w") as f:
        f.write(f"ply\nformat ascii 1.0\nelement vertex {len(pts)}\nproperty float x\nproperty float y\nproperty float z\n"
                "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
        f.writelines(f"{p[0]!r} {p[1]!r} {p[2]!r} 128 128 128\n" for p in pts.tolist())


def test_propagate_route_with_align_returns_the_pose_and_without_it_answers_as_before(ops, scans, tmp_path):
    """The fixture's clouds through the demo: A (with two far points that keep B inside the unit ball of A's normalisation) is loaded and clicked, B
    follows by /propagate with "align" from the identity.  The pose is held against the truth in the normalised coordinates, with the margins above
    (the translation's divided by the scale); the reference ICP on these normalised clouds converges to 1.4141e-3 rad and 2.540e-4.  A second session
    that is GIVEN the returned pose and no "align" answers with the fields of before, equal value for value."""
    import http.client
    import json
    import threading
    from point_sam_amd.demo_server import DemoSession, serve
    from point_sam_amd.predictor import PointSAMPredictor
    a, b = A.icp_case()
    a = np.concatenate([a.astype(np.float64), [[1.1, 1.0, 0.9], [-1.2, -1.1, -1.0]]], 0)
    _write_ply(tmp_path / "a.ply", a)
    _write_ply(tmp_path / "b.ply", b.astype(np.float64))
    shift = a.mean(0)
    scale = np.linalg.norm(a - shift, axis=1).max()
    Rm, t = A.TRUE_POSE[:, :3], A.TRUE_POSE[:, 3]
    truth = np.concatenate([Rm, ((Rm @ shift + t - shift) / scale)[:, None]], 1)       # A_n = R B_n + (R c + t - c) / s
    model = scans[0].model

    def session(body):
        sess = DemoSession(PointSAMPredictor(model), models_dir=str(tmp_path), output_dir=str(tmp_path / "results"))
        srv = serve(sess, "127.0.0.1", 0)
        threading.Thread(target=srv.serve_forever, daemon=True).start()

        def req(method, path, data=None):
            c = http.client.HTTPConnection("127.0.0.1", srv.server_address[1], timeout=120)
            c.request(method, path, None if data is None else json.dumps(data), {"Content-Type": "application/json"})
            r = c.getresponse()
            return r.status, json.loads(r.read())
        try:
            st, cloud = req("GET", "/pointcloud/a.ply")
            assert st == 200 and len(cloud["xyz"]) == 3 * len(a)
            k = int(np.argmin(np.linalg.norm(a - np.array([0.15, 0.1, 0.15]), axis=1)))      # the top of the sphere
            st, seg = req("POST", "/segment", {"prompt_point": cloud["xyz"][3 * k:3 * k + 3], "prompt_label": 1})
            assert st == 200, seg
            return req("POST", "/propagate", dict({"pointcloud": "b.ply", "radius": A.TRANSFER_RADIUS}, **body))
        finally:
            srv.shutdown()

    fields = {"radius": A.ICP_RADIUS, "final_radius": A.ICP_FINAL, "shrink": A.ICP_SHRINK, "iterations": A.ICP_ITERATIONS}
    st, out = session({"align": fields})
    assert st == 200, out
    pose = np.array(out["pose"])
    rot, tr = A.pose_error(pose, truth)
    print(f"/propagate with align: {out['align']}, rotation error {rot:.4e} rad, translation error {tr:.4e} (normalised; scale {scale:.4f})")
    assert pose.shape == (3, 4) and rot <= ROTATION_MARGIN and tr <= TRANSLATION_MARGIN / scale
    stats = out["align"]
    assert set(stats) == {"pairs", "coverage", "rms", "iterations", "converged"} and stats["converged"] is True
    assert stats["pairs"] > 6000 and stats["coverage"] > 0.98 and 0 < stats["rms"] < 0.02 / scale and 1 < stats["iterations"] < A.ICP_ITERATIONS
    st, plain = session({"pose": out["pose"]})
    assert st == 200 and set(plain) == {"xyz", "rgb", "objects", "lost", "scores"} == set(out) - {"pose", "align"}
    assert all(plain[k] == out[k] for k in plain)
    assert len(plain["objects"]) == 1 and len(plain["objects"][0]["seg"]) == len(b) and plain["xyz"] == ((b.astype(np.float64) - shift) / scale).flatten().tolist()
