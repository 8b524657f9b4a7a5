"""The scan map without a GPU: the properties of its definition (tests/scanmap_reference.py: the dictionary form and the np.unique form held equal),
scanmap.labels_from_logits, every refusal of ops.map_* and ScanMap that comes before device work, the header / binding sync of the psam_map_* entries
and the demo's /map routes against a stand-in predictor that answers from the reference."""
import http.client
import json
import os
import re
import threading

import numpy as np
import pytest
import torch

import scanmap_reference as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("psam_map_bytes", "psam_map_clear", "psam_map_add_workspace_bytes", "psam_map_add", "psam_map_locate", "psam_map_labels", "psam_map_cloud",
                "psam_map_fields")
H = 2.0 ** -4


def _two_scans(seed=0):
    """5000 uniform points, then 4000 posed ones with a NaN and an infinity among them; random labels in -1 .. 4."""
    rng = np.random.default_rng(seed)
    a_xyz = rng.uniform(-1, 1, (5000, 3)).astype(np.float32)
    a_rgb = rng.uniform(-1, 1, (5000, 3)).astype(np.float32)
    b_xyz = rng.uniform(-0.9, 0.9, (4000, 3)).astype(np.float32)
    b_rgb = rng.uniform(-1, 1, (4000, 3)).astype(np.float32)
    b_xyz[17, 1], b_xyz[2900, 0], b_rgb[555, 2] = np.nan, np.inf, np.nan
    return (a_xyz, a_rgb, rng.integers(-1, 5, 5000).astype(np.int32)), (b_xyz, b_rgb, rng.integers(-1, 5, 4000).astype(np.int32)), SM.rotation_pose()


@pytest.fixture(scope="module")
def two_scans():
    a, b, pose = _two_scans()
    ref, fast = SM.RefMap(H, 1 << 14), SM.FastMap(H, 1 << 14)
    out = [(ref.add(*a), fast.add(*a)), (ref.add(*b, pose), fast.add(*b, pose))]
    return a, b, pose, ref, fast, out


def _same_map(ref, fast):
    for x, y in zip(ref.fields(), fast.fields()):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    for mv in (1, 2, 3):
        for x, y in zip(ref.labels(mv), fast.labels(mv)):
            assert np.array_equal(x, y)
    for x, y in zip(ref.cloud(), fast.cloud()):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))


def test_both_forms_of_the_reference_agree(two_scans):
    a, b, pose, ref, fast, out = two_scans
    for (ids_r, *counts_r), (ids_f, *counts_f) in out:
        assert np.array_equal(ids_r, ids_f) and counts_r == counts_f
    _same_map(ref, fast)
    assert np.array_equal(ref.locate(b[0], pose), fast.locate(b[0], pose)) and np.array_equal(ref.locate(a[0]), fast.locate(a[0]))
    # the second scan met old and new voxels, rejected points, and tied votes
    ids2, new2, acc2, rej2 = out[1][0]
    V1 = out[0][0][1]
    assert rej2 >= 3 and new2 > 0 and ((ids2 >= 0) & (ids2 < V1)).sum() > 0 and ref.V == V1 + new2
    label, votes = ref.labels()
    tied = sum(1 for v in range(ref.V) if sum(1 for (u, l), n in ref.pairs.items() if u == v and n == votes[v]) > 1 and votes[v] > 0)
    assert tied > 50, "random labels in -1 .. 4 exercise the tie rule"


def test_locate_of_a_scan_returns_the_ids_of_its_add(two_scans):
    a, b, pose, ref, fast, out = two_scans
    ok_b = SM.point_terms(b[0], b[1], pose, ref.inv_h)[0]
    assert np.array_equal(ref.locate(a[0]), out[0][0][0])
    loc = ref.locate(b[0], pose)
    assert np.array_equal(loc[ok_b], out[1][0][0][ok_b])
    assert SM.point_terms(b[0], None, pose, ref.inv_h)[0][555] and not ok_b[555] and out[1][0][0][555] == -1, \
        "a bad colour rejects the point of an add; a locate has no colours and tests the position alone"
    assert ref.locate(np.array([[np.nan, 0, 0], [0, 2, 0]], dtype=np.float32)).tolist() == [-1, -1]


def test_ids_are_stable_and_new_ids_follow_the_lowest_point_index(two_scans):
    a, b, pose, ref, fast, out = two_scans
    one = SM.RefMap(H, 1 << 14)
    ids1, new1, acc1, rej1 = one.add(*a)
    assert new1 == one.V and rej1 == 0 and acc1 == 5000
    # the first point of every voxel, in index order, carries ids 0, 1, 2, ...
    firsts = [ids1.tolist().index(v) for v in range(one.V)]
    assert firsts == sorted(firsts) and ids1[0] == 0
    keys_before, first_before = list(one.keys), list(one.first)
    ids2, new2, _, _ = one.add(*b, pose)
    assert one.keys[:len(keys_before)] == keys_before and one.first[:len(first_before)] == first_before
    fresh = ids2[ids2 >= len(keys_before)]
    _, where = np.unique(fresh, return_index=True)
    assert np.array_equal(np.sort(where), where), "new ids grow with the lowest accepted point index"
    assert set(one.first[len(keys_before):]) == {2} and set(one.last[v] for v in set(ids2[ids2 >= 0].tolist())) == {2}
    assert any(l == 1 for l in one.last), "a voxel the second scan did not touch keeps last_seen 1"


def test_per_key_state_does_not_depend_on_the_order_of_the_points(two_scans):
    a, b, pose, ref, fast, out = two_scans
    rng = np.random.default_rng(5)
    pa, pb = rng.permutation(5000), rng.permutation(4000)
    other = SM.RefMap(H, 1 << 14)
    other.add(a[0][pa], a[1][pa], a[2][pa])
    other.add(b[0][pb], b[1][pb], b[2][pb], pose)
    assert other.by_key() == ref.by_key()
    assert other.keys != ref.keys, "the ids follow the order, the per-key state does not"


def test_every_centroid_lies_in_its_own_voxel(two_scans):
    a, b, pose, ref, fast, out = two_scans
    xyz, rgb = ref.cloud()
    assert np.array_equal(ref.locate(xyz), np.arange(ref.V))
    assert (np.abs(rgb) <= 1).all()


def test_ties_go_to_the_lower_label_and_min_votes_cuts():
    m = SM.RefMap(0.5, 16)
    p = np.array([[0.1, 0.1, 0.1]] * 7 + [[-0.6, 0.1, 0.1]] * 3 + [[0.1, -0.6, 0.1]], dtype=np.float32)
    lab = np.array([7, 3, 7, 3, 9, -1, -5, 2 ** 31 - 1, 2 ** 31 - 1, 0, -1], dtype=np.int32)
    ids, new, acc, rej = m.add(p, np.zeros_like(p), lab)
    assert ids.tolist() == [0] * 7 + [1] * 3 + [2] and (new, acc, rej) == (3, 11, 0)
    label, votes = m.labels()
    assert label.tolist() == [3, 2 ** 31 - 1, -1] and votes.tolist() == [2, 2, 0]
    assert m.labels(2)[0].tolist() == [3, 2 ** 31 - 1, -1] and m.labels(3)[0].tolist() == [-1, -1, -1] and m.labels(3)[1].tolist() == [0, 0, 0]
    m.add(p[:1], np.zeros((1, 3), np.float32), np.array([7], dtype=np.int32))
    assert m.labels()[0][0] == 7 and m.labels()[1][0] == 3, "a majority flips when another vote arrives"
    assert m.fields()[0].tolist() == [8, 3, 1]
    fast = SM.FastMap(0.5, 16)
    fast.add(p, np.zeros_like(p), lab)
    fast.add(p[:1], np.zeros((1, 3), np.float32), np.array([7], dtype=np.int32))
    _same_map(m, fast)


def test_acceptance_at_the_boundary_and_rejection_past_it():
    xyz, rgb, accepted = SM.boundary_case()
    for Map in (SM.RefMap, SM.FastMap):
        m = Map(H, 64)
        ids, new, acc, rej = m.add(xyz, rgb, np.arange(len(xyz), dtype=np.int32))
        assert np.array_equal(ids >= 0, accepted) and acc == accepted.sum() and rej == (~accepted).sum()
        assert m.fields()[0].sum() == acc
    # the fixed point of -1, 0 and 1, and the mean that comes back
    q, ok = SM.fixed(np.array([-1, 0, 1, 0.5], dtype=np.float32))
    assert ok.all() and q.tolist() == [0, 1 << 20, 1 << 21, 3 << 19]
    assert SM.mean(1 << 21, 1) == 1.0 and SM.mean(0, 5) == -1.0 and SM.mean(3 << 20, 2) == 0.5
    # a pose that carries part of a scan out of [-1, 1]
    m = SM.RefMap(H, 64)
    shift = np.array([[1, 0, 0, 0.5], [0, 1, 0, 0], [0, 0, 1, 0]], dtype=np.float64)
    p = np.array([[0.4, 0, 0], [0.5, 0, 0], [0.6, 0, 0]], dtype=np.float32)
    assert (m.add(p, np.zeros_like(p), None, shift)[0] >= 0).tolist() == [True, True, False]


def test_overflow_is_a_function_of_the_inputs_and_kills_the_map():
    a, _, _ = _two_scans()
    full = SM.RefMap(H, 1 << 14)
    full.add(*a)
    V, pairs = full.V, len(full.pairs)
    for Map in (SM.RefMap, SM.FastMap):
        assert Map(H, V, pairs).add(*a)[1] == V
        for caps in ((V - 1, pairs), (V, pairs - 1)):
            m = Map(H, *caps)
            with pytest.raises(SM.RefOverflow):
                m.add(*a)
            with pytest.raises(SM.RefOverflow):
                m.add(*a)


def test_labels_from_logits():
    from point_sam_amd.scanmap import labels_from_logits
    inf, nan = float("inf"), float("nan")
    logits = torch.tensor([[1.0, -1.0, 0.0, nan, -inf, 2.0, 0.5],
                           [0.5, -2.0, -0.25, -inf, -inf, 1.0, nan],
                           [-inf, -inf, -inf, -inf, -inf, -inf, -inf]])
    assert labels_from_logits(logits).tolist() == [0, -1, -1, -1, -1, 0, 0]
    assert labels_from_logits(logits, ids=[10, 2 ** 31 - 1, 5]).tolist() == [10, -1, -1, -1, -1, 10, 10]
    assert labels_from_logits(logits, threshold=0.75).tolist() == [0, -1, -1, -1, -1, 0, -1]
    assert labels_from_logits(logits, threshold=-1.5).tolist() == [0, 0, 0, -1, -1, 0, 0]
    assert labels_from_logits(logits[1:2], ids=torch.tensor([4])).tolist() == [4, -1, -1, -1, -1, 4, -1]
    assert labels_from_logits(logits).dtype == torch.int32
    for bad in (logits[0], logits.double(), "x"):
        with pytest.raises((ValueError, TypeError)):
            labels_from_logits(bad)
    for ids in ([1, 2], [1, 2, -3], [1.0, 2.0, 3.0], [1, 2, 2 ** 31]):
        with pytest.raises(ValueError):
            labels_from_logits(logits, ids=ids)
    with pytest.raises(ValueError):
        labels_from_logits(logits, threshold=nan)


def test_header_and_binding_declare_the_same_map_entries():
    from point_sam_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "pointsam_hip.h")).read()
    declared = set(re.findall(r"\b(psam_map_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(ENTRY_POINTS) == {n for n in _lib.SIGNATURES if n.startswith("psam_map_")}
    assert int(re.search(r"#define PSAM_MAP_HEADER_INTS (\d+)", hdr).group(1)) == ops.MAP_HEADER_INTS


def test_sizes_and_refusals_of_the_c_entries_before_any_launch():
    """No GPU is touched and nothing is launched: every call here is a size query or is refused by the argument checks, which come before any launch.
    The pointers are addresses inside a host buffer, as in the sibling CPU tests; no call that would pass every check is made."""
    from point_sam_amd import _lib
    from point_sam_amd.build import build_library
    build_library()
    lib = _lib.load()
    cap = lambda n: max(64, 1 << (2 * n - 1).bit_length())
    a16 = lambda b: (b + 15) & ~15
    for mv, mp in ((1, 1), (100, 7), (4096, 8192), (1 << 20, 1 << 21)):
        want = 64 + a16(cap(mv) * 8) + a16(cap(mv) * 4) + a16(cap(mp) * 8) + a16(cap(mp) * 4) + mv * 64 + a16(mv * 8) + a16(mv * 8)
        assert lib.psam_map_bytes(mv, mp) == want
    for bad in (0, -1, (1 << 28) + 1):
        assert lib.psam_map_bytes(bad, 4) == 0 and lib.psam_map_bytes(4, bad) == 0 and lib.psam_map_add_workspace_bytes(bad) == 0
    M = 1000
    ws_bytes = lib.psam_map_add_workspace_bytes(M)
    assert ws_bytes == a16(cap(M) * 8) + a16(cap(M) * 4) + a16(M * 4) + a16((1 + 1) * 4) + a16(cap(M) * 4) + 16
    nbytes = lib.psam_map_bytes(64, 128)
    import ctypes
    host = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(host) + 15) & ~15                       # 16-byte aligned, inside the host buffer; every call below is refused first
    q = p + (1 << 15)
    err = lambda: lib.psam_last_error_string().decode()
    pose = (_lib.f32 * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    bad_pose = (_lib.f32 * 12)(1, 0, 0, 0, 0, float("nan"), 0, 0, 0, 0, 1, 0)
    assert lib.psam_map_clear(None, nbytes, 64, 128, 16.0, None) == -1 and "null pointer" in err()
    assert lib.psam_map_clear(p, nbytes, 0, 128, 16.0, None) == -1 and "max_voxels" in err()
    assert lib.psam_map_clear(p, nbytes, 64, (1 << 28) + 1, 16.0, None) == -1
    assert lib.psam_map_clear(p, nbytes - 1, 64, 128, 16.0, None) == -3 and "psam_map_bytes" in err()
    assert lib.psam_map_clear(p + 8, nbytes, 64, 128, 16.0, None) == -2 and "aligned" in err()
    for inv_h in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.psam_map_clear(p, nbytes, 64, 128, inv_h, None) == -1 and "inv_h" in err()
    add = lambda map_=p, nb=nbytes, xyz=p, rgb=p, M_=M, pose_=None, ids=p, ws=q, wb=ws_bytes: lib.psam_map_add(map_, nb, 64, 128, xyz, rgb, None, M_, pose_, ids, ws, wb, None)
    for kw in ({"map_": None}, {"xyz": None}, {"rgb": None}, {"ids": None}, {"ws": None}):
        assert add(**kw) == -1 and "null pointer" in err()
    for m in (0, -5, (1 << 28) + 1):
        assert add(M_=m) == -1 and "2^28" in err()
    assert add(pose_=ctypes.addressof(bad_pose)) == -1 and "pose must be finite" in err()
    assert add(nb=nbytes - 1) == -3 and add(wb=ws_bytes - 1) == -3 and "psam_map_add_workspace_bytes" in err()
    assert add(ws=q + 4) == -2 and add(map_=p + 4) == -2
    assert lib.psam_map_locate(p, nbytes, 64, 128, None, M, None, p, None) == -1
    assert lib.psam_map_locate(p, nbytes, 64, 128, p, 0, None, p, None) == -1
    assert lib.psam_map_locate(p, nbytes, 64, 128, p, M, ctypes.addressof(bad_pose), p, None) == -1
    assert lib.psam_map_locate(p, nbytes - 1, 64, 128, p, M, ctypes.addressof(pose), p, None) == -3
    for V in (0, 65, -1):                                         # V outside 1 .. max_voxels: refused by all three read-outs
        assert lib.psam_map_labels(p, nbytes, 64, 128, V, 1, p, p, None) == -1 and "V" in err()
        assert lib.psam_map_cloud(p, nbytes, 64, 128, V, p, p, None) == -1 and "V" in err()
        assert lib.psam_map_fields(p, nbytes, 64, 128, V, p, p, p, p, p, None) == -1 and "V" in err()
    for mv in (0, -3):                                            # min_votes is an argument of psam_map_labels alone
        assert lib.psam_map_labels(p, nbytes, 64, 128, 1, mv, p, p, None) == -1 and "min_votes" in err()
    assert lib.psam_map_labels(p, nbytes, 64, 128, 8, 1, None, p, None) == -1 and lib.psam_map_cloud(p, nbytes, 64, 128, 8, p, None, None) == -1
    assert lib.psam_map_fields(p, nbytes, 64, 128, 8, None, None, None, None, None, None) == -1
    assert lib.psam_map_fields(p, nbytes, 64, 128, 8, None, None, None, p + 4, None, None) == -2
    assert lib.psam_map_fields(p, nbytes, 64, 128, 8, None, None, None, None, p + 4, None) == -2


def test_wrappers_refuse_bad_arguments_before_device_work():
    from point_sam_amd import ops
    from point_sam_amd.scanmap import ScanMap
    for bad in (0, -1.0, float("nan"), float("inf"), 1e-40, 1e39, "x", None, True):
        with pytest.raises(ValueError):
            ops.map_inv_h(bad)
        with pytest.raises(ValueError):
            ScanMap(bad, 64, device="cpu")
    assert ops.map_inv_h(2 ** -7) == np.float32(128)
    for bad in (0, -3, (1 << 28) + 1, 2.5, "x", True, None):
        with pytest.raises(ValueError):
            ops.map_capacities(bad)
        with pytest.raises(ValueError):
            ScanMap(0.25, bad, device="cpu")
        if bad is not None:
            with pytest.raises(ValueError):
                ops.map_capacities(64, bad)
            with pytest.raises(ValueError):
                ScanMap(0.25, 64, bad, device="cpu")
    assert ops.map_capacities(100) == (100, 200) and ops.map_capacities(1 << 28) == (1 << 28, 1 << 28) and ops.map_capacities(5, 3) == (5, 3)
    block = torch.zeros(ops.map_bytes(64, 128) // 8 + 2, dtype=torch.int64)
    xyz, rgb = torch.zeros(10, 3), torch.zeros(10, 3)
    lab = torch.zeros(10, dtype=torch.int32)
    with pytest.raises(TypeError):
        ops.map_add(block, 64, 128, "x", rgb)
    with pytest.raises(TypeError):
        ops.map_add(block, 64, 128, xyz.double(), rgb)
    with pytest.raises(TypeError):
        ops.map_add(block, 64, 128, xyz, rgb.half())
    with pytest.raises(ValueError):
        ops.map_add(block, 64, 128, torch.zeros(10, 2), rgb)
    with pytest.raises(ValueError):
        ops.map_add(block, 64, 128, torch.zeros(0, 3), torch.zeros(0, 3))
    with pytest.raises(ValueError):
        ops.map_add(block, 64, 128, xyz, rgb[:9])
    with pytest.raises(TypeError):
        ops.map_add(block, 64, 128, xyz, rgb, lab.long())
    with pytest.raises(TypeError):
        ops.map_add(block, 64, 128, xyz, rgb, [0] * 10)
    with pytest.raises(ValueError):
        ops.map_add(block, 64, 128, xyz, rgb, lab[:9])
    for pose in (np.eye(3), [[1, 0, 0, 0]] * 3 + [[0, 0, 0, 2]], np.full((3, 4), np.nan), "x"):
        with pytest.raises(ValueError):
            ops.map_add(block, 64, 128, xyz, rgb, lab, pose)
        with pytest.raises(ValueError):
            ops.map_locate(block, 64, 128, xyz, pose)
    with pytest.raises(TypeError):
        ops.map_add("x", 64, 128, xyz, rgb)
    with pytest.raises(TypeError):
        ops.map_add(block.int(), 64, 128, xyz, rgb)
    with pytest.raises(ValueError):
        ops.map_add(block, 0, 128, xyz, rgb)
    with pytest.raises(ValueError):
        ops.map_locate(block, 64, 128, torch.zeros(3))
    with pytest.raises(TypeError):
        ops.map_locate(block, 64, 128, np.zeros((3, 3), dtype=np.float32))
    for fn in (ops.map_labels, ops.map_cloud, ops.map_fields):
        for V in (0, 65, 2.0, True):
            with pytest.raises(ValueError):
                fn(block, 64, 128, V)
        with pytest.raises(TypeError):
            fn([1, 2], 64, 128, 8)
    for mv in (0, -1, 1.5, 2 ** 31):
        with pytest.raises(ValueError):
            ops.map_labels(block, 64, 128, 8, mv)
    with pytest.raises(ValueError):
        ops.map_clear(block, 64, 128, 0.0)
    with pytest.raises(TypeError):
        ops.map_clear(None, 64, 128, 0.25)
    with pytest.raises(TypeError):
        ops.map_header("x")
    # the same block is too short for a larger map: refused by the size check, still before any device work ...
    with pytest.raises(ValueError):
        ops.map_labels(block, 4096, 8192, 8)
    # ... and a block that passes every check but lives on the CPU is the project's "no CPU fallback" error
    from point_sam_amd._lib import PointSamHipError
    with pytest.raises(PointSamHipError):
        ops.map_cloud(block, 64, 128, 8)


def test_predictor_map_entries_refuse_before_any_cloud():
    from point_sam_amd.predictor import PointSAMPredictor
    pred = PointSAMPredictor(model=None)
    with pytest.raises(TypeError):
        pred.map_add("not a map")
    with pytest.raises(TypeError):
        pred.map_lookup(None)


# ------------------------------------------------------------------------------------------------ the demo's routes
class _RefScanMap:
    """scanmap.ScanMap's surface over the reference."""

    def __init__(self, voxel_size, max_voxels):
        self.ref = SM.RefMap(voxel_size, max_voxels)

    num_voxels = property(lambda self: self.ref.V)
    num_adds = property(lambda self: self.ref.adds)

    def cloud(self):
        return tuple(torch.from_numpy(a) for a in self.ref.cloud())

    def labels(self, min_votes=1):
        return tuple(torch.from_numpy(a) for a in self.ref.labels(min_votes))

    def clear(self):
        self.ref.clear()


class FakeMapper:
    """set_pointcloud as tests/test_demo_server_cpu.py's stand-in; new_map / map_add answer from the reference."""

    def __init__(self):
        self.adds = []

    def set_pointcloud(self, xyz, rgb):
        self.xyz, self.rgb = xyz, rgb

    def new_map(self, voxel_size, max_voxels):
        return _RefScanMap(voxel_size, max_voxels)

    def map_add(self, m, labels=None, pose=None):
        from point_sam_amd.scanmap import AddResult, MapOverflow
        self.adds.append((labels.clone(), pose))
        try:
            ids, new, acc, rej = m.ref.add(self.xyz[0].numpy(), self.rgb[0].numpy(), None if labels is None else labels.numpy(), pose)
        except SM.RefOverflow as e:
            raise MapOverflow(f"ScanMap: {e}") from None
        return AddResult(torch.from_numpy(ids), new, acc, rej)


def _req(port, path, body=None):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=20)
    c.request("POST", path, None if body is None else json.dumps(body), {"Content-Type": "application/json"})
    r = c.getresponse()
    return r.status, json.loads(r.read())


def _upload(port, xyz, rgb):
    st, _ = _req(port, "/sampled_pointcloud", {"points": {str(i): float(v) for i, v in enumerate(xyz.flatten())},
                                               "colors": {str(i): float(v) for i, v in enumerate(rgb.flatten())}})
    assert st == 200


def test_map_routes_answer_from_the_reference():
    from point_sam_amd.demo_server import DemoSession, build_parser, serve
    args = build_parser().parse_args(["--map-voxel-size", "0.25", "--map-max-voxels", "12"])
    assert (args.map_voxel_size, args.map_max_voxels) == (0.25, 12) and build_parser().parse_args([]).map_max_voxels == 1 << 20
    for bad in ({"map_voxel_size": 0.0}, {"map_max_voxels": 0}):
        with pytest.raises(ValueError):
            DemoSession(FakeMapper(), device="cpu", **bad)
    pred = FakeMapper()
    srv = serve(DemoSession(pred, device="cpu", map_voxel_size=0.25, map_max_voxels=12), "127.0.0.1", 0)      # 24 pairs
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    try:
        port = srv.server_address[1]
        assert _req(port, "/map/add", {})[0] == 400 and _req(port, "/map", {})[0] == 400
        rng = np.random.default_rng(3)
        xyz = rng.uniform(-0.1, 0.1, (40, 3)).astype(np.float32)      # the eight voxels around the origin, three labels: inside both capacities
        rgb = rng.uniform(0, 1, (40, 3)).astype(np.float32)
        lab = rng.integers(-1, 3, 40).astype(int).tolist()
        _upload(port, xyz, rgb)
        assert _req(port, "/map", {})[0] == 400, "before any add the map is empty"
        ref = SM.RefMap(0.25, 12)
        for body, pose in (({"labels": lab}, None), ({"labels": lab, "pose": SM.rotation_pose(5, 5, (0.05, 0, 0)).tolist()}, SM.rotation_pose(5, 5, (0.05, 0, 0))), ({}, None)):
            want = ref.add(xyz, rgb, np.asarray(body.get("labels", [-1] * 40), dtype=np.int32), pose)
            st, out = _req(port, "/map/add", body)
            assert st == 200 and (out["new_voxels"], out["accepted"], out["rejected"]) == want[1:] and out["num_voxels"] == ref.V and out["num_adds"] == ref.adds
        assert pred.adds[2][0].tolist() == [-1] * 40, "without labels and without kept masks every point is unlabelled"
        for body, mv in (({}, 1), ({"min_votes": 2}, 2)):
            st, out = _req(port, "/map", body)
            assert st == 200
            cx, cr = ref.cloud()
            label, votes = ref.labels(mv)
            assert np.array_equal(np.asarray(out["xyz"], dtype=np.float32).reshape(-1, 3).view(np.int32), cx.view(np.int32))
            assert np.array_equal(np.asarray(out["rgb"], dtype=np.float32).reshape(-1, 3).view(np.int32), cr.view(np.int32))
            assert out["labels"] == label.tolist() and out["votes"] == votes.tolist()
        n = len(pred.adds)
        for bad in ({"labels": lab[:-1]}, {"labels": [0.5] * 40}, {"labels": [2 ** 31] * 40}, {"labels": "x"}, {"pose": [[1, 0, 0]]}, {"other": 1}, [1]):
            assert _req(port, "/map/add", bad)[0] == 400, bad
        for bad in ({"min_votes": 0}, {"min_votes": 1.5}, {"min_votes": True}, {"x": 1}, [2]):
            assert _req(port, "/map", bad)[0] == 400, bad
        assert len(pred.adds) == n, "a refused request never reaches the predictor"
        # a full map is a 400, and /map/clear revives it
        t = np.linspace(-0.9, 0.9, 20)
        far = np.concatenate([np.stack([t, -t, np.zeros(20)], 1), np.stack([t, t, np.full(20, 0.6)], 1)]).astype(np.float32)      # 16 voxels
        _upload(port, far, rgb)
        st, out = _req(port, "/map/add", {})
        assert st == 400 and "MapOverflow" not in out["error"] and "ScanMap" in out["error"]
        assert _req(port, "/map/clear")[0] == 200
        _upload(port, xyz, rgb)
        st, out = _req(port, "/map/add", {"labels": lab})
        assert st == 200 and out["num_adds"] == 1
    finally:
        srv.shutdown()
