"""Scan map carving without a GPU: the reference walk (tests/carve_reference.py) against the geometric definition in exact rationals, its closed-form
entry, the header / binding sync of the psam_carve_* entries, their sizes and every refusal that comes before a launch, the wrappers' refusals,
occupied()'s arithmetic and the demo's routes against a stand-in predictor that answers from the reference."""
import ctypes
import http.client
import itertools
import json
import os
import re
import threading

import numpy as np
import pytest
import torch

import carve_reference as CR
import scanmap_reference as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("psam_carve_bytes", "psam_carve_clear", "psam_carve_workspace_bytes", "psam_carve_scan", "psam_carve_fields")
MAP_ENTRY_POINTS = ("psam_map_bytes", "psam_map_clear", "psam_map_add_workspace_bytes", "psam_map_add", "psam_map_locate", "psam_map_labels", "psam_map_cloud",
                    "psam_map_fields")


# ------------------------------------------------------------------------------------------------ the walk
def test_walk_equals_the_geometric_definition_on_a_5_cubed_grid():
    cells = list(itertools.product(range(5), repeat=3))
    touched = 0
    for o in cells:
        for e in cells:
            if e < o:
                continue                                           # the other direction is checked through the symmetry below
            w = CR.walk(o, e)
            assert len(set(w)) == len(w) and set(w) == CR.geometric(o, e), (o, e)
            assert CR.walk(e, o) == w[::-1], (o, e)
            path = [o] + w + [e]
            assert all(CR.chebyshev(a, b) == 1 for a, b in zip(path, path[1:])) or o == e, (o, e)
            touched += len(w) < sum(abs(e[a] - o[a]) for a in range(3)) - 1
    assert touched > 1000, "many pairs pass through an edge or a corner: the tie rule is exercised"
    assert CR.walk((0, 0, 0), (0, 0, 0)) == [] and CR.walk((1, 1, 1), (2, 2, 2)) == [] and CR.walk((0, 0, 0), (2, 2, 0)) == [(1, 1, 0)]
    assert CR.walk((0, 0, 0), (2, 1, 0)) == [(1, 0, 0), (1, 1, 0)], "t = 1/4 (x), 1/2 (y), 3/4 (x): no tie"


def test_walk_hand_cases():
    # (0,0) -> (4,2): x crosses at 1/8, 3/8, 5/8, 7/8; y at 1/4, 3/4: no ties, five cells between
    assert CR.walk((0, 0, 0), (4, 2, 0)) == [(1, 0, 0), (1, 1, 0), (2, 1, 0), (3, 1, 0), (3, 2, 0)]
    # (0,0) -> (3,1): x at 1/6, 3/6, 5/6; y at 1/2: a tie at 1/2, the corner between (1,0), (2,0), (1,1), (2,1) is passed through
    assert CR.walk((0, 0, 0), (3, 1, 0)) == [(1, 0, 0), (2, 1, 0)]
    assert CR.walk((5, 5, 5), (2, 8, 5)) == [(4, 6, 5), (3, 7, 5)]
    assert CR.walk((0, 0, 0), (3, 0, 0)) == [(1, 0, 0), (2, 0, 0)]


def test_the_kernels_difference_form_is_the_same_walk():
    cells = list(itertools.product(range(5), repeat=3))
    for o in cells:
        for e in cells:
            if o != e:
                assert CR.walk_by_differences(o, e) == CR.walk(o, e), (o, e)
    rng = np.random.default_rng(1)
    for trial in range(200):
        hi = (9, 70, 2000)[trial % 3]
        o, e = (tuple(int(v) for v in rng.integers(0, hi, 3)) for _ in range(2))
        if o == e:
            continue
        w = CR.walk(o, e)
        assert CR.walk_by_differences(o, e) == w, (o, e)
        for margin in (0, 1, 3):
            assert CR.walk_by_differences(o, e, margin) == [c for c in w if CR.chebyshev(c, e) > margin], (o, e, margin)


def test_closed_form_entry_equals_the_walk_on_random_pairs():
    rng = np.random.default_rng(0)
    for trial in range(300):
        hi = (6, 40, 3000)[trial % 3]
        o = tuple(int(v) for v in rng.integers(0, hi, 3))
        e = tuple(int(v) for v in rng.integers(0, hi, 3))
        n = [abs(e[a] - o[a]) for a in range(3)]
        if max(n) == 0:
            continue
        a = n.index(max(n))
        s = [CR._sign(e[b] - o[b]) for b in range(3)]
        full = [o] + CR.walk(o, e) + [e]
        # the state right after the k-th crossing of the longest axis = the first cell of the walk whose a-coordinate is o_a + k s_a
        for k in sorted({1, max(n) // 2 + 1, max(n)} | {int(v) for v in rng.integers(1, max(n) + 1, 3)}):
            kk = CR.entry(o, e, k)
            cell = tuple(o[b] + s[b] * kk[b] for b in range(3))
            first = next(c for c in full if c[a] == o[a] + k * s[a])
            assert cell == first, (o, e, k)
            rest = full[full.index(first) + 1:-1]
            assert CR.walk(o, e, kk) == rest, (o, e, k)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_and_binding_declare_the_same_carve_entries():
    from point_sam_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "pointsam_hip.h")).read()
    declared = set(re.findall(r"\b(psam_carve_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(ENTRY_POINTS) == {n for n in _lib.SIGNATURES if n.startswith("psam_carve_")}
    assert set(re.findall(r"\b(psam_map_[a-z0-9_]+)\s*\(", hdr)) == set(MAP_ENTRY_POINTS) == {n for n in _lib.SIGNATURES if n.startswith("psam_map_")}, \
        "carving adds no psam_map_* name"
    assert int(re.search(r"#define PSAM_CARVE_HEADER_INTS (\d+)", hdr).group(1)) == ops.CARVE_HEADER_INTS
    assert "scan map carving" in hdr


def test_sizes_and_refusals_of_the_c_entries_before_any_launch():
    """No GPU is touched and nothing is launched: every call here is a size query or is refused by the argument checks, which come before any launch.
    The pointers are addresses inside a host buffer; no call that would pass every check is made."""
    from point_sam_amd import _lib
    from point_sam_amd.build import build_library
    build_library()
    lib = _lib.load()
    cap = lambda n: max(64, 1 << (2 * n - 1).bit_length())
    a16 = lambda b: (b + 15) & ~15
    for mv in (1, 100, 4096, 1 << 20, 1 << 28):
        assert lib.psam_carve_bytes(mv) == 64 + 16 * mv
    for M in (1, 1000, 4097):
        assert lib.psam_carve_workspace_bytes(M) == a16(cap(M) * 8) + a16(cap(M) * 4) + 2 * a16(M * 4) + 16, "the table, rep, the ray list, the origin's key"
    for bad in (0, -1, (1 << 28) + 1):
        assert lib.psam_carve_bytes(bad) == 0 and lib.psam_carve_workspace_bytes(bad) == 0
    M, mv, mp = 1000, 64, 128
    map_bytes, carve_bytes, ws_bytes = lib.psam_map_bytes(mv, mp), lib.psam_carve_bytes(mv), lib.psam_carve_workspace_bytes(M)
    host = ctypes.create_string_buffer(1 << 18)
    p = (ctypes.addressof(host) + 15) & ~15                       # 16-byte aligned, inside the host buffer; every call below is refused first
    c, q = p + (1 << 16), p + (1 << 17)
    err = lambda: lib.psam_last_error_string().decode()
    addr = lambda arr: ctypes.addressof(arr)
    bad_pose = (_lib.f32 * 12)(1, 0, 0, 0, 0, float("nan"), 0, 0, 0, 0, 1, 0)
    inf_pose = (_lib.f32 * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, float("inf"))
    origin = (_lib.f32 * 3)(0.0, 0.0, 0.0)
    assert lib.psam_carve_clear(None, carve_bytes, mv, None) == -1 and "null pointer" in err()
    assert lib.psam_carve_clear(c, carve_bytes, 0, None) == -1 and "max_voxels" in err()
    assert lib.psam_carve_clear(c, carve_bytes, (1 << 28) + 1, None) == -1
    assert lib.psam_carve_clear(c, carve_bytes - 1, mv, None) == -3 and "psam_carve_bytes" in err()
    assert lib.psam_carve_clear(c + 8, carve_bytes, mv, None) == -2 and "aligned" in err()

    def scan(map_=p, mb=map_bytes, mv_=mv, mp_=mp, carve=c, cb=carve_bytes, xyz=p, M_=M, pose=None, origin_=addr(origin), margin=1, stamp=1, ws=q, wb=ws_bytes):
        return lib.psam_carve_scan(map_, mb, mv_, mp_, carve, cb, xyz, M_, pose, origin_, margin, stamp, ws, wb, None)
    for kw in ({"map_": None}, {"carve": None}, {"xyz": None}, {"origin_": None}, {"ws": None}):
        assert scan(**kw) == -1 and "null pointer" in err()
    for m in (0, -5, (1 << 28) + 1):
        assert scan(M_=m) == -1 and "2^28" in err()
    for margin in (-1, 1 << 21, 2 ** 31 - 1):
        assert scan(margin=margin) == -1 and "margin" in err()
    for stamp in (0, -1, -2 ** 31):
        assert scan(stamp=stamp) == -1 and "stamp" in err()
    for kw in ({"mv_": 0}, {"mp_": 0}, {"mv_": (1 << 28) + 1}):
        assert scan(**kw) == -1 and "max_voxels" in err()
    assert scan(pose=addr(bad_pose)) == -1 and "pose must be finite" in err()
    assert scan(pose=addr(inf_pose)) == -1 and "pose must be finite" in err()
    for i, v in itertools.product(range(3), (float("nan"), float("inf"), -float("inf"))):
        o = (_lib.f32 * 3)(0.0, 0.0, 0.0)
        o[i] = v
        assert scan(origin_=addr(o)) == -1 and "origin must be finite" in err()
    assert scan(mb=map_bytes - 1) == -3 and "psam_map_bytes" in err()
    assert scan(cb=carve_bytes - 1) == -3 and "psam_carve_bytes" in err()
    assert scan(wb=ws_bytes - 1) == -3 and "psam_carve_workspace_bytes" in err()
    assert scan(map_=p + 4) == -2 and scan(carve=c + 8) == -2 and scan(ws=q + 4) == -2 and "aligned" in err()
    for V in (0, mv + 1, -1):
        assert lib.psam_carve_fields(c, carve_bytes, mv, V, c, c, c, c, None) == -1 and "V" in err()
    assert lib.psam_carve_fields(c, carve_bytes, mv, 8, None, None, None, None, None) == -1 and "null pointer" in err()
    assert lib.psam_carve_fields(None, carve_bytes, mv, 8, c, c, c, c, None) == -1
    assert lib.psam_carve_fields(c, carve_bytes - 1, mv, 8, c, None, None, None, None) == -3
    assert lib.psam_carve_fields(c + 4, carve_bytes, mv, 8, c, None, None, None, None) == -2
    assert lib.psam_carve_fields(c, carve_bytes, 0, 8, c, None, None, None, None) == -1


# ------------------------------------------------------------------------------------------------ the wrappers
def _host_map(voxel_size=0.25, max_voxels=64):
    """A ScanMap whose block lives in host memory: the constructor's clear would be refused (no CPU fallback), so the object is put together by hand.
    Every call made on it here is refused before it reaches the block."""
    from point_sam_amd import ops
    from point_sam_amd.scanmap import ScanMap
    m = ScanMap.__new__(ScanMap)
    m.voxel_size, (m.max_voxels, m.max_pairs) = voxel_size, ops.map_capacities(max_voxels)
    m._block = torch.zeros(ops.map_bytes(m.max_voxels, m.max_pairs) // 8 + 2, dtype=torch.int64)
    m._V = m._adds = m._flags = m._carves = 0
    m._carve = None
    return m


def test_wrappers_refuse_bad_arguments_before_device_work():
    from point_sam_amd import ops
    from point_sam_amd._lib import PointSamHipError
    block = torch.zeros(ops.map_bytes(64, 128) // 8 + 2, dtype=torch.int64)
    carve = torch.zeros(ops.carve_bytes(64) // 8, dtype=torch.int64)
    assert ops.carve_bytes(64) == 64 + 16 * 64
    xyz = torch.zeros(10, 3)
    for bad in (0, -1, (1 << 28) + 1, 2.5, True, None):
        with pytest.raises(ValueError):
            ops.carve_bytes(bad)
    for bad in ("x", None, [0, 0], [0, 0, 0, 0], [[0, 0, 0]], [0, float("nan"), 0], [0, 0, float("inf")], [1e39, 0, 0], ["a", "b", "c"]):
        with pytest.raises(ValueError):
            ops.carve_origin(bad)
        with pytest.raises(ValueError):
            ops.carve_scan(block, 64, 128, carve, xyz, bad)
    assert ops.carve_origin([0, 0.5, 1]).tolist() == [0.0, 0.5, 1.0] and ops.carve_origin(torch.tensor([1.0, 2.0, 3.0])).dtype == np.float32
    # an origin without a cell: outside [-1, 1]^3 as it is, or carried out by the pose; exactly 1 is inside
    shift = np.array([[1, 0, 0, 0.5], [0, 1, 0, 0], [0, 0, 1, 0]], dtype=np.float64)
    assert ops.carve_origin([1, -1, 1], None, 0.25) is not None and ops.carve_origin([0.5, 0, 0], shift, 0.25) is not None
    for origin, pose in (([1.0001, 0, 0], None), ([0, -1.5, 0], None), ([0.6, 0, 0], shift), ([0, 0, 0], np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 3e38]]))):
        with pytest.raises(ValueError, match="no cell"):
            ops.carve_origin(origin, pose, 0.25)
        with pytest.raises(ValueError, match="no cell"):
            _host_map().carve(xyz, origin, pose)
    for margin in (-1, 1 << 21, 1.0, True, None):
        with pytest.raises(ValueError):
            ops.carve_scan(block, 64, 128, carve, xyz, [0, 0, 0], None, margin)
    for stamp in (0, -1, 2 ** 31, 1.0, True):
        with pytest.raises(ValueError):
            ops.carve_scan(block, 64, 128, carve, xyz, [0, 0, 0], None, 1, stamp)
    with pytest.raises(TypeError):
        ops.carve_scan(block, 64, 128, carve, "x", [0, 0, 0])
    with pytest.raises(TypeError):
        ops.carve_scan(block, 64, 128, carve, xyz.double(), [0, 0, 0])
    with pytest.raises(ValueError):
        ops.carve_scan(block, 64, 128, carve, torch.zeros(0, 3), [0, 0, 0])
    with pytest.raises(ValueError):
        ops.carve_scan(block, 64, 128, carve, torch.zeros(10, 2), [0, 0, 0])
    for pose in (np.eye(3), np.full((3, 4), np.nan), "x"):
        with pytest.raises(ValueError):
            ops.carve_scan(block, 64, 128, carve, xyz, [0, 0, 0], pose)
    with pytest.raises(TypeError):
        ops.carve_scan("x", 64, 128, carve, xyz, [0, 0, 0])
    with pytest.raises(ValueError):
        ops.carve_scan(block, 0, 128, carve, xyz, [0, 0, 0])
    with pytest.raises(ValueError):
        ops.carve_scan(block, 4096, 8192, carve, xyz, [0, 0, 0])                  # the map block is too short for that map
    for bad in ("x", None, [1, 2]):
        with pytest.raises(TypeError):
            ops.carve_scan(block, 64, 128, bad, xyz, [0, 0, 0])
        with pytest.raises(TypeError):
            ops.carve_clear(bad, 64)
        with pytest.raises(TypeError):
            ops.carve_fields(bad, 64, 8)
        with pytest.raises(TypeError):
            ops.carve_header(bad)
    with pytest.raises(TypeError):
        ops.carve_clear(carve.int(), 64)
    with pytest.raises(ValueError):
        ops.carve_scan(block, 64, 128, carve[:-1], xyz, [0, 0, 0])
    with pytest.raises(ValueError):
        ops.carve_clear(carve, 65)
    for V in (0, 65, 2.0, True):
        with pytest.raises(ValueError):
            ops.carve_fields(carve, 64, V)
    # blocks that pass every check but live on the CPU: the project's "no CPU fallback" error, before any launch
    for call in (lambda: ops.carve_clear(carve, 64), lambda: ops.carve_fields(carve, 64, 8), lambda: ops.carve_scan(block, 64, 128, carve, xyz, [0, 0, 0])):
        with pytest.raises(PointSamHipError):
            call()
    h = torch.arange(8, dtype=torch.int64)
    h[5] = (7 << 32) | 0xfffffffe                                  # words 10, 11
    assert ops.carve_header(h)[ops.CARVE_H_CROSSED] == (7 << 32) | 0xfffffffe


def test_predictor_carve_entries_refuse_before_any_cloud():
    from point_sam_amd.predictor import PointSAMPredictor
    pred = PointSAMPredictor(model=None)
    with pytest.raises(TypeError):
        pred.map_carve("not a map", [0, 0, 0])
    with pytest.raises(TypeError):
        pred.map_carve_frames("not a map", None)
    with pytest.raises(TypeError):
        pred.map_carve_frames(_host_map(), "not frames")


def test_occupied_arithmetic_on_hand_made_counts():
    from point_sam_amd.scanmap import MapOverflow, occupied_from_counts
    hits = torch.tensor([0, 0, 0, 1, 1, 2, 2, 5, 2 ** 31 - 1, 0], dtype=torch.int32)
    misses = torch.tensor([0, 1, 2, 1, 2, 2, 3, 4, 2 ** 31 - 1, 2 ** 31 - 1], dtype=torch.int32)
    assert occupied_from_counts(hits, misses).tolist() == [True, True, False, True, False, True, False, True, True, False]
    assert occupied_from_counts(hits, misses, 1).tolist() == [True, False, False, True, False, True, False, True, True, False]
    assert occupied_from_counts(hits, misses, 0).tolist() == [True, False, False, True, False, True, False, True, True, False], "0 misses never exceed hits * num"
    assert occupied_from_counts(hits, misses, 2, 2, 1).tolist() == [True, True, False, True, True, True, True, True, True, False], "free needs misses > 2 hits"
    assert occupied_from_counts(hits, misses, 2, 1, 2).tolist() == [True, True, False, True, False, False, False, False, False, False], "free needs 2 misses > hits"
    assert occupied_from_counts(hits, misses, 2, 2 ** 31 - 1, 2 ** 31 - 1).tolist()[8] is True, "int64: (2^31 - 1)^2 does not wrap"
    want = CR.occupied(hits.numpy(), misses.numpy(), 2, 3, 2)
    assert occupied_from_counts(hits, misses, 2, 3, 2).numpy().tolist() == want.tolist()
    m = _host_map()
    assert m.num_carves == 0
    m._V = 3                                                       # three voxels, never carved: everything is occupied, without a launch
    assert m.occupied().tolist() == [True] * 3 and m.hits().tolist() == [0] * 3 and m.last_missed().dtype == torch.int32
    for bad in ({"min_misses": -1}, {"min_misses": 1.5}, {"min_misses": True}, {"num": -1}, {"den": 0}, {"den": 2 ** 31}):
        with pytest.raises(ValueError, match="occupied"):
            m.occupied(**bad)
    m._flags = 1                                                   # a dead map
    for call in (m.occupied, m.hits, lambda: m.carve(torch.zeros(4, 3), [0, 0, 0])):
        with pytest.raises(MapOverflow):
            call()


# ------------------------------------------------------------------------------------------------ the demo's routes
class _RefScanMap:
    """scanmap.ScanMap's surface over the references."""

    def __init__(self, voxel_size, max_voxels):
        self.ref = SM.RefMap(voxel_size, max_voxels)
        self.cut = CR.RefCarve(self.ref)

    num_voxels = property(lambda self: self.ref.V)
    num_adds = property(lambda self: self.ref.adds)
    num_carves = property(lambda self: self.cut.carves)

    def cloud(self):
        return tuple(torch.from_numpy(a) for a in self.ref.cloud())

    def labels(self, min_votes=1):
        return tuple(torch.from_numpy(a) for a in self.ref.labels(min_votes))

    def occupied(self, min_misses=2):
        hits, misses, _, _ = self.cut.fields()
        return torch.from_numpy(CR.occupied(hits, misses, min_misses))

    def clear(self):
        self.ref.clear()
        self.cut.clear()


class FakeMapper:
    """tests/test_scanmap_cpu.py's stand-in, with map_carve: map_add takes exactly (m, labels, pose), as the demo calls it today."""

    def __init__(self):
        self.calls = []

    def set_pointcloud(self, xyz, rgb):
        self.xyz, self.rgb = xyz, rgb

    def new_map(self, voxel_size, max_voxels):
        return _RefScanMap(voxel_size, max_voxels)

    def map_add(self, m, labels=None, pose=None):
        from point_sam_amd.scanmap import AddResult
        self.calls.append("add")
        ids, new, acc, rej = m.ref.add(self.xyz[0].numpy(), self.rgb[0].numpy(), None if labels is None else labels.numpy(), pose)
        return AddResult(torch.from_numpy(ids), new, acc, rej)

    def map_carve(self, m, origin, pose=None, margin=1):
        from point_sam_amd.scanmap import CarveResult
        self.calls.append(("carve", tuple(origin), margin))
        return CarveResult(*m.cut.carve(self.xyz[0].numpy(), origin, pose, margin)[:6])


def _req(port, path, body=None):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=20)
    c.request("POST", path, None if body is None else json.dumps(body), {"Content-Type": "application/json"})
    r = c.getresponse()
    return r.status, json.loads(r.read())


def _upload(port, xyz, rgb):
    st, _ = _req(port, "/sampled_pointcloud", {"points": {str(i): float(v) for i, v in enumerate(xyz.flatten())},
                                               "colors": {str(i): float(v) for i, v in enumerate(rgb.flatten())}})
    assert st == 200


def _wall(x, n=6):
    """A wall of n x n points in the plane at x, one per voxel of size 0.25 around the middle."""
    t = (np.arange(n) - n / 2 + 0.5) * 0.25
    y, z = np.meshgrid(t, t, indexing="ij")
    return np.stack([np.full(n * n, x), y.ravel(), z.ravel()], 1).astype(np.float32)


def test_map_routes_carve_and_answer_as_before_without_the_new_keys():
    from point_sam_amd.demo_server import DemoSession, serve
    pred = FakeMapper()
    srv = serve(DemoSession(pred, device="cpu", map_voxel_size=0.25, map_max_voxels=256), "127.0.0.1", 0)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    try:
        port = srv.server_address[1]
        ghost = np.array([[0.1, 0.1, 0.1], [0.1, -0.1, 0.1]], dtype=np.float32)      # two voxels half way to the wall
        wall = _wall(0.8)
        first = np.concatenate([wall, ghost])
        rgb = np.zeros_like(first)
        origin = [-0.9, 0.05, 0.05]
        ref = SM.RefMap(0.25, 256)
        cut = CR.RefCarve(ref)
        _upload(port, first, rgb)
        # without the new keys: exactly the five keys of before, and the predictor sees an add alone
        st, out = _req(port, "/map/add", {})
        want = ref.add(first, rgb, np.full(len(first), -1, dtype=np.int32))
        assert st == 200 and out == {"new_voxels": want[1], "accepted": want[2], "rejected": want[3], "num_voxels": ref.V, "num_adds": 1}
        assert pred.calls == ["add"]
        st, out = _req(port, "/map", {})
        assert st == 200 and set(out) == {"xyz", "rgb", "labels", "votes"}
        # with an origin: the add as before, then the carve, and the carve's counts in the answer
        for scan, margin in ((first, None), (wall, 0), (wall, None)):
            _upload(port, scan, np.zeros_like(scan))
            body = {"origin": origin} if margin is None else {"origin": origin, "margin": margin}
            n = len(pred.calls)
            st, out = _req(port, "/map/add", body)
            want = ref.add(scan, np.zeros_like(scan), np.full(len(scan), -1, dtype=np.int32))
            rays, acc, rej, hit, missed, crossed, _ = cut.carve(scan, origin, None, 1 if margin is None else margin)
            assert st == 200 and pred.calls[n:] == ["add", ("carve", tuple(origin), 1 if margin is None else margin)]
            assert out == {"new_voxels": want[1], "accepted": want[2], "rejected": want[3], "num_voxels": ref.V, "num_adds": ref.adds, "rays": rays,
                           "hit_voxels": hit, "missed_voxels": missed, "crossed": crossed, "num_carves": cut.carves}
            assert rays > 0 and crossed > 0
        hits, misses, _, _ = cut.fields()
        ghost_ids = ref.locate(ghost)
        assert misses[ghost_ids].tolist() == [2, 2] and hits[ghost_ids].tolist() == [1, 1]
        for body, mm in (({"min_misses": 2}, 2), ({"min_misses": 3, "min_votes": 1}, 3), ({"min_misses": 0}, 0)):
            st, out = _req(port, "/map", body)
            occ = CR.occupied(hits, misses, mm)
            assert st == 200 and set(out) == {"xyz", "rgb", "labels", "votes", "occupied"} and out["occupied"] == occ.tolist()
            assert all(isinstance(v, bool) for v in out["occupied"])
        assert not CR.occupied(hits, misses, 2)[ghost_ids].any() and CR.occupied(hits, misses, 2)[ref.locate(wall)].all()
        n = len(pred.calls)
        for bad in ({"origin": [0, 0]}, {"origin": "x"}, {"origin": [0, 0, "z"]}, {"origin": [0, True, 0]}, {"origin": [0, 0, 1e39]}, {"origin": [1.5, 0, 0]},
                    {"origin": origin, "margin": -1}, {"origin": origin, "margin": 1.5}, {"origin": origin, "margin": True}, {"origin": origin, "margin": 1 << 21},
                    {"margin": 1}, {"origin": origin, "other": 1}):
            assert _req(port, "/map/add", bad)[0] == 400, bad
        for bad in ({"min_misses": -1}, {"min_misses": 1.5}, {"min_misses": True}, {"min_misses": "2"}):
            assert _req(port, "/map", bad)[0] == 400, bad
        assert len(pred.calls) == n, "a refused request never reaches the predictor"
        assert _req(port, "/map/clear")[0] == 200
        _upload(port, first, rgb)
        st, out = _req(port, "/map/add", {"origin": origin})
        assert st == 200 and out["num_adds"] == 1 and out["num_carves"] == 1
    finally:
        srv.shutdown()
