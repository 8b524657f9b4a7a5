"""Scan map normals and point-to-plane tracking without a GPU: the numpy reference tests/map_normals_reference.py against itself (the constants of its
loop, the definition form of the step against the vectorised form, hand cases of the normals), the C ABI (header, binding, sizes, refusals before any
launch) and the refusals of the Python layers that come before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import align_plane_reference as AP
import align_reference as AR
import map_normals_reference as MN
import scanmap_reference as SM
import track_reference as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ENTRY_POINTS = ("psam_scanmap_normals", "psam_scanmap_plane_step", "psam_scanmap_plane_workspace_bytes")
BY_NAME = {c["name"]: c for c in TR.cases()}


# ------------------------------------------------------------------------------------------------ the reference
def test_loop_fixture_constants():
    """The table of the change that added the entries: point-to-plane against the map takes a third of the steps of point-to-point and ends a
    tenth as far from the truth."""
    ref, a, b = TR.loop_case()
    nrm, out = MN.loop_reference(ref, b)
    assert ref.V == TR.REF_LOOP_VOXELS and int(nrm["valid"].sum()) == MN.REF_VALID_VOXELS and int((nrm["valid"] & ~nrm["gap"]).sum()) == MN.REF_GAPLESS_VOXELS
    assert out["converged"] and out["reason"] == "tolerance" and out["iterations"] == MN.REF_PLANE_STEPS
    assert tuple(h[0] for h in out["history"]) == MN.REF_PLANE_USED and tuple(out["unused"]) == MN.REF_PLANE_UNUSED
    assert all(u + n == len(b) for u, n in zip(MN.REF_PLANE_USED, MN.REF_PLANE_UNUSED)), "every query is paired at every step"
    rot, tr = AR.pose_error(out["pose"])
    print(f"plane loop: {out['iterations']} steps, rotation error {rot:.4e} rad, translation error {tr:.4e}, rms {out['rms']:.4e}, updates {out['updates'][-1]}")
    assert abs(rot - MN.REF_PLANE_ROTATION_ERROR) < 1e-7 and abs(tr - MN.REF_PLANE_TRANSLATION_ERROR) < 1e-7
    assert 3 * out["iterations"] <= TR.REF_LOOP_ITERATIONS and 9 * rot < TR.REF_ROTATION_ERROR and 9 * tr < TR.REF_TRANSLATION_ERROR
    # the unused pairs of the last step are exactly the queries whose voxel has no normal
    near = MN.step(ref, b, nrm["normal"], TR.LOOP_FINAL, out["pose"].astype(F))[0]
    assert (near >= 0).all() and int((~nrm["valid"][near]).sum()) == MN.REF_PLANE_UNUSED[-1]


@pytest.mark.parametrize("name", ["sizes M=65", "sizes M=257", "full table", "high corner", "boundary", "skip", "min_count 2", "V below the map's", "bits",
                                  "skip hands on", "tie and q == r2"])
def test_vectorised_step_equals_the_definition(name):
    case = BY_NAME[name]
    ref = TR.build(case)
    V = case.get("V") or ref.V
    nrm = MN.normals(ref, 1, 1, V, case.get("skip"), case.get("min_count", 1))["normal"]      # min_voxels 1: many used pairs
    nrm[::7] = 0                                                   # and some that are not
    a, b = MN.reference(case, nrm, ref), MN.reference(case, nrm, ref, definition=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[1][0] + a[1][30] == (a[0] >= 0).sum() and a[1][31] >= a[1][0] + a[1][30]


def test_pairs_are_the_point_to_point_steps():
    case = BY_NAME["sizes M=257"]
    ref = TR.build(case)
    nrm = MN.normals(ref)["normal"]
    near, sums, _ = MN.reference(case, nrm, ref)
    want, point, _ = TR.reference(case, ref)
    assert np.array_equal(near, want) and sums[0] + sums[30] == point[0] and sums[31] == point[19]


def test_hand_cases_of_the_normals():
    h = 2.0 ** -3
    # a 5 x 5 sheet of single-point voxels on one lattice plane z = const: S has no z entry at all, so the normal is exactly (0, 0, 1) and curvature 0
    ij = np.stack(np.meshgrid(np.arange(5), np.arange(5), indexing="ij"), -1).reshape(-1, 2)
    sheet = np.concatenate([(ij + 0.5) * h - 0.25, np.full((25, 1), 0.0625)], 1).astype(F)
    ref = SM.RefMap(h, 64)
    ref.add(sheet, np.zeros_like(sheet))
    n = MN.normals(ref)
    assert ref.V == 25 and n["count"].min() == 4 and n["count"].max() == 9
    ok = n["count"] >= 5
    assert ok.sum() == 21 and (n["normal"][ok] == np.array([0, 0, 1], dtype=F)).all() and (n["curvature"][ok] == 0).all()
    assert (n["normal"][~ok] == 0).all() and (n["curvature"][~ok] == 0).all() and (n["scatter"][:, [2, 4, 5]] == 0).all()
    wide = MN.normals(ref, reach=2)
    assert wide["count"].min() == 9 and wide["count"].max() == 25 and (wide["normal"] == np.array([0, 0, 1], dtype=F)).all()
    # a voxel that is not allowed has count 0 and enters no other voxel's neighbourhood
    skip = np.zeros(25, dtype=bool)
    skip[12] = True                                                # the centre of the sheet
    s = MN.normals(ref, skip=skip)
    assert s["count"][12] == 0 and (s["normal"][12] == 0).all() and (s["scatter"][12] == 0).all()
    centre = ij[12]
    beside = np.abs(ij - centre).max(1) == 1
    assert (s["count"][beside] == n["count"][beside] - 1).all() and (s["count"][~beside & ~skip] == n["count"][~beside & ~skip]).all()
    # min_count: the means of voxels seen twice only
    ref.add(sheet[:10], np.zeros_like(sheet[:10]))
    twice = MN.normals(ref, min_count=2, min_voxels=1)
    assert (twice["count"][10:] == 0).all() and (twice["count"][:10] > 0).all()
    # V below the map's: ids at or above V are no neighbours
    low = MN.normals(ref, V=5, min_voxels=1)
    assert len(low["count"]) == 5 and low["count"].tolist() == [2, 3, 3, 3, 2]
    # the int64 bound of the definition: 125 voxels with q <= 2^21
    assert 125 * 125 * (1 << 42) < 1 << 63


def test_order_of_the_adds_does_not_enter_a_normal():
    case = BY_NAME["sizes M=257"]
    pts = np.concatenate(case["adds"])
    a, b = SM.RefMap(case["h"], 4096), SM.RefMap(case["h"], 4096)
    a.add(pts, np.zeros_like(pts))
    perm = np.random.default_rng(3).permutation(len(pts))
    b.add(pts[perm], np.zeros_like(pts))
    na, nb = MN.normals(a), MN.normals(b)
    assert a.keys != b.keys and sorted(a.keys) == sorted(b.keys)
    at = [b.id_of[k] for k in a.keys]
    assert np.array_equal(na["normal"].view(np.int32), nb["normal"][at].view(np.int32)) and np.array_equal(na["scatter"], nb["scatter"][at])


def test_reference_leaves_out_no_voxel_on_the_named_maps():
    ref = TR.loop_case()[0]
    for name, r in [("loop", ref)] + [(n, TR.build(BY_NAME[n])) for n in ("sizes M=257", "full table", "high corner")]:
        for reach in (1, 2):
            n = MN.normals(r, reach)
            assert int((n["valid"] & ~n["gap"]).sum()) == 0, (name, reach)
    assert not MN.normals(TR.build(BY_NAME["boundary"]), 2)["valid"].any(), "boundary: every voxel below min_voxels"


# ------------------------------------------------------------------------------------------------ the C ABI
def _ctype(decl: str):
    from point_sam_amd import _lib
    decl = decl.strip()
    if "*" in decl or decl.startswith("psam_stream_t"):
        return _lib.ptr
    return {"float": _lib.f32, "int32_t": _lib.i32, "size_t": _lib.size_t}[decl.split()[-2] if len(decl.split()) > 1 else decl]


def test_header_and_binding_declare_the_same_entries():
    from point_sam_amd import _lib, ops
    from point_sam_amd.build import SOURCES
    hdr = open(os.path.join(ROOT, "include", "pointsam_hip.h")).read()
    declared = set(re.findall(r"\b(psam_scanmap_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(ENTRY_POINTS) == {n for n in _lib.SIGNATURES if n.startswith("psam_scanmap_")}
    for n in ENTRY_POINTS:
        ret, params = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % n, hdr).groups()
        assert _lib.SIGNATURES[n] == (_lib.size_t if n.endswith("_bytes") else _lib.i32, [_ctype(p) for p in params.split(",")]), n
        assert ret == ("size_t" if n.endswith("_bytes") else "int32_t")
    assert "scan map normals */" in hdr
    assert int(re.search(r"#define PSAM_SCANMAP_NORMALS_MAX_REACH (\d+)", hdr).group(1)) == ops.MAP_NORMALS_MAX_REACH == 2
    flags = dict(SOURCES)
    assert flags["map_normals.hip"] == flags["scanmap.hip"] == ["-ffp-contract=off", "-fno-slp-vectorize"]
    csrc = os.path.join(ROOT, "point_sam_amd", "csrc")
    shared, a, b = (open(os.path.join(csrc, f)).read() for f in ("normal_eigen.h", "normals.hip", "map_normals.hip"))
    for one in ("void normal_rotate(", "double normal_to_double(", "void normal_solve("):
        assert one in shared and one not in a and one not in b, "one copy of the eigen-solve"
    track = open(os.path.join(csrc, "track.hip")).read()
    assert track.count("map_find_rest(") == 1 and "psam_scanmap_plane_step" in track, "one copy of the pair search: both steps are track.hip's kernel"


def test_sizes_and_refusals_of_the_c_entries_before_any_launch():
    """Nothing is launched: every call is a size query or is refused by the argument checks.  The pointers are addresses inside a host buffer."""
    from point_sam_amd import _lib
    from point_sam_amd.build import build_library
    build_library()
    lib = _lib.load()
    for M in (1, 64, 65, 2113, 1 << 28):
        assert lib.psam_scanmap_plane_workspace_bytes(M) == lib.psam_plane_workspace_bytes(M) == (M + 63) // 64 * 32 * 8
    for bad in (0, -1, (1 << 28) + 1):
        assert lib.psam_scanmap_plane_workspace_bytes(bad) == 0
    host = ctypes.create_string_buffer(1 << 18)
    p = (ctypes.addressof(host) + 15) & ~15
    mv, mp, M = 64, 128, 100
    nbytes, ws_bytes = lib.psam_map_bytes(mv, mp), lib.psam_scanmap_plane_workspace_bytes(M)
    sums, ws, q, nrm = p + (1 << 17), p + (1 << 17) + 256, p + (1 << 16), p + (1 << 16) + 4096
    err = lambda: lib.psam_last_error_string().decode()
    good = dict(map=p, map_bytes=nbytes, mv=mv, mp=mp, V=8, normals=nrm, skip=None, min_count=1, reach=1, r2=0.01, qry=q, M=M, bits=None, pose=None, nearest=None,
                sums=sums, ws=ws, ws_bytes=ws_bytes)
    step = lambda **change: lib.psam_scanmap_plane_step(*dict(good, **change).values(), None)
    for change in (dict(map=None), dict(qry=None), dict(sums=None), dict(ws=None), dict(normals=None), dict(M=0), dict(M=(1 << 28) + 1), dict(V=0),
                   dict(V=mv + 1), dict(mv=0), dict(mp=0), dict(reach=0), dict(reach=5), dict(min_count=0), dict(r2=0.0), dict(r2=float("nan")),
                   dict(r2=float("inf"))):
        assert step(**change) == -1 and err().startswith("psam_scanmap_plane_step"), change
    bad_pose = (ctypes.c_float * 12)(*([1.0] * 11 + [float("nan")]))
    assert step(pose=ctypes.addressof(bad_pose)) == -1 and "pose" in err()
    for change in (dict(map=p + 8), dict(sums=sums + 4), dict(ws=ws + 4), dict(skip=p + 4), dict(bits=p + 4), dict(qry=q + 2), dict(nearest=q + 1),
                   dict(normals=nrm + 2)):
        assert step(**change) == -2 and "aligned" in err(), change
    assert step(map_bytes=nbytes - 1) == -3 and "map block too small" in err()
    assert step(ws_bytes=ws_bytes - 1) == -3 and "psam_scanmap_plane_workspace_bytes" in err()
    assert step(ws_bytes=lib.psam_track_workspace_bytes(M)) == -3, "the point-to-point workspace is too small for thirty-two sums"

    count, scat, normal, curv = p + (1 << 16), p + (1 << 16) + 1024, p + (1 << 16) + 8192, p + (1 << 16) + 12288
    good = dict(map=p, map_bytes=nbytes, mv=mv, mp=mp, V=8, skip=None, min_count=1, reach=1, min_voxels=5, count=count, scatter=scat, normal=normal,
                curvature=curv)
    normals = lambda **change: lib.psam_scanmap_normals(*dict(good, **change).values(), None)
    for change in (dict(map=None), dict(count=None), dict(normal=None), dict(curvature=None), dict(V=0), dict(V=mv + 1), dict(mv=0), dict(mp=0),
                   dict(mv=(1 << 28) + 1), dict(reach=0), dict(reach=3), dict(reach=-1), dict(min_voxels=0), dict(min_voxels=-2), dict(min_count=0)):
        assert normals(**change) == -1 and err().startswith("psam_scanmap_normals"), change
    for change in (dict(map=p + 8), dict(skip=p + 4), dict(scatter=scat + 4), dict(count=count + 2), dict(normal=normal + 1), dict(curvature=curv + 2)):
        assert normals(**change) == -2 and "aligned" in err(), change
    assert normals(map_bytes=nbytes - 1) == -3 and "map block too small" in err()


# ------------------------------------------------------------------------------------------------ the wrappers
def _host_map(voxel_size=0.125, max_voxels=64, V=0):
    """tests/test_carve_cpu.py's: a ScanMap put together by hand over a host block; every call made on it here is refused before it reaches the block."""
    from point_sam_amd import ops
    from point_sam_amd.scanmap import ScanMap
    m = ScanMap.__new__(ScanMap)
    m.voxel_size, (m.max_voxels, m.max_pairs) = voxel_size, ops.map_capacities(max_voxels)
    m._block = torch.zeros(ops.map_bytes(m.max_voxels, m.max_pairs) // 8 + 2, dtype=torch.int64)
    m._adds = m._flags = m._carves = 0
    m._V, m._carve = V, None
    return m


def test_wrappers_refuse_bad_arguments_before_device_work():
    from point_sam_amd import ops
    from point_sam_amd._lib import PointSamHipError
    from point_sam_amd.align import AlignConfig, PlaneConfig
    from point_sam_amd.scanmap import MapOverflow
    xyz, nrm = torch.zeros(100, 3), torch.zeros(8, 3)
    cfg = AlignConfig(radius=0.25, final_radius=0.125, shrink=0.8)
    m = _host_map(V=8)
    # track: the normals and the plane configuration
    for bad in (torch.zeros(7, 3), torch.zeros(8, 3, dtype=torch.float64), torch.zeros(8, 4), torch.zeros(24), "x", 1, False, np.zeros((8, 3), dtype=F)):
        with pytest.raises(ValueError, match="normals"):
            m.track(xyz, cfg, normals=bad)
    with pytest.raises(ValueError, match="needs normals"):
        m.track(xyz, cfg, plane=PlaneConfig())
    with pytest.raises(TypeError, match="PlaneConfig"):
        m.track(xyz, cfg, normals=nrm, plane={"condition": 1e-9})
    with pytest.raises(TypeError, match="occupied"):
        m.track(xyz, cfg, occupied="x", normals=nrm)
    with pytest.raises(ValueError, match="at most 4"):
        m.track(xyz, AlignConfig(radius=0.51), normals=True)
    # empty and dead maps
    dead = _host_map(V=8)
    dead._flags = 1
    for call in (lambda mm: mm.normals(), lambda mm: mm.track_plane_step(xyz, nrm), lambda mm: mm.track(xyz, cfg, normals=True)):
        with pytest.raises(ValueError, match="empty"):
            call(_host_map())
        with pytest.raises(MapOverflow):
            call(dead)
    # normals()
    for bad in ("x", 1, [True] * 8):
        with pytest.raises(TypeError, match="occupied"):
            m.normals(occupied=bad)
    with pytest.raises(ValueError, match="occupied"):
        m.normals(occupied=torch.ones(7, dtype=torch.bool))
    for bad in (0, 3, -1, 1.0, True):
        with pytest.raises(ValueError, match="reach"):
            m.normals(reach=bad)
    for bad in (0, -1, 2.5, True, 2 ** 31):
        with pytest.raises(ValueError, match="min_voxels"):
            m.normals(min_voxels=bad)
        with pytest.raises(ValueError, match="min_count"):
            m.normals(min_count=bad)
    block, mv, mp = m._block, m.max_voxels, m.max_pairs
    for skip in (torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), [0]):
        with pytest.raises(ValueError, match="skip"):
            ops.map_normals(block, mv, mp, 8, skip=skip)
    for V in (0, 65, 2.0, True):
        with pytest.raises(ValueError):
            ops.map_normals(block, mv, mp, V)
    with pytest.raises(TypeError):
        ops.map_normals("x", mv, mp, 8)
    with pytest.raises(ValueError):
        ops.map_normals(block, 4096, 8192, 8)                      # the block is too short for that map
    with pytest.raises(PointSamHipError):
        ops.map_normals(block, mv, mp, 8)                          # everything in order, but the block lives on the CPU: no CPU fallback
    # track_plane_step: track_step's checks, and the normals
    step = lambda *a, **k: ops.track_plane_step(block, mv, mp, 8, *a, voxel_size=0.125, **k)
    for bad in (torch.zeros(7, 3), torch.zeros(8, 3, dtype=torch.float64), torch.zeros(8, 2), "x", None):
        with pytest.raises(ValueError, match="normals"):
            step(xyz, bad)
    with pytest.raises(TypeError):
        step(xyz.double(), nrm)
    for bad in (torch.zeros(0, 3), torch.zeros(10, 2)):
        with pytest.raises(ValueError):
            step(bad, nrm)
    for pose in (np.eye(3), np.full((3, 4), np.nan), "x"):
        with pytest.raises(ValueError):
            step(xyz, nrm, pose)
    for radius in (0.0, -1.0, float("nan"), "r", 0.51):
        with pytest.raises(ValueError):
            step(xyz, nrm, None, radius)
    with pytest.raises(ValueError, match="bits"):
        step(xyz, nrm, bits=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="skip"):
        step(xyz, nrm, skip=torch.zeros(2, dtype=torch.int64))
    for n in (0, -1, 1.0, True, 2 ** 31):
        with pytest.raises(ValueError, match="min_count"):
            step(xyz, nrm, min_count=n)
    with pytest.raises(PointSamHipError):
        step(xyz, nrm)


def test_predictor_passes_normals_and_plane_through():
    import inspect
    from point_sam_amd.predictor import PointSAMPredictor
    from point_sam_amd.scanmap import ScanMap
    a, b = inspect.signature(PointSAMPredictor.map_align).parameters, inspect.signature(ScanMap.track).parameters
    for name in ("normals", "plane"):
        assert a[name].default is None and b[name].default is None
    assert list(b)[-2:] == ["normals", "plane"] and list(a)[-2:] == ["normals", "plane"]
