"""Scan map normals and point-to-plane tracking on the GPU (csrc/map_normals.hip, csrc/track.hip; ops.map_normals / track_plane_step, ScanMap.normals /
track_plane_step / track(normals=...), predictor.map_align(normals=...)) against the plain numpy reference tests/map_normals_reference.py.  Counts
and scatter matrices are exact; normals are held to numpy.linalg.eigh of the exact scatter under tests/test_gpu_superpoints.py's budget; `nearest`
and the three counts of a step are exact, its other sums exact on the lattice case and otherwise within M * 2^-53 * sum |term| of the exactly rounded
value, the bound tests/test_gpu_track.py uses.  Every call goes through the C entry with its outputs between guard words, and the map's block is compared
bit for bit before and after: both entries only read it."""
import ctypes

import numpy as np
import pytest
import torch

import align_plane_reference as AP
import align_reference as AR
import map_normals_reference as MN
import scanmap_reference as SM
import track_reference as TR
from point_sam_amd.config import get_config
from point_sam_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu
f32 = np.float32
U = 2.0 ** -53
GUARD_WORDS = 512
GUARD = -7.25                # the sentinel of every floating-point output and guard: no output of a case takes this value
IGUARD = -99                 # the same for int32 outputs
CASES = TR.cases()
BY_NAME = {c["name"]: c for c in CASES}


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
    """-> (ScanMap on the device, RefMap): the case's adds in order; the ids of every add agree (tests/test_gpu_track.py's)."""
    from point_sam_amd.scanmap import ScanMap
    m, ref = ScanMap(case["h"], case["max_voxels"]), SM.RefMap(case["h"], case["max_voxels"])
    for pts in case["adds"]:
        got = m.add(_dev(pts), _dev(np.zeros_like(pts)))
        assert np.array_equal(got.ids.cpu().numpy(), ref.add(pts, np.zeros_like(pts))[0])
    assert m.num_voxels == ref.V
    return m, ref


_maps = {}


def _shared_map(case):
    """One device map per distinct list of adds: no call of this file changes it."""
    key = (case["h"], case["max_voxels"]) + tuple(a.tobytes() for a in case["adds"])
    if key not in _maps:
        _maps[key] = _device_map(case)
    return _maps[key]


# ------------------------------------------------------------------------------------------------ the maps of the normals
def _surface(n):
    """n single-point voxels on a wavy sheet: cells (i, j) of a 16 x 17 grid at h = 2^-4, the first n of them."""
    g = np.random.default_rng(n)
    ij = np.stack(np.meshgrid(np.arange(16), np.arange(17), indexing="ij"), -1).reshape(-1, 2)[:n]
    xy = (ij + g.uniform(0.1, 0.9, size=ij.shape)) * 2.0 ** -4 - 0.5
    return np.concatenate([xy, 0.08 * np.sin(6 * xy[:, :1]) * np.cos(5 * xy[:, 1:])], 1).astype(f32)


def _sheet():
    """tests/test_map_normals_cpu.py's: a 5 x 5 sheet of single-point voxels on one lattice plane."""
    ij = np.stack(np.meshgrid(np.arange(5), np.arange(5), indexing="ij"), -1).reshape(-1, 2)
    return np.concatenate([(ij + 0.5) * 2.0 ** -3 - 0.25, np.full((25, 1), 0.0625)], 1).astype(f32)


def _map_cases():
    out = {"loop": dict(h=TR.LOOP_H, max_voxels=TR.LOOP_MAX_VOXELS, adds=[TR.loop_case()[1]])}
    for name in ("sizes M=257", "full table", "high corner", "boundary"):
        out[name] = BY_NAME[name]
    out["one voxel"] = dict(h=2.0 ** -3, max_voxels=8, adds=[np.array([[0.3, -0.2, 0.1]], dtype=f32)])
    for n in (255, 256, 257):                                      # the last block of 256 threads: full less one, full, one over
        out[f"{n} voxels"] = dict(h=2.0 ** -4, max_voxels=512, adds=[_surface(n)])
    out["sheet"] = dict(h=2.0 ** -3, max_voxels=64, adds=[_sheet()])
    return out


MAPS = _map_cases()
SKIP = np.zeros(1216, dtype=bool)
SKIP[::3] = True
VARIANTS = {"": {}, "skip": dict(skip=SKIP), "min_count 2": dict(min_count=2), "V below the map's": dict(V=700), "min_voxels 9": dict(min_voxels=9)}
NORMAL_CASES = [(name, reach, "") for name in MAPS for reach in (1, 2)] + [("sizes M=257", reach, v) for v in list(VARIANTS)[1:] for reach in (1, 2)]
NO_VOXEL_LEFT_OUT = ("loop", "sizes M=257", "full table", "high corner")      # a CPU run of the reference (tests/test_map_normals_cpu.py)
_references = {}


def _reference(name, reach, variant=""):
    """Computed once and shared; nothing writes into it."""
    key = (name, reach, variant)
    if key not in _references:
        kw = dict(VARIANTS[variant])
        _references[key] = MN.normals(_shared_map(MAPS[name])[1], reach, kw.pop("min_voxels", 5), **kw)
        for a in _references[key].values():
            a.setflags(write=False)
    return _references[key]


def _raw_normals(m, reach=1, min_voxels=5, V=None, skip=None, min_count=1, scatter=True):
    """psam_scanmap_normals itself: every output lies between guard words that stay intact, and the map's block is bit for bit what it was.
    -> (count [V] int32, scatter [V, 6] f64 or None, normal [V, 3] f32, curvature [V] f32)."""
    from point_sam_amd import _lib
    lib = _lib.load()
    V = m.num_voxels if V is None else V
    G = GUARD_WORDS
    count = torch.full((V + 2 * G,), IGUARD, dtype=torch.int32, device="cuda")
    normal = torch.full((3 * V + 2 * G,), GUARD, dtype=torch.float32, device="cuda")
    curv = torch.full((V + 2 * G,), GUARD, dtype=torch.float32, device="cuda")
    scat = torch.full((6 * V + 2 * G,), GUARD, dtype=torch.float64, device="cuda") if scatter else None
    skipw = None if skip is None else _dev(_pack(np.asarray(skip, dtype=bool)[:V], garbage=False))
    before = m._block.clone()
    st = lib.psam_scanmap_normals(m._block.data_ptr(), m._block.numel() * 8, m.max_voxels, m.max_pairs, V, None if skipw is None else skipw.data_ptr(), min_count,
                                  reach, min_voxels, count[G:].data_ptr(), None if scat is None else scat[G:].data_ptr(), normal[G:].data_ptr(),
                                  curv[G:].data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert st == 0, lib.psam_last_error_string()
    torch.cuda.synchronize()
    assert torch.equal(m._block, before), "the map block is only read"
    out = []
    for t, width, guard in ((count, 1, IGUARD), (scat, 6, GUARD), (normal, 3, GUARD), (curv, 1, GUARD)):
        if t is None:
            out.append(None)
            continue
        h = t.cpu().numpy()
        assert (h[:G] == guard).all() and (h[G + width * V:] == guard).all(), "a guard word around an output was written"
        out.append(h[G:G + width * V].reshape((V, width) if width > 1 else (V,)).copy())
    return tuple(out)


# ------------------------------------------------------------------------------------------------ 1. the normals
@pytest.mark.parametrize("name,reach,variant", NORMAL_CASES, ids=lambda v: str(v))
def test_normals_equal_the_reference(ops, name, reach, variant):
    """Counts and the fp64 words of float(S): exact.  On voxels with n >= min_voxels and an eigenvalue gap l1 - l0 >= 1e-4 l2: |n_dev x n_ref| <= 1e-7,
    | |n| - 1 | <= 1e-7 and |curvature - ref| <= 1e-7, the reference (numpy.linalg.eigh of the exact scatter) in fp64 -- tests/test_gpu_superpoints.py's
    budget, for its reasons: fp32 rounding of a unit vector is at most sqrt(3) 2^-25 = 5.2e-8, the fp64 solver's share is below 1e-9 under the gap
    condition; the curvature is at most 1/3, its fp32 rounding 1.5e-8.  Voxels without the gap may be left out, up to 1 % of the valid ones.  Below
    min_voxels and for a voxel that is not allowed: exact zeros."""
    m, ref = _shared_map(MAPS[name])
    want = _reference(name, reach, variant)
    kw = dict(VARIANTS[variant])
    min_voxels = kw.pop("min_voxels", 5)
    dc, ds, dn, dk = _raw_normals(m, reach, min_voxels, **kw)
    V = kw.get("V", ref.V)
    assert dc.shape == (V,) and np.array_equal(dc, want["count"]), np.nonzero(dc != want["count"])[0][:5]
    assert np.array_equal(ds.view(np.int64), want["scatter"].view(np.int64)), "float(S), bit for bit"
    valid, ok = want["valid"], want["gap"]
    assert not dn[~valid].any() and not dk[~valid].any(), "no normal below min_voxels"
    assert not np.signbit(dn[~valid]).any() and not np.signbit(dk[~valid]).any(), "exact zeros"
    if variant in ("skip", "min_count 2"):
        off = ~MN.allowed(ref, V, kw.get("skip"), kw.get("min_count", 1))[:V]
        assert off.sum() > 100 and not dc[off].any() and not ds[off].any() and not dn[off].any(), "a voxel that is not allowed"
    left_out = int(valid.sum() - ok.sum())
    print(f"{name} reach {reach} {variant}: {int(valid.sum())} valid voxels of {V}, counts {dc.min()} .. {dc.max()}, {left_out} without the eigenvalue gap")
    assert left_out <= 0.01 * valid.sum()
    if name in NO_VOXEL_LEFT_OUT and not variant:
        assert left_out == 0
    if name == "boundary":
        assert not valid.any(), "every voxel below min_voxels"
    if name == "one voxel":
        assert dc.tolist() == [1] and not ds.any()
    if name == "full table":
        assert m.num_voxels == 32 == m.max_voxels
    if name == "sizes M=257":
        assert int(m.counts().max()) > 1
    if name == "sheet":
        assert valid.sum() == (21 if reach == 1 else 25)
        assert (dn[valid] == np.array([0, 0, 1], dtype=f32)).all() and (dk[valid] == 0).all(), "means on one lattice plane"
    if not ok.any():
        return
    a, b = dn[ok].astype(np.float64), want["vector"][ok]
    cross = np.linalg.norm(np.cross(a, b), axis=1)
    length = np.abs(np.linalg.norm(a, axis=1) - 1)
    dcurv = np.abs(dk[ok].astype(np.float64) - want["curvature64"][ok])
    print(f"{name} reach {reach} {variant}: worst |n x n_ref| {cross.max():.3e}, worst | |n| - 1 | {length.max():.3e}, worst curvature difference {dcurv.max():.3e}")
    assert cross.max() <= 1e-7 and length.max() <= 1e-7 and dcurv.max() <= 1e-7
    # the sign rule, on the stored fp32 values themselves: the component of largest magnitude is positive, on a tie the lowest axis decides
    mag = np.abs(dn[valid])
    lead = np.where((mag[:, 0] >= mag[:, 1]) & (mag[:, 0] >= mag[:, 2]), 0, np.where(mag[:, 1] >= mag[:, 2], 1, 2))
    assert (dn[valid][np.arange(len(lead)), lead] > 0).all()


def test_two_calls_give_the_same_bytes_and_scatter_is_optional(ops):
    m, _ = _shared_map(MAPS["sizes M=257"])
    runs = [_raw_normals(m, 2), _raw_normals(m, 2), _raw_normals(m, 2, scatter=False)]
    for other in runs[1:]:
        assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip((runs[0][0], runs[0][2], runs[0][3]), (other[0], other[2], other[3])))
    assert np.array_equal(runs[0][1], runs[1][1]) and runs[2][1] is None


def test_the_order_of_the_points_does_not_enter_a_normal(ops):
    """The same points in another order: other ids, the same normal per voxel KEY."""
    from point_sam_amd.scanmap import ScanMap
    case = MAPS["sizes M=257"]
    m, _ = _shared_map(case)
    pts = np.concatenate(case["adds"])
    perm = np.random.default_rng(3).permutation(len(pts))
    other = ScanMap(case["h"], case["max_voxels"])
    for part in (pts[perm][:900], pts[perm][900:]):
        other.add(_dev(part), _dev(np.zeros_like(part)))
    ka, kb = m.keys().cpu().numpy(), other.keys().cpu().numpy()
    assert not np.array_equal(ka, kb) and np.array_equal(np.sort(ka), np.sort(kb))
    at = np.argsort(kb)[np.searchsorted(np.sort(kb), ka)]
    for reach in (1, 2):
        a, b = _raw_normals(m, reach), _raw_normals(other, reach)
        for x, y in zip(a, b):
            assert np.array_equal(x, y[at])


# ------------------------------------------------------------------------------------------------ 2. the plane step
def _raw_step(m, qry, r2, reach, pose=None, take=None, V=None, skip=None, min_count=1, nearest=True, garbage=True, normals=None):
    """psam_scanmap_plane_step (normals [V, 3] f32 on the device) or, without normals, psam_track_step: `sums` and the workspace lie between guard words
    that stay intact, and the map's block is bit for bit what it was.  -> (nearest [M] int32 or None, sums [32] or [20])."""
    from point_sam_amd import _lib, ops
    lib = _lib.load()
    q = _dev(np.ascontiguousarray(qry, dtype=f32))
    M = len(qry)
    V = m.num_voxels if V is None else V
    W = 20 if normals is None else 32
    n_ws = (lib.psam_track_workspace_bytes if normals is None else lib.psam_scanmap_plane_workspace_bytes)(M) // 8
    assert n_ws == -(-M // 64) * W
    buf = torch.full((3 * GUARD_WORDS + W + n_ws,), GUARD, dtype=torch.float64, device="cuda")
    sums = buf[GUARD_WORDS:GUARD_WORDS + W]
    ws = buf[2 * GUARD_WORDS + W:2 * GUARD_WORDS + W + n_ws]
    near = torch.full((M + 2 * GUARD_WORDS,), IGUARD, dtype=torch.int32, device="cuda") if nearest else None
    bits = None if take is None else _dev(_pack(take, garbage))
    skipw = None if skip is None else _dev(_pack(np.asarray(skip, dtype=bool)[:V], garbage=False))
    words = ops.transfer_pose(pose)
    P = None if words is None else (ctypes.c_float * 12)(*[float(w) for w in words])
    before = m._block.clone()
    lead = (m._block.data_ptr(), m._block.numel() * 8, m.max_voxels, m.max_pairs, V)
    rest = (None if skipw is None else skipw.data_ptr(), min_count, reach, float(r2), q.data_ptr(), M, None if bits is None else bits.data_ptr(),
            None if P is None else ctypes.addressof(P), None if near is None else near[GUARD_WORDS:].data_ptr(), sums.data_ptr(), ws.data_ptr(), n_ws * 8,
            torch.cuda.current_stream().cuda_stream)
    if normals is None:
        st = lib.psam_track_step(*lead, *rest)
    else:
        assert normals.dtype == torch.float32 and tuple(normals.shape) == (V, 3) and normals.is_contiguous()
        st = lib.psam_scanmap_plane_step(*lead, normals.data_ptr(), *rest)
    assert st == 0, lib.psam_last_error_string()
    torch.cuda.synchronize()
    assert torch.equal(m._block, before), "the map block is only read"
    host = buf.cpu().numpy()
    guards = np.concatenate([host[:GUARD_WORDS], host[GUARD_WORDS + W:2 * GUARD_WORDS + W], host[2 * GUARD_WORDS + W + n_ws:]])
    assert (guards == GUARD).all(), "a guard word around sums or the workspace was written"
    if near is not None:
        n = near.cpu().numpy()
        assert (n[:GUARD_WORDS] == IGUARD).all() and (n[GUARD_WORDS + M:] == IGUARD).all()
        near = n[GUARD_WORDS:GUARD_WORDS + M]
    return near, host[GUARD_WORDS:GUARD_WORDS + W].copy()


def _fed_normals(m, V, spoil=True):
    """The normals a step of the tests is fed: the device's own (reach 2, so that sparse maps have some), and with `spoil` rows of zeros, rows with a
    NaN and rows with an infinity among them.  -> [V, 3] f32 on the host."""
    n = _raw_normals(m, 2, 3, V, scatter=False)[2]
    if spoil:
        n[::11] = 0
        n[5::13, 1] = np.nan
        n[7::17, 2] = np.inf
        n[3::19, 0] = -np.inf
    return n


def _check_case(case, nrm=None, exact=False):
    """The device's plane step equals the reference's, and its `nearest` is psam_track_step's -> (nearest, sums) of the reference."""
    m, ref = _shared_map(case)
    V = case.get("V") or ref.V
    nrm = _fed_normals(m, V) if nrm is None else nrm
    want_near, want, mass = MN.reference(case, nrm, ref)
    radius = case.get("radius", case["h"])
    reach = case.get("reach") or TR.reach_of(radius, case["h"])
    args = (m, case["qry"], TR.r2_of(radius), reach, case.get("pose"), case.get("take"), case.get("V"), case.get("skip"), case.get("min_count", 1))
    near, got = _raw_step(*args, normals=_dev(nrm))
    point_near, point = _raw_step(*args)
    assert np.array_equal(near, point_near), "the pair is psam_track_step's"
    bad = np.nonzero(near != want_near)[0]
    assert len(bad) == 0, (len(bad), bad[:5], near[bad[:5]], want_near[bad[:5]])
    paired = want_near >= 0
    used = np.zeros(len(paired), dtype=bool)
    used[paired] = AP.used_normals(nrm)[want_near[paired]]
    assert got[0] == want[0] == used.sum() and got[30] == want[30] == (paired & ~used).sum() and got[31] == want[31] == point[19], (got[[0, 30, 31]], want[[0, 30, 31]])
    assert got[0] + got[30] == point[0]
    err = np.abs(got - want)
    bound = np.zeros(32) if exact else len(case["qry"]) * U * mass
    print(f"{case['name']}: M = {len(case['qry'])}, V = {ref.V}, reach {reach}: used {int(got[0])}, unused {int(got[30])}, with a cell {int(got[31])}, "
          f"max |error| / bound = {'exact' if exact else float(np.max(err[1:30] / np.maximum(bound[1:30], 1e-300)))}")
    assert np.isfinite(got).all() and (err <= bound).all(), (np.nonzero(err > bound)[0], got, want, bound)
    return want_near, want


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_plane_step_equals_the_reference(ops, case):
    near, sums = _check_case(case)
    if case["name"] == "sizes M=2113":
        assert sums[0] > 500 and sums[30] > 50, "used and unused pairs, in 34 waves"
    if case["name"] == "skip hands on":
        assert near.tolist() == [-1, 2] and sums[0] + sums[30] == 1 and sums[31] == 2


@pytest.mark.parametrize("kind", ["device", "zeros", "nan", "inf", "tiny"])
def test_the_used_pair_rule_on_normals_fed_by_the_test(ops, kind):
    """A pair is used iff nn, in fp32, is finite and > 0: all-zero rows use nothing, one NaN or infinity unuses a row, a normal whose square
    underflows to zero in fp32 is not used either, and unnormalised normals are taken as given."""
    case = BY_NAME["sizes M=257"]
    m, ref = _shared_map(case)
    nrm = _fed_normals(m, ref.V, spoil=False)
    if kind == "zeros":
        nrm[:] = 0
    elif kind == "nan":
        nrm[::2, 0] = np.nan
    elif kind == "inf":
        nrm[::2] = np.inf
        nrm[1::4] *= 3.5                                          # not normalised: taken as given
    elif kind == "tiny":
        nrm[::2] = f32(1e-23)                                      # nn = 3e-46 rounds to zero in fp32
        nrm[1::2] *= f32(2.0 ** -40)                               # nn = 2^-80: small, positive, used
    near, sums = _check_case(case, nrm)
    if kind == "zeros":
        assert not sums[:30].any() and sums[30] == (near >= 0).sum() > 100
    if kind in ("nan", "inf", "tiny"):
        assert sums[0] > 30 and sums[30] > 30


def test_lattice_case_is_exact(ops):
    case = TR.lattice_case()
    _, ref = _shared_map(case)
    near, sums = _check_case(case, AP.axis_normals(ref.V, 5, zeros=0.2), exact=True)
    assert sums[0] > 200 and sums[30] > 40 and (near < 0).sum() > 100 and sums[31] == 700


def test_a_wider_cube_with_the_same_r2_gives_the_same_words(ops):
    case = BY_NAME["reach 1"]
    m, ref = _shared_map(case)
    nrm = _dev(_fed_normals(m, ref.V))
    runs = [_raw_step(m, case["qry"], TR.r2_of(case["h"]), reach, case["pose"], normals=nrm) for reach in (1, 2, 4)]
    for near, sums in runs[1:]:
        assert np.array_equal(near, runs[0][0]) and np.array_equal(sums.view(np.int64), runs[0][1].view(np.int64))


def test_two_calls_and_no_nearest_give_the_same_words(ops):
    case = BY_NAME["sizes M=2113"]
    m, ref = _shared_map(case)
    nrm, r2 = _dev(_fed_normals(m, ref.V)), TR.r2_of(case["h"])
    runs = [_raw_step(m, case["qry"], r2, 1, case["pose"], nearest=n, normals=nrm)[1].view(np.int64) for n in (True, True, False)]
    runs.append(_raw_step(m, case["qry"], r2, 1, case["pose"], take=np.ones(2113, dtype=bool), normals=nrm)[1].view(np.int64))
    for other in runs[1:]:
        assert np.array_equal(runs[0], other)


# ------------------------------------------------------------------------------------------------ 3. the wrappers
def test_wrappers_give_the_entrys_words(ops):
    from point_sam_amd.scanmap import MapNormals
    case = BY_NAME["skip"]
    m, ref = _shared_map(case)
    skip_host = case["skip"][:ref.V]
    skip = _dev(_pack(skip_host, garbage=False))
    # normals
    raw = _raw_normals(m, 2, 4, None, skip_host, 2)
    count, normal, curvature, scatter = ops.map_normals(m._block, m.max_voxels, m.max_pairs, ref.V, 2, 4, skip, 2, scatter=True)
    assert count.dtype == torch.int32 and normal.shape == (ref.V, 3) and curvature.dtype == torch.float32 and scatter.shape == (ref.V, 6)
    for got, want in zip((count, scatter, normal, curvature), raw):
        assert np.array_equal(got.cpu().numpy(), want)
    assert len(ops.map_normals(m._block, m.max_voxels, m.max_pairs, ref.V)) == 3
    occupied = _dev(~skip_host)
    mine = m.normals(2, 4, occupied, 2)
    assert isinstance(mine, MapNormals) and torch.equal(mine.normal, normal) and torch.equal(mine.curvature, curvature) and torch.equal(mine.count, count)
    default = m.normals()
    for got, want in zip((default.count, default.normal, default.curvature), (lambda r: (r[0], r[2], r[3]))(_raw_normals(m, 1, 5))):
        assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(m.normals(occupied=True).normal, default.normal), "never carved: everything is occupied"
    # the step
    take = np.random.default_rng(5).uniform(size=300) < 0.7
    nrm = _dev(_fed_normals(m, ref.V))
    want = _raw_step(m, case["qry"], TR.r2_of(2 * case["h"]), 2, case["pose"], take, None, skip_host, 2, normals=nrm)
    sums, near = m.track_plane_step(_dev(case["qry"]), nrm, case["pose"], 2 * case["h"], _dev(_pack(take)), skip, 2, return_nearest=True)
    assert sums.dtype == torch.float64 and sums.shape == (32,) and near.dtype == torch.int32 and near.shape == (300,)
    assert np.array_equal(near.cpu().numpy(), want[0]) and np.array_equal(sums.cpu().numpy().view(np.int64), want[1].view(np.int64))
    alone = ops.track_plane_step(m._block, m.max_voxels, m.max_pairs, ref.V, _dev(case["qry"]), nrm, case["pose"], 2 * case["h"], _dev(_pack(take)), skip, 2,
                                 voxel_size=case["h"])
    assert torch.equal(alone, sums)
    default = m.track_plane_step(_dev(case["qry"]), nrm)        # radius None: the voxel size
    assert np.array_equal(default.cpu().numpy().view(np.int64), _raw_step(m, case["qry"], TR.r2_of(case["h"]), 1, normals=nrm)[1].view(np.int64))
    with pytest.raises(ValueError, match="at most 4"):
        m.track_plane_step(_dev(case["qry"]), nrm, None, 4.5 * case["h"])
    with pytest.raises(ValueError, match="normals"):
        m.track_plane_step(_dev(case["qry"]), nrm[:-1])


def test_a_dead_map_and_an_empty_map_raise(ops):
    from point_sam_amd.align import AlignConfig
    from point_sam_amd.scanmap import MapOverflow, ScanMap
    q, nrm = _dev(np.zeros((10, 3), dtype=f32)), _dev(np.zeros((4, 3), dtype=f32))
    cfg = AlignConfig(radius=0.25)
    m = ScanMap(0.125, 4)
    calls = (lambda: m.normals(), lambda: m.track_plane_step(q, nrm), lambda: m.track(q, cfg, normals=True), lambda: m.track(q, cfg, normals=nrm))
    for call in calls:
        with pytest.raises(ValueError, match="empty"):
            call()
    pts = np.random.default_rng(0).uniform(-0.9, 0.9, (50, 3)).astype(f32)
    with pytest.raises(MapOverflow):
        m.add(_dev(pts), _dev(np.zeros_like(pts)))
    for call in calls:
        with pytest.raises(MapOverflow):
            call()


def test_entry_refusals_leave_every_output_untouched(ops):
    from point_sam_amd import _lib
    lib = _lib.load()
    case = TR.lattice_case()
    m, ref = _shared_map(case)
    q = _dev(case["qry"])
    M, V = len(case["qry"]), ref.V
    host_nrm = AP.axis_normals(V, 5, zeros=0.2)
    nrm = _dev(host_nrm)
    sums = torch.full((32,), GUARD, dtype=torch.float64, device="cuda")
    near = torch.full((M,), IGUARD, dtype=torch.int32, device="cuda")
    ws = torch.zeros(lib.psam_scanmap_plane_workspace_bytes(M) // 8, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    block = dict(map=m._block.data_ptr(), map_bytes=m._block.numel() * 8, max_voxels=m.max_voxels, max_pairs=m.max_pairs, V=V)
    good = dict(block, normals=nrm.data_ptr(), skip=None, min_count=1, reach=1, r2=float(TR.r2_of(case["h"])), qry=q.data_ptr(), M=M, qry_bits=None, pose=None,
                nearest=near.data_ptr(), sums=sums.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel() * 8)
    call = lambda **kw: lib.psam_scanmap_plane_step(*{**good, **kw}.values(), stream)
    nan_pose = (ctypes.c_float * 12)(*([1.0] * 11 + [float("nan")]))
    short = lib.psam_map_bytes(m.max_voxels, m.max_pairs) - 1
    for code, kw in ((-1, dict(map=None)), (-1, dict(normals=None)), (-1, dict(qry=None)), (-1, dict(sums=None)), (-1, dict(ws=None)), (-1, dict(M=0)),
                     (-1, dict(V=m.max_voxels + 1)), (-1, dict(V=0)), (-1, dict(max_pairs=0)), (-1, dict(max_voxels=0)), (-1, dict(reach=5)), (-1, dict(reach=0)),
                     (-1, dict(min_count=0)), (-1, dict(r2=float("nan"))), (-1, dict(pose=ctypes.addressof(nan_pose))),
                     (-2, dict(map=m._block.data_ptr() + 8)), (-2, dict(sums=sums.data_ptr() + 4)), (-2, dict(ws=ws.data_ptr() + 4)),
                     (-2, dict(skip=ws.data_ptr() + 4)), (-2, dict(qry_bits=ws.data_ptr() + 4)), (-2, dict(qry=q.data_ptr() + 2)),
                     (-2, dict(nearest=near.data_ptr() + 1)), (-2, dict(normals=nrm.data_ptr() + 2)),
                     (-3, dict(ws_bytes=ws.numel() * 8 - 1)), (-3, dict(map_bytes=short))):
        assert call(**kw) == code, (kw, lib.psam_last_error_string())
        assert lib.psam_last_error_string().decode().startswith("psam_scanmap_plane_step")
    torch.cuda.synchronize()
    assert bool((sums == GUARD).all()) and bool((near == IGUARD).all())
    assert call() == 0
    want_near, want, _ = MN.reference(case, host_nrm, ref)
    assert np.array_equal(sums.cpu().numpy(), want) and np.array_equal(near.cpu().numpy(), want_near)

    count = torch.full((V,), IGUARD, dtype=torch.int32, device="cuda")
    scat = torch.full((V, 6), GUARD, dtype=torch.float64, device="cuda")
    normal = torch.full((V, 3), GUARD, dtype=torch.float32, device="cuda")
    curv = torch.full((V,), GUARD, dtype=torch.float32, device="cuda")
    good = dict(block, skip=None, min_count=1, reach=1, min_voxels=5, count=count.data_ptr(), scatter=scat.data_ptr(), normal=normal.data_ptr(),
                curvature=curv.data_ptr())
    call = lambda **kw: lib.psam_scanmap_normals(*{**good, **kw}.values(), stream)
    for code, kw in ((-1, dict(map=None)), (-1, dict(count=None)), (-1, dict(normal=None)), (-1, dict(curvature=None)), (-1, dict(V=0)),
                     (-1, dict(V=m.max_voxels + 1)), (-1, dict(max_voxels=0)), (-1, dict(max_pairs=0)), (-1, dict(reach=0)), (-1, dict(reach=3)),
                     (-1, dict(min_voxels=0)), (-1, dict(min_count=0)),
                     (-2, dict(map=m._block.data_ptr() + 8)), (-2, dict(skip=ws.data_ptr() + 4)), (-2, dict(scatter=scat.data_ptr() + 4)),
                     (-2, dict(count=count.data_ptr() + 2)), (-2, dict(normal=normal.data_ptr() + 1)), (-2, dict(curvature=curv.data_ptr() + 2)),
                     (-3, dict(map_bytes=short))):
        assert call(**kw) == code, (kw, lib.psam_last_error_string())
        assert lib.psam_last_error_string().decode().startswith("psam_scanmap_normals")
    torch.cuda.synchronize()
    assert bool((count == IGUARD).all()) and bool((scat == GUARD).all()) and bool((normal == GUARD).all()) and bool((curv == GUARD).all())
    assert call() == 0
    want = MN.normals(ref)
    assert np.array_equal(count.cpu().numpy(), want["count"]) and np.array_equal(scat.cpu().numpy(), want["scatter"])


# ------------------------------------------------------------------------------------------------ 4. the loop, on the fixture tests/test_map_normals_cpu.py verifies
ROTATION_MARGIN = max(10 * MN.REF_PLANE_ROTATION_ERROR, 1e-6)      # ten times the reference plane loop's recorded error against the truth: 6.7592e-3 rad
TRANSLATION_MARGIN = max(10 * MN.REF_PLANE_TRANSLATION_ERROR, 1e-6)      # 1.5397e-3


def _same_alignment(a, b):
    return (np.array_equal(a.pose.view(np.int64), b.pose.view(np.int64)) and (a.pairs, a.coverage, a.rms, a.iterations, a.converged, a.reason) ==
            (b.pairs, b.coverage, b.rms, b.iterations, b.converged, b.reason) and a.history == b.history)


@pytest.fixture(scope="module")
def loop(ops):
    m, ref = _shared_map(MAPS["loop"])
    assert m.num_voxels == ref.V == TR.REF_LOOP_VOXELS
    b = TR.loop_case()[2]
    return m, ref, _dev(b), b


def _config():
    from point_sam_amd.align import AlignConfig
    return AlignConfig(radius=TR.LOOP_RADIUS, final_radius=TR.LOOP_FINAL, shrink=TR.LOOP_SHRINK)


def test_plane_track_on_the_device_converges_faster_and_nearer_than_point_to_point(ops, loop):
    from point_sam_amd.align import PlaneConfig
    m, ref, qry, b = loop
    before = m._block.clone()
    out = m.track(qry, _config(), TR.LOOP_INIT, normals=True)
    rot, tr = AR.pose_error(out.pose)
    print(f"device plane track: {out.iterations} steps (reference {MN.REF_PLANE_STEPS}, point to point {TR.REF_LOOP_ITERATIONS}), {out.pairs} used pairs, coverage "
          f"{out.coverage:.4f}, rms {out.rms:.6f}, rotation error {rot:.4e} rad (margin {ROTATION_MARGIN:.4e}, point to point {TR.REF_ROTATION_ERROR:.4e}), "
          f"translation error {tr:.4e} (margin {TRANSLATION_MARGIN:.4e}, point to point {TR.REF_TRANSLATION_ERROR:.4e}), {out.reason}")
    assert out.converged and out.reason == "tolerance" and out.iterations == len(out.history)
    assert rot <= ROTATION_MARGIN and tr <= TRANSLATION_MARGIN
    assert rot < TR.REF_ROTATION_ERROR and tr < TR.REF_TRANSLATION_ERROR
    assert out.iterations < TR.REF_LOOP_ITERATIONS
    assert out.history[0][2] == TR.LOOP_RADIUS and out.history[-1][2] == TR.LOOP_FINAL
    assert _same_alignment(out, m.track(qry, _config(), TR.LOOP_INIT, normals=True)), "run to run"
    assert _same_alignment(out, m.track(qry, _config(), TR.LOOP_INIT, normals=m.normals().normal, plane=PlaneConfig())), "True is normals().normal"
    assert torch.equal(m._block, before)
    # normals=None is the point-to-point run, bit for bit: align.icp with track_step as the step, as before
    from point_sam_amd import align as A
    point = m.track(qry, _config(), TR.LOOP_INIT)
    by_hand = A.icp(m, qry, _config(), TR.LOOP_INIT, None, step=lambda mm, points, pose, radius, row: mm.track_step(points, pose, radius, row, None, 1))
    assert _same_alignment(point, m.track(qry, _config(), TR.LOOP_INIT, normals=None, plane=None)) and _same_alignment(point, by_hand)
    assert point.reason == "fixed point" and point.iterations > out.iterations
    normal = m.normals().normal
    for bad in (normal[:-1], normal.double(), normal.cpu(), normal.reshape(-1)):
        with pytest.raises(ValueError, match="normals"):
            m.track(qry, _config(), TR.LOOP_INIT, normals=bad)
    with pytest.raises(ValueError, match="needs normals"):
        m.track(qry, _config(), TR.LOOP_INIT, plane=PlaneConfig())


def test_plane_track_pairs_no_freed_voxel(ops, loop):
    """occupied= frees a slab of voxels: they get no normal, enter no other voxel's normal and are never paired."""
    m, ref, qry, b = loop
    slab = m.cloud()[0][:, 2] < -0.25
    assert 50 < int(slab.sum()) < ref.V - 50
    out = m.track(qry, _config(), TR.LOOP_INIT, occupied=~slab, normals=True)
    assert 16 <= out.pairs < MN.REF_PLANE_USED[-1]
    nrm = m.normals(occupied=~slab)
    assert not bool(nrm.normal[slab].any()) and not bool(nrm.count[slab].any())
    want = MN.normals(ref, skip=slab.cpu().numpy())
    assert np.array_equal(nrm.count.cpu().numpy(), want["count"])
    assert _same_alignment(out, m.track(qry, _config(), TR.LOOP_INIT, occupied=~slab, normals=nrm.normal))
    assert _same_alignment(m.track(qry, _config(), TR.LOOP_INIT, occupied=True, normals=True), m.track(qry, _config(), TR.LOOP_INIT, normals=True))


# ------------------------------------------------------------------------------------------------ the predictor
@pytest.fixture(scope="module")
def pred():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd.model import PointCloudSAM
    from point_sam_amd.predictor import PointSAMPredictor
    cfg = get_config("tiny")
    return PointSAMPredictor(PointCloudSAM(cfg, random_state_dict(cfg, 3), "cuda", precision="f16x3"))


def test_predictor_map_align_passes_normals_through(ops, pred, loop):
    from point_sam_amd.align import PlaneConfig
    m, _, xyz, b = loop
    pred.set_scene(xyz, torch.zeros(len(b), 3, device="cuda"), max_points=1024)
    cfg = _config()
    out = pred.map_align(m, cfg, TR.LOOP_INIT, normals=True)
    assert _same_alignment(out, m.track(xyz, cfg, TR.LOOP_INIT, normals=True)) and out.converged and out.reason == "tolerance"
    loose = PlaneConfig(tol_rotation=1e-3, tol_translation=1e-3)
    nrm = m.normals(reach=2).normal
    part = pred.map_align(m, cfg, TR.LOOP_INIT, min_count=1, normals=nrm, plane=loose)
    assert _same_alignment(part, m.track(xyz, cfg, TR.LOOP_INIT, None, None, 1, nrm, loose)) and part.converged
    assert _same_alignment(pred.map_align(m, cfg, TR.LOOP_INIT), m.track(xyz, cfg, TR.LOOP_INIT))
    with pytest.raises(ValueError, match="needs normals"):
        pred.map_align(m, cfg, TR.LOOP_INIT, plane=loose)
