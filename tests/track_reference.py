"""Scan map tracking (include/pointsam_hip.h, "scan map tracking") in plain numpy, from the definition and independent of the package.  The map is
tests/scanmap_reference.py's RefMap (its cells, its pose arithmetic, its voxel mean); the sums are tests/align_reference.py's sums_from -- math.fsum
over the exact fp64 terms, so the exactly rounded values.

    takes part         query i, if `take` is None or take[i]
    posed coordinate   p = scanmap_reference.posed(query, pose words)
    cell               the query has one iff all three cells exist and -1 <= p_a <= 1 on every axis
    candidates         the map voxels v in the (2 reach + 1)^3 cells around cell(p) (cells off [0, 2^21)^3 skipped) with v < V, count(v) >= min_count,
                       skip[v] false and q = (dx dx + dy dy) + dz dz <= r2 in fp32, d = p - mean(v), NaN false
    pair               the candidate lowest in (q, v)

Two forms of one definition: `step(..., definition=True)` loops over the cube, query by query; `step` is vectorised over the queries for the ICP loop.
tests/test_track_cpu.py holds them equal.  Each returns (nearest [M] int32, sums [20], mass [20]).
"""
import math

import numpy as np

import align_reference as AR
import scanmap_reference as SM

F = np.float32
LIM = 1 << SM.AXIS_BITS


def r2_of(radius):
    r = F(radius)
    return F(r * r)


def reach_of(radius, voxel_size):
    """max(1, ceil(fl32(radius) * fl32(1 / fl32(voxel_size)))), the product in fp64"""
    return max(1, math.ceil(float(F(radius)) * float(SM.inv_h_of(voxel_size))))


def means(ref):
    """[V, 3] float32: the voxels' mean positions, RefMap.cloud()'s bits."""
    return ref.cloud()[0].reshape(ref.V, 3)


def _queries(ref, qry, pose, take):
    qry = np.ascontiguousarray(qry, dtype=F)
    p = SM.posed(qry, SM.pose_words(pose))
    cell, cell_ok = SM.cells(p, ref.inv_h)
    _, inside = SM.fixed(p)
    take = np.ones(len(qry), dtype=bool) if take is None else np.asarray(take, dtype=bool)
    return qry, p, cell, take & cell_ok.all(1) & inside.all(1)


def _allowed(ref, V, skip, min_count):
    V = ref.V if V is None else V
    ok = (np.arange(ref.V) < V) & (np.asarray(ref.count, dtype=np.int64).reshape(ref.V) >= min_count)
    if skip is not None:
        ok[:min(V, ref.V)] &= ~np.asarray(skip, dtype=bool)[:min(V, ref.V)]
    return ok


def _q(p, s):
    with np.errstate(invalid="ignore", over="ignore"):
        d = (p - s).astype(F)
        return ((d[..., 0] * d[..., 0]).astype(F) + (d[..., 1] * d[..., 1]).astype(F)).astype(F) + (d[..., 2] * d[..., 2]).astype(F)


def nearest_definition(ref, qry, r2, reach, pose=None, take=None, V=None, skip=None, min_count=1):
    """-> (nearest [M] int32, q [M] float32, has_cell [M] bool): per query the first of its candidates sorted by (q, v)."""
    qry, p, cell, has_cell = _queries(ref, qry, pose, take)
    mean, allowed = means(ref), _allowed(ref, V, skip, min_count)
    near, best = np.full(len(qry), -1, dtype=np.int32), np.zeros(len(qry), dtype=F)
    r2 = F(r2)
    for i in np.nonzero(has_cell)[0].tolist():
        cx, cy, cz = (int(c) for c in cell[i])
        found = []
        for dz in range(-reach, reach + 1):
            for dy in range(-reach, reach + 1):
                for dx in range(-reach, reach + 1):
                    c = (cx + dx, cy + dy, cz + dz)
                    if min(c) < 0 or max(c) >= LIM:
                        continue
                    v = ref.id_of.get(c[0] | (c[1] << SM.AXIS_BITS) | (c[2] << (2 * SM.AXIS_BITS)))
                    if v is None or not allowed[v]:
                        continue
                    q = F(_q(p[i], mean[v]))
                    if q <= r2:
                        found.append((q, v))
        if found:
            best[i], near[i] = min(found)
    return near, best, has_cell


def nearest(ref, qry, r2, reach, pose=None, take=None, V=None, skip=None, min_count=1):
    """The same, vectorised over the queries: the map's keys sorted, one binary search per cell of the cube."""
    qry, p, cell, has_cell = _queries(ref, qry, pose, take)
    M = len(qry)
    near, best = np.full(M, -1, dtype=np.int64), np.zeros(M, dtype=F)
    if ref.V == 0:
        return near.astype(np.int32), best, has_cell
    mean, allowed = means(ref), _allowed(ref, V, skip, min_count)
    keys = np.asarray(ref.keys, dtype=np.int64)
    order = np.argsort(keys, kind="stable")
    skeys = keys[order]
    r2 = F(r2)
    for dz in range(-reach, reach + 1):
        for dy in range(-reach, reach + 1):
            for dx in range(-reach, reach + 1):
                n = cell + np.array([dx, dy, dz], dtype=np.int64)
                ok = has_cell & (n >= 0).all(1) & (n < LIM).all(1)
                n = np.where(ok[:, None], n, 0)
                k = n[:, 0] | (n[:, 1] << SM.AXIS_BITS) | (n[:, 2] << (2 * SM.AXIS_BITS))
                at = np.clip(np.searchsorted(skeys, k), 0, ref.V - 1)
                v = order[at]
                ok &= (skeys[at] == k) & allowed[v]
                q = _q(p, mean[v])
                with np.errstate(invalid="ignore"):
                    better = ok & (q <= r2) & ((near < 0) | (q < best) | ((q == best) & (v < near)))
                near[better], best[better] = v[better], q[better]
    return near.astype(np.int32), best, has_cell


def step(ref, qry, radius, pose=None, take=None, V=None, skip=None, min_count=1, reach=None, r2=None, definition=False):
    """One step -> (nearest [M] int32, sums [20], mass [20]).  radius: the search radius; reach None: reach_of(radius, the map's voxel size);
    r2 None: fl32(radius * radius)."""
    find = nearest_definition if definition else nearest
    reach = max(1, math.ceil(float(F(radius)) * float(ref.inv_h))) if reach is None else reach
    near, q, has_cell = find(ref, qry, r2_of(radius) if r2 is None else r2, reach, pose, take, V, skip, min_count)
    return (near,) + AR.sums_from(means(ref) if ref.V else np.zeros((1, 3), dtype=F), qry, near, q, has_cell)


# ------------------------------------------------------------------------------------------------ the loop
def icp(ref, qry, radius, final_radius=None, shrink=1.0, iterations=30, min_pairs=16, init=None, take=None, skip=None, min_count=1):
    """align_reference.icp with `step` above as its step -> dict(pose [3, 4] float64, pairs, coverage, rms, iterations, converged, history, nearest)."""
    pose = np.concatenate([np.eye(3), np.zeros((3, 1))], 1) if init is None else np.asarray(init, dtype=np.float64)[:3].copy()
    out = dict(pose=pose, pairs=0, coverage=0.0, rms=float("nan"), iterations=0, converged=False, history=[], nearest=None)
    last = radius if final_radius is None else final_radius
    for k in range(iterations):
        rk = AR.radius_of_step(radius, final_radius, shrink, k)
        near, m, _ = step(ref, qry, rk, pose.astype(F), take, None, skip, min_count)
        out["iterations"] = k + 1
        if m[0] < min_pairs:
            break
        try:
            Rm, t, rms = AR.solve(m)
        except ValueError:
            break
        new = np.concatenate([Rm, t[:, None]], 1)
        same = np.array_equal(new.astype(F), pose.astype(F))
        pose = new
        out.update(pose=pose, pairs=int(m[0]), coverage=m[0] / max(m[19], 1.0), rms=rms, nearest=near)
        out["history"].append((int(m[0]), rms, rk))
        if same and rk == last:
            out["converged"] = True
            break
    return out


# ------------------------------------------------------------------------------------------------ the inputs the tests share
LOOP_H = 2.0 ** -4
LOOP_RADIUS, LOOP_FINAL, LOOP_SHRINK = 2 * LOOP_H, LOOP_H, 0.8
LOOP_MAX_VOXELS = 4096
# the start of the loop: the truth turned by half a degree about a fixed axis and moved by half a voxel
LOOP_INIT = np.concatenate([AR.rotation([0.0, 0.0, 1.0], 0.5) @ AR.TRUE_POSE[:, :3], (AR.TRUE_POSE[:, 3] + LOOP_H / 2 * np.array([0.0, 0.0, 1.0]))[:, None]], 1)
# What the reference loop (loop_reference on loop_case()) was measured to do on the CPU; tests/test_track_cpu.py recomputes and holds all of it:
# converged (a fixed point) at step 18 of at most 30 with all 6100 queries paired against 601 voxels; against TRUE_POSE its rotation is off by
# 6.3695e-3 rad and its translation by 2.3991e-3 -- the map is a cloud of voxel means half a voxel apart, not the surface.
REF_LOOP_ITERATIONS, REF_LOOP_VOXELS, REF_LOOP_PAIRS = 18, 601, 6100
REF_ROTATION_ERROR, REF_TRANSLATION_ERROR = 6.3695e-3, 2.3991e-3


def loop_case():
    """-> (RefMap of align_reference.icp_case()'s cloud a, added once under the identity at LOOP_H; a; b the queries)."""
    a, b = AR.icp_case()
    ref = SM.RefMap(LOOP_H, LOOP_MAX_VOXELS)
    ref.add(a, np.zeros_like(a))
    return ref, a, b


def loop_reference(ref, b, **more):
    return icp(ref, b, LOOP_RADIUS, LOOP_FINAL, LOOP_SHRINK, init=LOOP_INIT, **more)


def random_case(seed, n_map=1500, n_qry=700, h=2.0 ** -3):
    """A case (cases() below): a seeded map of uniformly random points in [-0.9, 0.9]^3, in two adds so that many voxels hold several points, and
    queries beside them."""
    g = np.random.default_rng(seed)
    adds = [g.uniform(-0.9, 0.9, size=(n_map // 2, 3)).astype(F) for _ in range(2)]
    return dict(name=f"random {seed}", h=h, max_voxels=4096, adds=adds, qry=g.uniform(-0.95, 0.95, size=(n_qry, 3)).astype(F))


# ------------------------------------------------------------------------------------------------ the cases of the step
H = 2.0 ** -3
UP1, DOWN1 = np.nextafter(F(1), F(2)), np.nextafter(F(-1), F(-2))


def build(case):
    """The RefMap of a case: its adds in order, each under the identity."""
    ref = SM.RefMap(case["h"], case["max_voxels"])
    for pts in case["adds"]:
        ref.add(pts, np.zeros_like(pts))
    return ref


def reference(case, ref=None, definition=False):
    ref = build(case) if ref is None else ref
    return step(ref, case["qry"], case.get("radius", case["h"]), case.get("pose"), case.get("take"), case.get("V"), case.get("skip"),
                case.get("min_count", 1), case.get("reach"), None, definition)


def _case(name, adds, qry, h=H, max_voxels=4096, **more):
    return dict(name=name, h=h, max_voxels=max_voxels, adds=[np.asarray(a, dtype=F).reshape(-1, 3) for a in adds], qry=np.asarray(qry, dtype=F).reshape(-1, 3), **more)


def cases():
    """Every case of the step, shared by the CPU test (definition form == vectorised form) and the GPU test (device == reference)."""
    out = []
    g = np.random.default_rng(7)
    half = g.uniform(-0.9, 0.9, size=(2, 750, 3)).astype(F)
    pose = SM.rotation_pose(3.0, -2.0, (0.01, -0.02, 0.015))
    for M in (1, 63, 64, 65, 257, 2113):                           # 2113 = 34 waves: a combine segment adds two rows
        q = g.uniform(-0.95, 0.95, size=(M, 3)).astype(F)
        out.append(_case(f"sizes M={M}", half, q, pose=pose if M % 2 else None))
    q = g.uniform(-0.95, 0.95, size=(300, 3)).astype(F)
    for reach in (1, 2, 4):                                        # the same r2 under a wider cube: the same outputs
        out.append(_case(f"reach {reach}", half, q, reach=reach, pose=pose))
    out.append(_case("radius 2 h", half, q, radius=2 * H))
    out.append(_case("radius h / 2", half, q, radius=H / 2, pose=pose))
    # a table at load 0.5: 32 voxels in a 4 x 4 x 2 block of cells, max_voxels = 32, 64 slots
    grid = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(2), indexing="ij"), -1).reshape(-1, 3)
    full = ((grid + g.uniform(0.1, 0.9, size=grid.shape)) * H - 0.25).astype(F)
    out.append(_case("full table", [full], g.uniform(-0.4, 0.4, size=(200, 3)), max_voxels=32))
    # a tie and q == r2 at once: two single-point voxels at exactly 2^-3 from the query on either side, along each axis and in both id orders; the
    # lower id wins whichever cell is probed first.  One voxel an ulp further (q = r2 + 2^-29) is not paired.
    c = np.array([0.0625, 0.0625, 0.0625])
    tie_map, tie_q = [], []
    for k, (axis, sign) in enumerate(((0, 1), (0, -1), (1, 1), (1, -1), (2, 1), (2, -1))):
        o = c + np.array([0.0, 0.0, 0.0]) + 0.5 * np.array([k % 3 - 1, k // 3, 0])      # six sites far apart
        e = np.zeros(3)
        e[axis] = 0.125 * sign
        tie_map += [o + e, o - e]                                  # ids 2 k and 2 k + 1: the lower one on the `sign` side
        tie_q.append(o)
    far = np.array([-0.5625, -0.5625, -0.5625])
    tie_map.append(far + np.array([0.125, 3 * 2.0 ** -16, 0.0]))   # q = fl32(2^-6 + 9 * 2^-32) = 2^-6 + 2^-29: one ulp past r2
    tie_q.append(far)
    out.append(_case("tie and q == r2", [np.array(tie_map)], np.array(tie_q)))
    # queries without a cell beside queries on the boundary, which have one
    edge = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, 0, -1), (1, 1, 1), (-1, -1, -1), (UP1, 0, 0), (0, DOWN1, 0), (0, 0, UP1), (np.nan, 0, 0),
            (0, np.inf, 0), (0, 0, -np.inf), (0.99, 0.99, 0.99), (-0.99, -0.99, -0.99)]
    walls = np.array([(0.95, 0.05, 0.05), (-0.95, 0.05, 0.05), (0.05, 0.95, 0.05), (0.05, 0.05, -0.95), (0.95, 0.95, 0.95), (-0.95, -0.95, -0.95),
                      (1, 1, 1), (-1, -1, -1)])
    out.append(_case("boundary", [walls], edge, reach=2, radius=2 * H))
    out.append(_case("boundary posed", [walls], edge, reach=4, radius=2 * H, pose=np.concatenate([np.eye(3), [[2.0 ** -10], [0], [0]]], 1)))
    # the cube leaves the grid at the high end: h = 2^-20, cells 2^21 - 1 .. 2^21 - 4 in every axis
    tiny = 2.0 ** -20
    top = 1.0 - tiny * g.uniform(0.05, 3.9, size=(40, 3))
    out.append(_case("high corner", [top[:20]], top[20:], h=tiny, max_voxels=64, reach=4, radius=4 * tiny))
    # skip, min_count, V, bits
    skip = np.zeros(1500, dtype=bool)
    skip[::3] = True
    out.append(_case("skip", half, q, skip=skip, pose=pose))
    out.append(_case("min_count 2", half, q, min_count=2, radius=2 * H))
    out.append(_case("V below the map's", half, q, V=700, radius=2 * H))
    out.append(_case("bits", half, q, take=g.uniform(size=300) < 0.6, pose=pose))
    # one voxel, skipped: the query has a cell (word 19) and no pair (word 0); beside it a query whose nearest is skipped and whose second is not
    lone = np.array([(0.5, 0.5, 0.5), (-0.5, -0.5, -0.5), (-0.45, -0.55, -0.5)])
    out.append(_case("skip hands on", [lone], [(0.51, 0.5, 0.5), (-0.49, -0.5, -0.5)], skip=np.array([True, True, False]), radius=H))
    return out


def lattice_case():
    """Single-point voxels and queries on the lattice 2^-6 Z^3: every term of every sum is a small multiple of 2^-12, so every sum is exact in any order."""
    g = np.random.default_rng(11)
    pts = np.unique(g.integers(-60, 60, size=(900, 3)), axis=0)
    cell = np.unique(np.floor((pts / 64.0 + 1.0) / H).astype(np.int64), axis=0, return_index=True)[1]      # one point per voxel
    q = g.integers(-60, 60, size=(700, 3)) / 64.0
    return _case("lattice", [pts[np.sort(cell)] / 64.0], q)
