"""Scan map normals and point-to-plane tracking (include/pointsam_hip.h, "scan map normals" and psam_scanmap_plane_step) in plain numpy and Python
integers, from the definition and independent of the package.  The map is tests/scanmap_reference.py's RefMap; a voxel's point is its mean
(track_reference.means: RefMap.cloud()'s bits) in superpoint_reference.fixed's fixed point; the eigen-solve is superpoint_reference.normals
(numpy.linalg.eigh of float(S)); the pair of a query is track_reference.nearest's and the sums are align_plane_reference.sums_from's -- math.fsum over
the exact fp64 terms, so the exactly rounded values.

    allowed voxel      u < V, count(u) >= min_count, skip[u] false
    neighbourhood      of v: the allowed voxels in the (2 reach + 1)^3 cells around v's own cell (cells off [0, 2^21)^3 skipped); empty when v itself
                       is not allowed
    scatter            n, s = sum q, P = sum q q^T over the neighbourhood's means, S = n P - s s^T in Python integers (exact)
    normal             n < min_voxels: (0, 0, 0) and curvature 0; else the eigenvector of the smallest eigenvalue of float(S), fp32, the component of
                       largest magnitude positive; curvature l0 / (l0 + l1 + l2)
    plane step         track_reference's pair; used iff the pair's normal has nn (fp32) finite and > 0; align_plane_reference's terms with p the
                       posed query, s the pair's mean, n its normal
"""
import numpy as np

import align_plane_reference as AP
import align_reference as AR
import scanmap_reference as SM
import superpoint_reference as SP
import track_reference as TR

F = np.float32
MASK = (1 << SM.AXIS_BITS) - 1
GAP = 1e-4                       # a normal is compared only where l1 - l0 >= GAP * l2 (tests/test_gpu_superpoints.py's rule)


def allowed(ref, V=None, skip=None, min_count=1):
    """[ref.V] bool."""
    V = ref.V if V is None else V
    ok = (np.arange(ref.V) < V) & (np.asarray(ref.count, dtype=np.int64).reshape(ref.V) >= min_count)
    if skip is not None:
        ok[:min(V, ref.V)] &= ~np.asarray(skip, dtype=bool)[:min(V, ref.V)]
    return ok


def scatter(ref, reach=1, V=None, skip=None, min_count=1):
    """-> (count [V] int64, s [V, 3] int64, S: V rows of six Python integers xx, xy, xz, yy, yz, zz), V at most the map's."""
    V = ref.V if V is None else V
    assert 0 < V <= ref.V and reach in (1, 2)
    q, inside = SP.fixed(TR.means(ref))
    assert inside.all()
    q = q.tolist()                                                 # Python integers from here on
    ok = allowed(ref, V, skip, min_count)
    count, s_out, S = np.zeros(V, dtype=np.int64), np.zeros((V, 3), dtype=np.int64), []
    for v in range(V):
        n, s, P = 0, [0, 0, 0], [0] * 6
        if ok[v]:
            key = int(ref.keys[v])
            c = (key & MASK, (key >> SM.AXIS_BITS) & MASK, key >> (2 * SM.AXIS_BITS))
            for dz in range(-reach, reach + 1):
                for dy in range(-reach, reach + 1):
                    for dx in range(-reach, reach + 1):
                        a = (c[0] + dx, c[1] + dy, c[2] + dz)
                        if min(a) < 0 or max(a) > MASK:
                            continue
                        u = ref.id_of.get(a[0] | (a[1] << SM.AXIS_BITS) | (a[2] << (2 * SM.AXIS_BITS)))
                        if u is None or not ok[u]:
                            continue
                        n += 1
                        for k in range(3):
                            s[k] += q[u][k]
                        for k, (i, j) in enumerate(SP.PAIRS):
                            P[k] += q[u][i] * q[u][j]
        count[v], s_out[v] = n, s
        S.append([n * P[k] - s[i] * s[j] for k, (i, j) in enumerate(SP.PAIRS)])
    return count, s_out, S


def normals(ref, reach=1, min_voxels=5, V=None, skip=None, min_count=1):
    """-> dict(count [V] int32, scatter [V, 6] float64 = float(S), normal [V, 3] f32, curvature [V] f32, vector [V, 3] and curvature64 [V]: the same
    in fp64 before the rounding and the sign rule, lam [V, 3] ascending eigenvalues, valid [V] bool: count >= min_voxels, gap [V] bool: valid and
    l1 - l0 >= GAP * l2)."""
    count, s, S = scatter(ref, reach, V, skip, min_count)
    normal, curvature, lam, _ = SP.normals(count, s, S, min_voxels)
    vector, curvature64, _ = SP.eigen(count, S, min_voxels)
    valid = count >= max(min_voxels, 1)
    return dict(count=count.astype(np.int32), scatter=SP.scatter_float(S), normal=normal, curvature=curvature, vector=vector, curvature64=curvature64,
                lam=lam, valid=valid, gap=valid & (lam[:, 1] - lam[:, 0] >= GAP * lam[:, 2]))


# ------------------------------------------------------------------------------------------------ the plane step
def _pose34(pose):
    return None if pose is None else np.asarray(pose, dtype=np.float64)[:3]


def step(ref, qry, nrm, radius, pose=None, take=None, V=None, skip=None, min_count=1, reach=None, r2=None, definition=False):
    """One point-to-plane step -> (nearest [M] int32, sums [32], mass [32]).  nrm [V, 3] f32, one per voxel id, taken as given."""
    find = TR.nearest_definition if definition else TR.nearest
    reach = TR.reach_of(radius, 1.0 / float(ref.inv_h)) if reach is None else reach
    near, q, has_cell = find(ref, qry, TR.r2_of(radius) if r2 is None else r2, reach, pose, take, V, skip, min_count)
    rows = np.zeros((ref.V, 3), dtype=F)
    rows[:len(nrm)] = np.asarray(nrm, dtype=F)[:ref.V]              # V below the map's: ids at or above V are never paired
    return (near,) + AP.sums_from(TR.means(ref), rows, qry, _pose34(pose), near, q, has_cell)


def reference(case, nrm, ref=None, definition=False):
    """track_reference.reference for the plane step: a case of track_reference.cases() and one normal per voxel."""
    ref = TR.build(case) if ref is None else ref
    return step(ref, case["qry"], nrm, case.get("radius", case["h"]), case.get("pose"), case.get("take"), case.get("V"), case.get("skip"),
                case.get("min_count", 1), case.get("reach"), None, definition)


# ------------------------------------------------------------------------------------------------ the loop
def icp(ref, nrm, qry, radius, final_radius=None, shrink=1.0, iterations=30, min_pairs=16, init=None, take=None, skip=None, min_count=1):
    """align_plane_reference.icp with `step` above as its step -> dict(pose, pairs, coverage, rms, iterations, converged, reason, history, updates,
    unused: word [30] per step)."""
    pose = np.concatenate([np.eye(3), np.zeros((3, 1))], 1) if init is None else np.asarray(init, dtype=np.float64)[:3].copy()
    out = dict(pose=pose, pairs=0, coverage=0.0, rms=float("nan"), iterations=0, converged=False, reason="iterations", history=[], updates=[], unused=[])
    last = radius if final_radius is None else final_radius
    for k in range(iterations):
        rk = AR.radius_of_step(radius, final_radius, shrink, k)
        _, m, _ = step(ref, qry, nrm, rk, pose.astype(F), take, None, skip, min_count)
        out["iterations"] = k + 1
        if m[0] < min_pairs:
            out["reason"] = "pairs"
            break
        try:
            new, rms, rot, tr = AP.solve(m, pose)
        except ValueError:
            out["reason"] = "degenerate"
            break
        same = np.array_equal(new.astype(F), pose.astype(F))
        small = rot <= AP.TOL_ROTATION and tr <= AP.TOL_TRANSLATION
        pose = new
        out.update(pose=pose, pairs=int(m[0]), coverage=m[0] / max(m[31], 1.0), rms=rms)
        out["history"].append((int(m[0]), rms, rk))
        out["updates"].append((rot, tr))
        out["unused"].append(int(m[30]))
        if rk == last and (small or same):
            out.update(converged=True, reason="tolerance" if small else "fixed point")
            break
    return out


def loop_reference(ref, b, reach=1, min_voxels=5, **more):
    """The plane loop on track_reference.loop_case(): normals of the map at `reach`, then icp under track_reference's LOOP_* schedule and LOOP_INIT."""
    nrm = normals(ref, reach, min_voxels)
    return nrm, icp(ref, nrm["normal"], b, TR.LOOP_RADIUS, TR.LOOP_FINAL, TR.LOOP_SHRINK, init=TR.LOOP_INIT, **more)


# What loop_reference (reach 1, min_voxels 5) was measured to do on the CPU; tests/test_map_normals_cpu.py recomputes and holds all of it.  596 of the
# 601 voxels have a normal and every one of those has the eigenvalue gap; the loop converges by tolerance at step 6 (point-to-point:
# track_reference.REF_LOOP_ITERATIONS = 18); every query is paired at every step, and the pairs whose voxel has no normal are the unused ones.
REF_VALID_VOXELS, REF_GAPLESS_VOXELS = 596, 0
REF_PLANE_STEPS = 6
REF_PLANE_USED = (6046, 6057, 6058, 6058, 6058, 6058)
REF_PLANE_UNUSED = (54, 43, 42, 42, 42, 42)
# against align_reference.TRUE_POSE (point-to-point: 6.3695e-3 rad and 2.3991e-3); the last update is |omega| = 1.2e-8, |v| = 3.5e-8, the rms 3.648e-3
REF_PLANE_ROTATION_ERROR, REF_PLANE_TRANSLATION_ERROR = 6.7592e-4, 1.5397e-4
