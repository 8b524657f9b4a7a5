"""Plain numpy reference of one point-to-plane ICP step, of its solve and of the loop, written from the definition in include/pointsam_hip.h ("pose
between two clouds": psam_plane_step) and independent of the package.  The pairs are tests/align_reference.py's (nearest / nearest_definition: the
same cells, posed coordinate and fp32 distance); the terms are formed in fp64 with exactly the operations and the order the header states, the sums
are math.fsum over them, so they are the exactly rounded sums of the terms.

    used pair          its source normal n has nn = (n_x n_x + n_y n_y) + n_z n_z, in fp32, finite and > 0
    terms              p = the posed coordinate (fp32 words), s = the pair, n its normal, converted to fp64; d = p - s;
                       r = (d_x n_x + d_y n_y) + d_z n_z; c = p x n with c_x = p_y n_z - p_z n_y and cyclic; J = (c, n)
    sums               [0] used pairs, [1] sum q, [2] sum r r, [3..8] sum J_a r, [9..29] sum J_a J_b for a <= b row-major,
                       [30] paired queries whose pair was not used, [31] participating queries that have a cell
"""
import math

import numpy as np

import align_reference as A
import transfer_reference as T

f32 = np.float32
SUMS = 32
TRIU = [(a, b) for a in range(6) for b in range(a, 6)]


def used_normals(normals):
    """[N] bool: nn in fp32, every operation rounded on its own, finite and > 0."""
    n = np.asarray(normals, dtype=f32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        nn = ((n[:, 0] * n[:, 0]).astype(f32) + (n[:, 1] * n[:, 1]).astype(f32)).astype(f32) + (n[:, 2] * n[:, 2]).astype(f32)
        nn = nn.astype(f32)
        return np.isfinite(nn) & (nn > 0)


def sums_from(src, normals, qry, pose, near, q, has_cell):
    """-> (sums [32] float64, the exactly rounded sums of the terms; mass [32] float64, sum |term| per word)."""
    src, normals, qry = np.asarray(src, dtype=f32), np.asarray(normals, dtype=f32), np.asarray(qry, dtype=f32)
    paired = near >= 0
    ok = np.zeros(len(qry), dtype=bool)
    ok[paired] = used_normals(normals)[near[paired]]
    i = np.nonzero(ok)[0]
    p = T.posed(qry, pose)[i].astype(np.float64)                    # pose_apply's fp32 words, converted
    s, n = src[near[i]].astype(np.float64), normals[near[i]].astype(np.float64)
    d = p - s
    r = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    J = [p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2], p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0], n[:, 0], n[:, 1], n[:, 2]]
    cols = [np.ones(len(i)), q[i].astype(np.float64), r * r] + [J[a] * r for a in range(6)] + [J[a] * J[b] for a, b in TRIU]
    cols += [np.ones(int((paired & ~ok).sum())), np.ones(int(has_cell.sum()))]
    assert len(cols) == SUMS
    return (np.array([math.fsum(c.tolist()) for c in cols], dtype=np.float64),
            np.array([math.fsum(np.abs(c).tolist()) for c in cols], dtype=np.float64))


def step(src, normals, r_index, qry, pose=None, radius=None, take=None, definition=False):
    """One point-to-plane ICP step -> (nearest [M] int32, sums [32], mass [32]).  pose: None or fp32-representable words (as the device is given)."""
    find = A.nearest_definition if definition else A.nearest
    near, q, has_cell = find(src, r_index, qry, A.r2_of(r_index if radius is None else radius), pose, take)
    return (near,) + sums_from(src, normals, qry, pose, near, q, has_cell)


# ------------------------------------------------------------------------------------------------ the solve and the loop
TOL_ROTATION, TOL_TRANSLATION, CONDITION = 1e-6, 1e-6, 1e-10         # a default PlaneConfig, restated: this file does not import the package


def rodrigues(w):
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    a, b = (1.0, 0.5) if th < 1e-12 else (math.sin(th) / th, (1.0 - math.cos(th)) / (th * th))
    return np.eye(3) + a * K + b * (K @ K)


def solve(m, pose, condition=CONDITION):
    """sums, the pose they were taken under (3 x 4 fp64) -> (new pose, rms, |omega|, |v|); ValueError for fewer than 6 used pairs or a system whose
    smallest eigenvalue is <= condition x the largest."""
    if m[0] < 6:
        raise ValueError("degenerate")
    Am = np.zeros((6, 6))
    for k, (a, b) in enumerate(TRIU):
        Am[a, b] = Am[b, a] = m[9 + k]
    g = np.array(m[3:9])
    lam, V = np.linalg.eigh(Am)
    if lam[0] <= condition * lam[-1]:
        raise ValueError("degenerate")
    z = -sum(V[:, k] * (V[:, k] @ g) / lam[k] for k in range(6))
    W = rodrigues(z[:3])
    U, _, Vt = np.linalg.svd(W @ pose[:, :3])
    Rm = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))]) @ Vt
    t = W @ pose[:, 3] + z[3:]
    return (np.concatenate([Rm, t[:, None]], 1), math.sqrt(max(m[2] + z @ g, 0.0) / m[0]), float(np.linalg.norm(z[:3])),
            float(np.linalg.norm(z[3:])))


def icp(src, normals, qry, radius, final_radius=None, shrink=1.0, iterations=30, min_pairs=16, init=None, take=None):
    """-> dict(pose [3, 4] float64, pairs, coverage, rms, iterations, converged, reason, history, updates).  Every update is composed onto the fp64
    pose; the step sees its fp32 rounding.  Converged: at the final radius the update is within the tolerances, or the fp32 words repeat."""
    pose = np.concatenate([np.eye(3), np.zeros((3, 1))], 1) if init is None else np.asarray(init, dtype=np.float64)[:3].copy()
    out = dict(pose=pose, pairs=0, coverage=0.0, rms=float("nan"), iterations=0, converged=False, reason="iterations", history=[], updates=[])
    last = radius if final_radius is None else final_radius
    for k in range(iterations):
        rk = A.radius_of_step(radius, final_radius, shrink, k)
        _, m, _ = step(src, normals, radius, qry, pose.astype(f32), rk, take)
        out["iterations"] = k + 1
        if m[0] < min_pairs:
            out["reason"] = "pairs"
            break
        try:
            new, rms, rot, tr = solve(m, pose)
        except ValueError:
            out["reason"] = "degenerate"
            break
        same = np.array_equal(new.astype(f32), pose.astype(f32))
        small = rot <= TOL_ROTATION and tr <= TOL_TRANSLATION
        pose = new
        out.update(pose=pose, pairs=int(m[0]), coverage=m[0] / max(m[31], 1.0), rms=rms)
        out["history"].append((int(m[0]), rms, rk))
        out["updates"].append((rot, tr))
        if rk == last and (small or same):
            out.update(converged=True, reason="tolerance" if small else "fixed point")
            break
    return out


# ------------------------------------------------------------------------------------------------ the inputs the tests share
SPHERE_CENTRE = np.array([0.15, 0.1, -0.05])


def analytic_normals(a):
    """The normals of align_reference.surfaces at its points a [N, 3]: (0, 0, 1) on the floor z = -0.35, (1, 0, 0) on the wall x = -0.5, (0, 1, 0) on the
    wall y = -0.4, radial on the sphere -- decided by which surface the point lies on (to 1e-6: the points are fp32 roundings); a point on two of them takes
    the one written last below."""
    a = np.asarray(a, dtype=np.float64)
    n = np.zeros_like(a)
    d = a - SPHERE_CENTRE
    ball = np.abs(np.linalg.norm(d, axis=1) - 0.2) < 1e-6
    n[ball] = d[ball] / np.linalg.norm(d[ball], axis=1, keepdims=True)
    n[np.abs(a[:, 1] + 0.4) < 1e-6] = (0.0, 1.0, 0.0)
    n[np.abs(a[:, 0] + 0.5) < 1e-6] = (1.0, 0.0, 0.0)
    n[np.abs(a[:, 2] + 0.35) < 1e-6] = (0.0, 0.0, 1.0)
    assert (np.abs(np.linalg.norm(n, axis=1) - 1.0) < 1e-9).all()   # every point lies on one of the four
    return n.astype(f32)


def plane_case():
    """-> (A [6000, 3] the sources, their analytic normals [6000, 3], B [6100, 3] the queries), all float32: align_reference.icp_case() with normals."""
    a, b = A.icp_case()
    return a, analytic_normals(a), b


# What the reference loop above (icp, on plane_case() under align_reference's ICP_RADIUS / ICP_FINAL / ICP_SHRINK and the tolerances above) was measured
# to do; tests/test_align_plane_cpu.py recomputes and holds all of it: converged by tolerance at step REF_PLANE_STEPS (point-to-point: 40) with the
# pair counts REF_PLANE_PAIRS per step; against TRUE_POSE its rotation is off by REF_PLANE_ROTATION_ERROR rad and its translation by
# REF_PLANE_TRANSLATION_ERROR (point-to-point: 1.4141e-3 and 2.9329e-4).  Carried with its pose instead of the true one (transfer at
# align_reference.TRANSFER_RADIUS, mask_rows), the packed masks agree on REF_PLANE_MASK_SHARE of the points at worst.
# Measured: 5 steps, updates (|omega|, |v|) of 6.0e-2 / 2.9e-2, 1.2e-2 / 2.4e-3, 6.3e-4 / 8.4e-5, 4.6e-5 / 1.3e-5 and 1.9e-8 / 3.4e-8; linearised rms
# 7.194e-4; the 6 x 6 system's condition number at the answer is 16.8.
REF_PLANE_STEPS = 5
REF_PLANE_PAIRS = (6100, 6100, 6100, 6100, 6100)
REF_PLANE_ROTATION_ERROR, REF_PLANE_TRANSLATION_ERROR, REF_PLANE_MASK_SHARE = 1.2249e-4, 8.1916e-5, 6100 / 6100


def axis_normals(n, seed, zeros=0.0):
    """n axis-aligned unit normals (+-x, +-y, +-z), a share `zeros` of them (0, 0, 0): with lattice coordinates every term is a short dyadic number."""
    g = np.random.default_rng(seed)
    out = np.zeros((n, 3), dtype=f32)
    out[np.arange(n), g.integers(0, 3, size=n)] = g.choice(np.array([-1.0, 1.0], dtype=f32), size=n)
    out[g.uniform(size=n) < zeros] = 0
    return out
