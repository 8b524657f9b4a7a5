"""Plain numpy reference of the radius 3-NN transfer plan, written from the definition in include/pointsam_hip.h and independent of the package.  Cells are
tests/scene_reference.py's, the weights follow tests/interp_reference.py's plan.  All arithmetic is fp32 and every intermediate is cast to float32, so
each operation is rounded on its own.

    h = r, inv_h = fl32(1 / r), r2 = fl32(r * r), origin = fl32(min of the sources per axis - r)
    query coordinate   p = the query bit for bit, or p_a = ((P[a][0] x + P[a][1] y) + P[a][2] z) + P[a][3] with a pose
    candidates         the indexed sources j of the 27 cells around cell(p) with q_j = (dx dx + dy dy) + dz dz <= r2
    selection          the three lowest in (q, j), lexicographic; missing entries idx = -1, w = 0
    exact hit          q_0 == 0 or one candidate: idx3 = (j0, -1, -1), w3 = (1, 0, 0)
    otherwise          a_j = 1 / max(q_j, eps); s = a0 + a1 (+ a2); w_j = a_j / s
"""
import numpy as np

import scene_reference as R

f32 = np.float32


def parameters(src, r):
    """-> (origin [3] float32, inv_h, r2): what ops.transfer_index derives from the sources and the radius."""
    r = f32(r)
    src = np.asarray(src, dtype=f32)
    return (src.min(0) - r).astype(f32), f32(1) / r, f32(r * r)


def posed(qry, pose=None):
    qry = np.asarray(qry, dtype=f32)
    if pose is None:
        return qry
    P = np.asarray(pose, dtype=f32)[:3]
    x, y, z = qry[:, 0], qry[:, 1], qry[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        cols = [((((P[a, 0] * x).astype(f32) + (P[a, 1] * y).astype(f32)).astype(f32) + (P[a, 2] * z).astype(f32)).astype(f32) + P[a, 3]).astype(f32)
                for a in range(3)]
    return np.stack(cols, 1).astype(f32)


def _dist(p, pts):
    with np.errstate(invalid="ignore", over="ignore"):
        d = (p[None, :] - pts).astype(f32)
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        return (((dx * dx).astype(f32) + (dy * dy).astype(f32)).astype(f32) + (dz * dz).astype(f32)).astype(f32)


def index(src, r, origin):
    """{cell (x, y, z): [source indices]}; a source without a cell is left out."""
    c, bad = R.cells(src, r, origin)
    table = {}
    for j in np.nonzero(~bad)[0].tolist():
        table.setdefault(tuple(int(v) for v in c[j]), []).append(j)
    return table


def candidates_grid(src, r, qry, pose=None, origin=None):
    """Per query the (j, q) arrays of its candidates, sorted by (q, j): the 27-cell definition."""
    src = np.asarray(src, dtype=f32)
    o, _, r2 = parameters(src, r)
    origin = o if origin is None else np.asarray(origin, dtype=f32)
    table = index(src, r, origin)
    p = posed(qry, pose)
    c, bad = R.cells(p, r, origin)
    out = []
    for i in range(len(p)):
        js = []
        if not bad[i]:
            cx, cy, cz = (int(v) for v in c[i])
            for dz in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        cell = (cx + dx, cy + dy, cz + dz)
                        if min(cell) >= 0 and max(cell) < (1 << R.AXIS_BITS):
                            js += table.get(cell, [])
        out.append(_select(p[i], src, np.asarray(js, dtype=np.int64), r2))
    return out


def candidates_brute(src, r, qry, pose=None):
    """The same over ALL sources, in the same fp32 arithmetic: the true radius search."""
    src = np.asarray(src, dtype=f32)
    _, _, r2 = parameters(src, r)
    p = posed(qry, pose)
    every = np.arange(len(src), dtype=np.int64)
    return [_select(p[i], src, every, r2) for i in range(len(p))]


def _select(p, src, js, r2):
    if len(js) == 0:
        return js, np.zeros(0, dtype=f32)
    q = _dist(p, src[js])
    with np.errstate(invalid="ignore"):
        keep = q <= r2                                   # NaN compares false
    js, q = js[keep], q[keep]
    order = np.lexsort((js, q))
    return js[order], q[order]


def plan_from(cands, eps=1e-8):
    """The per-query (j, q) lists -> (idx3 [M, 3] int32, w3 [M, 3] float32)."""
    M = len(cands)
    idx3 = np.full((M, 3), -1, dtype=np.int32)
    w3 = np.zeros((M, 3), dtype=f32)
    for i, (js, q) in enumerate(cands):
        n = min(len(js), 3)
        if n == 0:
            continue
        if n == 1 or q[0] == 0:
            idx3[i, 0], w3[i, 0] = js[0], 1
            continue
        with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
            a = (f32(1) / np.maximum(q[:n], f32(eps))).astype(f32)
            s = f32(a[0] + a[1])
            if n == 3:
                s = f32(s + a[2])
            w3[i, :n] = (a / s).astype(f32)
        idx3[i, :n] = js[:n]
    return idx3, w3


def plan(src, r, qry, pose=None, eps=1e-8, origin=None):
    return plan_from(candidates_grid(src, r, qry, pose, origin), eps)


# ------------------------------------------------------------------------------------------------ the inputs the tests share
POSE = np.array([[0.36, 0.48, -0.8, 0.01], [-0.8, 0.6, 0.0, -0.02], [0.48, 0.64, 0.6, 0.03]], dtype=f32)


def lattice_case():
    """seed 7: 901 sources on the 1/64 grid in 5^3 cells of 0.25 (empty cells, exact duplicates), 1543 queries on the 1/128 grid in [-1.5, 0.75), 200 of
    them copies of sources; r = 0.25.  Every coordinate and every difference is exact in fp32."""
    g = np.random.default_rng(7)
    cells = g.integers(0, 5, size=(40, 3))                                     # 40 of the 125 cells, some drawn twice: the others stay empty
    pick = cells[g.integers(0, len(cells), size=701)]
    src = (pick * 16 + g.integers(0, 16, size=(701, 3))).astype(f32) / f32(64) - f32(1)      # [-1, 0.25)
    src = np.concatenate([src, src[g.integers(0, 701, size=200)]], 0).astype(f32)            # exact duplicates
    qry = (g.integers(0, 288, size=(1543, 3)).astype(f32) / f32(128) - f32(1.5)).astype(f32)
    qry[g.choice(1543, 200, replace=False)] = src[g.integers(0, len(src), size=200)]
    return src, qry, 0.25


def uniform_case():
    g = np.random.default_rng(11)
    src = g.uniform(-1, 1, size=(20000, 3)).astype(f32)
    qry = g.uniform(-1.1, 1.1, size=(6007, 3)).astype(f32)
    return src, qry
