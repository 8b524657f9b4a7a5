"""Plain numpy reference of the interpolated scene masks, written from the definition in include/pointsam_hip.h and independent of the package.  The grid
is tests/scene_reference.py's.  All arithmetic is fp32 and every intermediate is cast to float32, so each operation is rounded on its own.

    candidates of scan point i   v = inv[i] and every nbr[v, o] in [0, Nw), o = 0 .. 25          (v outside [0, Nw): the point is OFF)
    distance                     q_r = (dx dx + dy dy) + dz dz, d = p - wxyz[r]
    selection                    the three lowest in (q, r), lexicographic; missing entries idx = -1, w = 0
    exact hit                    q_0 == 0 or one candidate: idx3 = (r0, -1, -1), w3 = (1, 0, 0)
    otherwise                    a_j = 1 / max(q_j, eps); s = a0 + a1 (+ a2); w_j = a_j / s
    apply                        off: fill; idx_1 unused: the word src[r, idx_0] copied; else acc = w0 l0 + w1 l1 (+ w2 l2)
"""
import numpy as np

import scene_reference as R

f32 = np.float32
NO_RANK = np.iinfo(np.int32).max
OFFSETS = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]      # dz slowest, the centre skipped


def neighbors(rep_xyz, h, origin=(-1.0, -1.0, -1.0)):
    """rep_xyz [V, 3]: one point per occupied voxel, in rank order -> nbr [V, 26] int32: the rank of the occupied voxel at the cell + offset, or -1."""
    c, bad = R.cells(rep_xyz, h, origin)
    assert not bad.any()
    c = c.astype(np.int64)
    rank = {tuple(cell): v for v, cell in enumerate(c.tolist())}
    assert len(rank) == len(c), "two representatives share a voxel"
    nbr = np.full((len(c), 26), -1, dtype=np.int32)
    for v, (x, y, z) in enumerate(c.tolist()):
        for o, (dz, dy, dx) in enumerate(OFFSETS):
            nbr[v, o] = rank.get((x + dx, y + dy, z + dz), -1)
    return nbr


def crop_coordinate(xyz, center, radius):
    """The crop's normalised coordinate: u = clamp((x - c) * fl32(1 / r), -1, 1) per axis, each operation rounded to fp32."""
    inv_r = f32(1) / f32(radius)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (np.asarray(xyz, dtype=f32) - np.asarray(center, dtype=f32)[None]).astype(f32)
        return np.minimum(np.maximum((d * inv_r).astype(f32), f32(-1)), f32(1)).astype(f32)


def plan(p, inv, wxyz, nbr, eps=1e-8):
    """p [M, 3] the query coordinates, inv [M], wxyz [Nw, 3], nbr [Nw, 26] -> (idx3 [M, 3] int32, w3 [M, 3] float32)."""
    p, wxyz, inv, nbr = np.asarray(p, dtype=f32), np.asarray(wxyz, dtype=f32), np.asarray(inv, dtype=np.int64), np.asarray(nbr, dtype=np.int64)
    M, Nw = len(p), len(wxyz)
    on = (inv >= 0) & (inv < Nw)
    v = np.where(on, inv, 0)
    cand = np.concatenate([v[:, None], nbr[v]], 1)                                   # [M, 27]
    ok = (cand >= 0) & (cand < Nw)
    safe = np.where(ok, cand, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (p[:, None, :] - wxyz[safe]).astype(f32)
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        q = (((dx * dx).astype(f32) + (dy * dy).astype(f32)).astype(f32) + (dz * dz).astype(f32)).astype(f32)
    q = np.where(ok, q, f32(np.inf)).astype(f32)
    r = np.where(ok, cand, NO_RANK)
    order = np.lexsort((r, q), axis=-1)[:, :3]                                       # by q, ties by r
    q3, r3 = np.take_along_axis(q, order, 1), np.take_along_axis(r, order, 1)
    count = ok.sum(1)
    copy = (q3[:, 0] == 0) | (count == 1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a = (f32(1) / np.maximum(q3, f32(eps))).astype(f32)
        s = (a[:, 0] + a[:, 1]).astype(f32)
        s = np.where(count >= 3, (s + a[:, 2]).astype(f32), s).astype(f32)
        w = (a / s[:, None]).astype(f32)
    used = np.arange(3)[None, :] < np.minimum(count, 3)[:, None]
    used &= ~copy[:, None] | (np.arange(3)[None, :] == 0)
    idx3 = np.where(used, r3, -1).astype(np.int32)
    w3 = np.where(used, w, f32(0)).astype(f32)
    w3[copy, 0] = 1
    idx3[~on], w3[~on] = -1, 0
    return idx3, w3


def apply_rows(src, idx3, w3, fill=0.0):
    """src [R, Nw] float32 -> [R, M] float32.  An idx3 entry outside [0, Nw) is unused; entries are used in order."""
    src = np.ascontiguousarray(src, dtype=f32)
    Nw = src.shape[1]
    ok = (idx3 >= 0) & (idx3 < Nw)
    ok0, ok1 = ok[:, 0], ok[:, 0] & ok[:, 1]
    ok2 = ok1 & ok[:, 2]
    j = np.where(ok, idx3, 0)
    l0, l1, l2 = src[:, j[:, 0]], src[:, j[:, 1]], src[:, j[:, 2]]
    with np.errstate(invalid="ignore", over="ignore"):
        acc = ((w3[None, :, 0] * l0).astype(f32) + (w3[None, :, 1] * l1).astype(f32)).astype(f32)
        acc = np.where(ok2[None], (acc + (w3[None, :, 2] * l2).astype(f32)).astype(f32), acc).astype(f32)
    out = np.where(ok1[None], acc.view(np.uint32), l0.view(np.uint32))               # one source: its word, untouched
    out = np.where(ok0[None], out, np.asarray(fill, dtype=f32).view(np.uint32))
    return np.ascontiguousarray(out.astype(np.uint32)).view(f32)


def blended(idx3, Nw):
    """[M] bool: the points whose value is computed (two or three sources), not copied or filled."""
    ok = (idx3 >= 0) & (idx3 < Nw)
    return ok[:, 0] & ok[:, 1]


def apply_bits(src, idx3, w3, thr=0.0):
    """-> (words [K, ceil(M / 64)] uint64, area [K] int32): value > thr in fp32, NaN false, an off point 0."""
    Nw = np.asarray(src).shape[1]
    val = apply_rows(src, idx3, w3, 0.0)
    on = (idx3[:, 0] >= 0) & (idx3[:, 0] < Nw)
    with np.errstate(invalid="ignore"):
        m = (val > f32(thr)) & on[None]
    return R.words(m), m.sum(1).astype(np.int32)
