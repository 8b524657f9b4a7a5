"""Normals, superpoints and mask snapping in plain numpy and Python integers, written from include/pointsam_hip.h and independent of the package.

    fixed point   q = floor((double)p * 2^20) + 2^20 per coordinate, an integer in [0, 2^21]; a point with a coordinate that is not finite or outside
                  [-1, 1] takes part in no neighbourhood
    scatter       over the points of voxel v and of nbr[v, 0 .. 25]: n, s = sum q, P = sum q q^T, S = n P - s s^T in Python integers (exact)
    normal        numpy.linalg.eigh of float(S): the eigenvector of the smallest eigenvalue, rounded to fp32, sign decided on the fp32 values;
                  curvature l0 / (l0 + l1 + l2) with l0 not below 0; n < min_points gives (0, 0, 0) and 0
    join          both ends have count >= min_points and curvature <= max_curvature, and |(x x' + y y') + z z'| >= cos_angle in fp64 from the fp32 normals
    union         a host union-find over the joining edges; label = the lowest voxel rank of the component, size in points
    absorb        per round, from the labels and sizes of its start: a voxel of a label below min_size takes the label of the neighbour (in a label of at
                  least min_size) with the largest |n . n'|, ties to the lower label
    compact       labels in use -> 0 .. S - 1 in increasing order of their value
    snap          bit i of row k iff label[i] >= 0 and cnt[k, label[i]] * 65536 > q16 * size[label[i]]
"""
import math

import numpy as np

ONE = 1 << 20


def fixed(xyz):
    """xyz [N, 3] f32 -> (q [N, 3] int64, ok [N] bool)."""
    xyz = np.asarray(xyz, dtype=np.float32)
    ok = np.all((xyz >= -1) & (xyz <= 1), axis=1)                  # NaN compares false
    q = np.zeros(xyz.shape, dtype=np.int64)
    q[ok] = np.floor(xyz[ok].astype(np.float64) * float(ONE)).astype(np.int64) + ONE
    return q, ok


PAIRS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def scatter(xyz, inv, nbr):
    """-> (count [V] int64, s [V, 3] int64, S: V rows of six Python integers xx, xy, xz, yy, yz, zz), over every voxel's neighbourhood."""
    q, ok = fixed(xyz)
    inv, nbr = np.asarray(inv), np.asarray(nbr)
    V = len(nbr)
    ok &= (inv >= 0) & (inv < V)
    assert len(q) < (1 << 21), "the int64 tables below hold N * 2^42"
    own = np.zeros((V, 10), dtype=np.int64)
    np.add.at(own[:, 0], inv[ok], 1)
    for a in range(3):
        np.add.at(own[:, 1 + a], inv[ok], q[ok, a])
    for c, (a, b) in enumerate(PAIRS):
        np.add.at(own[:, 4 + c], inv[ok], q[ok, a] * q[ok, b])
    tot = own.copy()
    for o in range(26):
        u = nbr[:, o]
        hit = u >= 0
        tot[hit] += own[u[hit]]
    S = []
    for row in tot.tolist():                                       # Python integers from here on
        n, s = row[0], row[1:4]
        S.append([n * row[4 + c] - s[a] * s[b] for c, (a, b) in enumerate(PAIRS)])
    return tot[:, 0].copy(), tot[:, 1:4].copy(), S


def scatter_float(S):
    """The exact integers rounded to fp64 once, to nearest even: [V, 6]."""
    return np.array([[float(x) for x in row] for row in S], dtype=np.float64).reshape(len(S), 6)


def _sign_default(n32):
    a = np.abs(n32)
    lead = 0 if (a[0] >= a[1] and a[0] >= a[2]) else (1 if a[1] >= a[2] else 2)
    return -n32 if n32[lead] < 0 else n32


def eigen(count, S, min_points=5):
    """numpy.linalg.eigh of float(S) per voxel with count >= min_points -> (vec [V, 3] f64: the unit eigenvector of the smallest eigenvalue, sign
    as eigh left it; curvature [V] f64; lam [V, 3] f64 ascending), zeros elsewhere."""
    V = len(S)
    Sf = scatter_float(S)
    vec, curv, lam = np.zeros((V, 3)), np.zeros(V), np.zeros((V, 3))
    for v in range(V):
        if count[v] < min_points or count[v] == 0:
            continue
        xx, xy, xz, yy, yz, zz = Sf[v]
        w, e = np.linalg.eigh(np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]))
        lam[v], vec[v] = w, e[:, 0]
        total = w[0] + w[1] + w[2]
        curv[v] = max(w[0], 0.0) / total if total > 0 else 0.0
    return vec, curv, lam


def normals(count, s, S, min_points=5, viewpoint=None):
    """-> (normal [V, 3] f32, curvature [V] f32, lam [V, 3] f64 ascending eigenvalues (0 where invalid), facing [V] f64: |n . (viewpoint - mean)|
    relative to |viewpoint - mean| (0 without a viewpoint))."""
    V = len(S)
    vec, curv64, lam = eigen(count, S, min_points)
    normal = np.zeros((V, 3), dtype=np.float32)
    facing = np.zeros(V)
    for v in range(V):
        if count[v] < min_points or count[v] == 0:
            continue
        n32 = vec[v].astype(np.float32)
        if viewpoint is None:
            n32 = _sign_default(n32)
        else:
            mean = (s[v].astype(np.float64) / float(count[v]) - float(ONE)) / float(ONE)
            d = np.asarray(viewpoint, dtype=np.float32).astype(np.float64) - mean
            dot = float(n32.astype(np.float64) @ d)
            facing[v] = abs(dot) / max(np.linalg.norm(d), 1e-300)
            if dot < 0:
                n32 = -n32
        normal[v] = n32
    return normal, curv64.astype(np.float32), lam, facing


def dots(normal, v, u):
    """|n_v . n_u| as the contract writes it: fp64 products of the fp32 values, added left to right."""
    a, b = normal[v].astype(np.float64), normal[u].astype(np.float64)
    return np.abs((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2])


def cos_of(angle_deg):
    return math.cos(math.radians(angle_deg))


def union(nbr, count, normal, curvature, cos_angle, max_curvature, min_points):
    """-> label [V] int64: the lowest voxel rank of every voxel's component."""
    nbr = np.asarray(nbr)
    V = len(nbr)
    smooth = (np.asarray(count) >= min_points) & (np.asarray(curvature, dtype=np.float32) <= np.float32(max_curvature))
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for o in range(13):
        u = nbr[:, o].astype(np.int64)
        v = np.flatnonzero((u >= 0) & smooth & smooth[np.maximum(u, 0)])
        v = v[dots(normal, v, u[v]) >= cos_angle]
        for a, b in zip(v.tolist(), u[v].tolist()):
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(v) for v in range(V)], dtype=np.int64)


def sizes_of(label, own):
    size = np.zeros(len(label), dtype=np.int64)
    np.add.at(size, label, own)
    return size


def absorb_round(nbr, label, size, normal, min_size):
    nbr = np.asarray(nbr)
    out = label.copy()
    small = np.flatnonzero(size[label] < min_size)
    if len(small) == 0:
        return out
    u = nbr[small].astype(np.int64)                                # [m, 26]
    lab = label[np.maximum(u, 0)]
    ok = (u >= 0) & (size[lab] >= min_size)
    d = np.where(ok, dots(normal, small[:, None], np.maximum(u, 0)), -1.0)
    best = d.max(1)
    winner = np.where(ok & (d == best[:, None]), lab, np.iinfo(np.int64).max).min(1)      # the largest product; among equals the lowest label
    out[small] = np.where(best >= 0, winner, label[small])
    return out


def superpoints(inv, nbr, count, normal, curvature, cos_angle, max_curvature, min_points=5, min_size=0, absorb_rounds=2):
    """-> (voxel_label [V] int32, point_label [N] int32, size [S] int32, S)."""
    inv, nbr = np.asarray(inv), np.asarray(nbr)
    V = len(nbr)
    has_cell = (inv >= 0) & (inv < V)
    own = np.bincount(inv[has_cell], minlength=V).astype(np.int64)
    label = union(nbr, count, normal, curvature, cos_angle, max_curvature, min_points)
    size = sizes_of(label, own)
    for _ in range(absorb_rounds if min_size > 0 else 0):
        label = absorb_round(nbr, label, size, normal, min_size)
        size = sizes_of(label, own)
    used = np.unique(label)                                        # increasing
    new_id = np.full(V, -1, dtype=np.int64)
    new_id[used] = np.arange(len(used))
    voxel_label = new_id[label].astype(np.int32)
    point_label = np.full(len(inv), -1, dtype=np.int32)
    point_label[has_cell] = voxel_label[inv[has_cell]]
    return voxel_label, point_label, size[used].astype(np.int32), len(used)


def partition(labels):
    """The partition a label array describes, whatever the ids: per element the lowest index that shares its label (-1 stays -1)."""
    labels = np.asarray(labels)
    first = {}
    out = np.empty(len(labels), dtype=np.int64)
    for i, l in enumerate(labels.tolist()):
        out[i] = -1 if l < 0 else first.setdefault(l, i)
    return out


def snap(masks, point_label, size, q16):
    """masks [K, N] bool -> (out [K, N] bool, area [K], changed [K])."""
    masks = np.asarray(masks, dtype=bool)
    point_label, size = np.asarray(point_label, dtype=np.int64), np.asarray(size, dtype=np.int64)
    S = len(size)
    has = (point_label >= 0) & (point_label < S)
    out = np.zeros_like(masks)
    for k in range(len(masks)):
        cnt = np.bincount(point_label[has & masks[k]], minlength=S).astype(np.int64)
        out[k, has] = (cnt * 65536 > int(q16) * size)[point_label[has]]
    return out, out.sum(1).astype(np.int32), (out != masks).any(1).astype(np.uint8)
