"""The scan map's definition (include/pointsam_hip.h, "scan map") in plain numpy, every operation rounded on its own.

Two forms of one definition: `RefMap`, a dictionary walked point by point, IS the definition; `FastMap` does the same with np.unique for the one
large case.  tests/test_scanmap_cpu.py holds them equal.  Neither touches the library.
"""
import numpy as np

F = np.float32
AXIS_BITS = 21
INT32_MAX = 2 ** 31 - 1


class RefOverflow(RuntimeError):
    pass


def inv_h_of(voxel_size):
    return F(1) / F(voxel_size)


def pose_words(pose):
    """3 x 4 or 4 x 4 -> twelve fp32 words, None stays None."""
    if pose is None:
        return None
    return np.asarray(pose, dtype=np.float64)[:3, :].astype(F).reshape(12)


def posed(xyz, words):
    """p_a = ((P[a][0] x + P[a][1] y) + P[a][2] z) + P[a][3] in fp32, one rounding per operation; no arithmetic without a pose."""
    xyz = np.ascontiguousarray(xyz, dtype=F)
    if words is None:
        return xyz.copy()
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    out = np.empty_like(xyz)
    with np.errstate(all="ignore"):
        for a in range(3):
            w = words[4 * a:4 * a + 4]
            out[:, a] = ((w[0] * x + w[1] * y) + w[2] * z) + w[3]
    return out


def cells(p, inv_h):
    """-> (cell [M, 3] int64, ok [M, 3]): floorf((p - (-1)) * inv_h) in fp32, in [0, 2^21); a NaN has no cell."""
    with np.errstate(all="ignore"):
        c = np.floor((p - F(-1)) * F(inv_h))
        ok = (c >= 0) & (c < F(1 << AXIS_BITS))
    return np.where(ok, c, 0).astype(np.int64), ok


def fixed(v):
    """-> (q int64, ok): floor((double)v * 2^20) + 2^20 for v in [-1, 1]."""
    with np.errstate(all="ignore"):
        ok = (v >= F(-1)) & (v <= F(1))
        q = np.floor(np.where(ok, v, 0).astype(np.float64) * 1048576.0).astype(np.int64) + (1 << 20)
    return q, ok


def point_terms(xyz, rgb, pose, inv_h):
    """-> (accepted [M] bool, key [M] int64, q [M, 3] int64, c [M, 3] int64); rgb None = a locate: positions only."""
    p = posed(xyz, pose_words(pose))
    cell, cell_ok = cells(p, inv_h)
    q, q_ok = fixed(p)
    ok = cell_ok.all(1) & q_ok.all(1)
    c = np.zeros_like(q)
    if rgb is not None:
        c, c_ok = fixed(np.ascontiguousarray(rgb, dtype=F))
        ok &= c_ok.all(1)
    key = cell[:, 0] | (cell[:, 1] << AXIS_BITS) | (cell[:, 2] << (2 * AXIS_BITS))
    return ok, key, q, c


def mean(total, count):
    """fl32(fl64(fl64(sum) / fl64(count)) * 2^-20 - 1)"""
    return F(np.float64(total) / np.float64(count) * np.float64(2.0 ** -20) - np.float64(1.0))


def boundary_case():
    """(xyz [n, 3], rgb [n, 3], accepted [n] bool): values at exactly -1 and 1 (accepted), one ulp past them, NaN and both infinities in a position
    and in a colour (rejected), among plain points.  Shared by the CPU and the GPU test."""
    up, down = np.nextafter(F(1), F(2)), np.nextafter(F(-1), F(-2))
    rows = [((0.25, -0.5, 0.75), (0.1, 0.2, 0.3), True),
            ((1.0, -1.0, 1.0), (1.0, -1.0, 0.0), True),
            ((-1.0, -1.0, -1.0), (-1.0, -1.0, -1.0), True),
            ((up, 0.0, 0.0), (0.0, 0.0, 0.0), False),
            ((0.0, down, 0.0), (0.0, 0.0, 0.0), False),
            ((0.0, 0.0, 0.0), (0.0, up, 0.0), False),
            ((0.0, 0.0, 0.0), (0.0, 0.0, down), False),
            ((np.nan, 0.0, 0.0), (0.0, 0.0, 0.0), False),
            ((0.0, np.inf, 0.0), (0.0, 0.0, 0.0), False),
            ((0.0, 0.0, -np.inf), (0.0, 0.0, 0.0), False),
            ((0.0, 0.0, 0.0), (np.nan, 0.0, 0.0), False),
            ((0.0, 0.0, 0.0), (0.0, np.inf, 0.0), False),
            ((0.0, 0.0, 0.0), (0.0, 0.0, -np.inf), False),
            ((0.0, 0.0, 0.0), (0.5, 0.5, 0.5), True),
            ((-0.999, 0.999, 0.0), (-0.999, 0.999, 0.0), True)]
    return (np.array([r[0] for r in rows], dtype=F), np.array([r[1] for r in rows], dtype=F), np.array([r[2] for r in rows], dtype=bool))


def rotation_pose(ax_deg=20.0, ay_deg=-35.0, t=(0.05, -0.1, 0.02)):
    """A rotation about x then y plus a translation, 3 x 4 float64."""
    a, b = np.deg2rad(ax_deg), np.deg2rad(ay_deg)
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    return np.concatenate([Ry @ Rx, np.asarray(t, dtype=np.float64)[:, None]], axis=1)


class RefMap:
    """The definition, point by point."""

    def __init__(self, voxel_size, max_voxels, max_pairs=None):
        self.inv_h = inv_h_of(voxel_size)
        self.max_voxels, self.max_pairs = max_voxels, 2 * max_voxels if max_pairs is None else max_pairs
        self.clear()

    def clear(self):
        self.id_of = {}
        self.keys, self.count, self.sum_q, self.sum_c, self.first, self.last = [], [], [], [], [], []
        self.pairs = {}
        self.adds, self.dead = 0, False

    @property
    def V(self):
        return len(self.keys)

    def add(self, xyz, rgb, labels=None, pose=None):
        if self.dead:
            raise RefOverflow("dead")
        ok, key, q, c = point_terms(xyz, rgb, pose, self.inv_h)
        M = len(ok)
        labels = np.full(M, -1, dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
        # both overflow conditions are functions of the inputs alone: count before anything changes
        new_keys = {int(k) for k in key[ok]} - set(self.id_of)
        if self.V + len(new_keys) > self.max_voxels:
            self.dead = True
            raise RefOverflow("voxels")
        add_no = self.adds + 1
        ids = np.full(M, -1, dtype=np.int32)
        for i in range(M):
            if not ok[i]:
                continue
            k = int(key[i])
            v = self.id_of.get(k)
            if v is None:                  # new ids in the order of the lowest accepted point index
                v = self.id_of[k] = self.V
                self.keys.append(k); self.count.append(0); self.sum_q.append([0, 0, 0]); self.sum_c.append([0, 0, 0])
                self.first.append(add_no); self.last.append(add_no)
            ids[i] = v
            self.count[v] += 1
            for a in range(3):
                self.sum_q[v][a] += int(q[i, a])
                self.sum_c[v][a] += int(c[i, a])
            self.last[v] = add_no
            if labels[i] >= 0:
                self.pairs[(v, int(labels[i]))] = self.pairs.get((v, int(labels[i])), 0) + 1
        self.adds = add_no
        if len(self.pairs) > self.max_pairs:
            self.dead = True
            raise RefOverflow("pairs")
        return ids, len(new_keys), int(ok.sum()), int(M - ok.sum())

    def locate(self, xyz, pose=None):
        ok, key, _, _ = point_terms(xyz, None, pose, self.inv_h)
        return np.array([self.id_of.get(int(k), -1) if o else -1 for o, k in zip(ok, key)], dtype=np.int32)

    def labels(self, min_votes=1):
        label, votes = np.full(self.V, -1, dtype=np.int32), np.zeros(self.V, dtype=np.int32)
        best = {}
        for (v, l), n in self.pairs.items():
            if v not in best or (n, -l) > (best[v][0], -best[v][1]):      # the highest count, a tie to the LOWER label
                best[v] = (n, l)
        for v, (n, l) in best.items():
            if n >= min_votes:
                label[v], votes[v] = l, n
        return label, votes

    def cloud(self):
        xyz, rgb = np.empty((self.V, 3), dtype=F), np.empty((self.V, 3), dtype=F)
        for v in range(self.V):
            for a in range(3):
                xyz[v, a] = mean(self.sum_q[v][a], self.count[v])
                rgb[v, a] = mean(self.sum_c[v][a], self.count[v])
        return xyz, rgb

    def fields(self):
        """(count, first_seen, last_seen int32 [V], keys int64 [V], sum_q, sum_c int64 [V, 3])"""
        i32 = lambda a: np.asarray(a, dtype=np.int32).reshape(self.V)
        return (i32(self.count), i32(self.first), i32(self.last), np.asarray(self.keys, dtype=np.int64).reshape(self.V),
                np.asarray(self.sum_q, dtype=np.int64).reshape(self.V, 3), np.asarray(self.sum_c, dtype=np.int64).reshape(self.V, 3))

    def by_key(self):
        """{key: (count, sum_q, sum_c, first, last, {label: votes})}: the state that does not depend on the order of the points."""
        votes = {}
        for (v, l), n in self.pairs.items():
            votes.setdefault(v, {})[l] = n
        return {self.keys[v]: (self.count[v], tuple(self.sum_q[v]), tuple(self.sum_c[v]), self.first[v], self.last[v], votes.get(v, {}))
                for v in range(self.V)}


class FastMap:
    """The same map with np.unique; arrays instead of dictionaries."""

    def __init__(self, voxel_size, max_voxels, max_pairs=None):
        self.inv_h = inv_h_of(voxel_size)
        self.max_voxels, self.max_pairs = max_voxels, 2 * max_voxels if max_pairs is None else max_pairs
        self.keys = np.empty(0, dtype=np.int64)
        self.count = np.empty(0, dtype=np.int64)
        self.sum_q, self.sum_c = np.empty((0, 3), dtype=np.int64), np.empty((0, 3), dtype=np.int64)
        self.first, self.last = np.empty(0, dtype=np.int32), np.empty(0, dtype=np.int32)
        self.pair_keys, self.pair_count = np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64)      # (id << 32) | label, sorted
        self.adds, self.dead = 0, False

    @property
    def V(self):
        return len(self.keys)

    def _find(self, key):
        """ids [n] of keys, -1 where the map has none"""
        if self.V == 0:
            return np.full(len(key), -1, dtype=np.int64)
        order = np.argsort(self.keys, kind="stable")
        pos = np.clip(np.searchsorted(self.keys[order], key), 0, self.V - 1)
        return np.where(self.keys[order][pos] == key, order[pos], -1)

    def add(self, xyz, rgb, labels=None, pose=None):
        if self.dead:
            raise RefOverflow("dead")
        ok, key, q, c = point_terms(xyz, rgb, pose, self.inv_h)
        M = len(ok)
        labels = np.full(M, -1, dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
        idx = np.nonzero(ok)[0]
        uniq, first_at, inverse = np.unique(key[idx], return_index=True, return_inverse=True)      # first_at: the lowest accepted position per key
        have = self._find(uniq)
        fresh = np.nonzero(have < 0)[0]
        if self.V + len(fresh) > self.max_voxels:
            self.dead = True
            raise RefOverflow("voxels")
        add_no = self.adds + 1
        fresh = fresh[np.argsort(first_at[fresh], kind="stable")]
        have[fresh] = self.V + np.arange(len(fresh))
        n_new = len(fresh)
        self.keys = np.concatenate([self.keys, uniq[fresh]])
        self.count = np.concatenate([self.count, np.zeros(n_new, dtype=np.int64)])
        self.sum_q = np.concatenate([self.sum_q, np.zeros((n_new, 3), dtype=np.int64)])
        self.sum_c = np.concatenate([self.sum_c, np.zeros((n_new, 3), dtype=np.int64)])
        self.first = np.concatenate([self.first, np.full(n_new, add_no, dtype=np.int32)])
        self.last = np.concatenate([self.last, np.full(n_new, add_no, dtype=np.int32)])
        v = have[inverse.reshape(-1)]
        ids = np.full(M, -1, dtype=np.int32)
        ids[idx] = v
        # bincount sums in fp64: exact, every partial sum of an add stays below 2^28 * 2^21 < 2^53
        self.count += np.bincount(v, minlength=self.V)
        for a in range(3):
            self.sum_q[:, a] += np.bincount(v, weights=q[idx, a].astype(np.float64), minlength=self.V).astype(np.int64)
            self.sum_c[:, a] += np.bincount(v, weights=c[idx, a].astype(np.float64), minlength=self.V).astype(np.int64)
        self.last[v] = add_no
        lab = labels[idx]
        pk, pn = np.unique((v[lab >= 0] << 32) | lab[lab >= 0], return_counts=True)
        allk, inv = np.unique(np.concatenate([self.pair_keys, pk]), return_inverse=True)
        alln = np.zeros(len(allk), dtype=np.int64)
        np.add.at(alln, inv.reshape(-1), np.concatenate([self.pair_count, pn]))
        self.pair_keys, self.pair_count = allk, alln
        self.adds = add_no
        if len(allk) > self.max_pairs:
            self.dead = True
            raise RefOverflow("pairs")
        return ids, n_new, len(idx), M - len(idx)

    def locate(self, xyz, pose=None):
        ok, key, _, _ = point_terms(xyz, None, pose, self.inv_h)
        return np.where(ok, self._find(key), -1).astype(np.int32)

    def labels(self, min_votes=1):
        label, votes = np.full(self.V, -1, dtype=np.int32), np.zeros(self.V, dtype=np.int32)
        v, l, n = self.pair_keys >> 32, self.pair_keys & 0xffffffff, self.pair_count
        order = np.lexsort((l, -n, v))                 # per voxel: the highest count first, then the lower label
        v, l, n = v[order], l[order], n[order]
        head = np.ones(len(v), dtype=bool)
        head[1:] = v[1:] != v[:-1]
        take = head & (n >= min_votes)
        label[v[take]], votes[v[take]] = l[take], n[take]
        return label, votes

    def cloud(self):
        n = self.count.astype(np.float64)[:, None]
        f = lambda s: (s.astype(np.float64) / n * np.float64(2.0 ** -20) - np.float64(1.0)).astype(F)
        return f(self.sum_q), f(self.sum_c)

    def fields(self):
        return (self.count.astype(np.int32), self.first.copy(), self.last.copy(), self.keys.copy(), self.sum_q.copy(), self.sum_c.copy())
