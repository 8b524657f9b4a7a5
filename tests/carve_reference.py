"""Scan map carving's definition (include/pointsam_hip.h, "scan map carving") in plain Python and numpy, on top of scanmap_reference.RefMap's cells and
pose.  `walk` IS the definition of a ray's cells; `geometric` states the same set with exact rationals (the open boxes the segment between the two
centres meets); `entry` is the closed form that starts a walk in the middle of a ray.  `RefCarve` keeps the four words per map voxel id.  Nothing here
touches the library.
"""
from fractions import Fraction

import numpy as np

import scanmap_reference as SM

F = np.float32
MASK = (1 << SM.AXIS_BITS) - 1


def cell_of_key(key):
    key = int(key)
    return (key & MASK, (key >> SM.AXIS_BITS) & MASK, key >> (2 * SM.AXIS_BITS))


def key_of_cell(c):
    return int(c[0]) | (int(c[1]) << SM.AXIS_BITS) | (int(c[2]) << (2 * SM.AXIS_BITS))


def _sign(d):
    return (d > 0) - (d < 0)


def walk(o, e, k=None):
    """The crossed cells of the ray from cell o to cell e, in order, o and e excluded.  k: the crossings per axis already made (entry's), the walk
    then goes on from there."""
    n = [abs(e[a] - o[a]) for a in range(3)]
    s = [_sign(e[a] - o[a]) for a in range(3)]
    k = [0, 0, 0] if k is None else list(k)
    cur = [o[a] + s[a] * k[a] for a in range(3)]
    out = []
    while tuple(cur) != tuple(e):
        live = [a for a in range(3) if k[a] < n[a]]
        best = live[0]
        for a in live[1:]:
            if (2 * k[a] + 1) * n[best] < (2 * k[best] + 1) * n[a]:
                best = a
        tied = [a for a in live if (2 * k[a] + 1) * n[best] == (2 * k[best] + 1) * n[a]]
        for a in tied:
            k[a] += 1
            cur[a] += s[a]
        if tuple(cur) != tuple(e):
            out.append(tuple(cur))
    return out


def walk_by_differences(o, e, margin=None):
    """csrc/carve.hip's form of the same walk: the three differences D_ab = (2 k_a + 1) n_b - (2 k_b + 1) n_a are kept by additions, an axis steps
    where it is <= both others, and nothing tests whether an axis still has crossings left.  margin: stop where the Chebyshev distance to e first is
    <= margin, as the kernel does (None: walk to the end)."""
    n = [abs(e[a] - o[a]) for a in range(3)]
    s = [_sign(e[a] - o[a]) if e[a] != o[a] else 1 for a in range(3)]
    r = list(n)
    D01, D02, D12 = n[1] - n[0], n[2] - n[0], n[2] - n[1]
    cur, out = list(o), []
    for _ in range(sum(n)):
        t0, t1, t2 = D01 <= 0 and D02 <= 0, D01 >= 0 and D12 <= 0, D02 >= 0 and D12 >= 0
        for a, t in enumerate((t0, t1, t2)):
            cur[a] += s[a] * t
            r[a] -= t
        D01 += 2 * n[1] * t0 - 2 * n[0] * t1
        D02 += 2 * n[2] * t0 - 2 * n[0] * t2
        D12 += 2 * n[2] * t1 - 2 * n[1] * t2
        if max(r) <= (0 if margin is None else margin):
            break
        out.append(tuple(cur))
    return out


def entry(o, e, k):
    """The crossings per axis right after the k-th crossing of the longest axis a (the lowest such axis), 1 <= k <= n_a, at t = (2 k - 1) / (2 n_a):
    axis b has made the crossings (2 j + 1) / (2 n_b) <= t, ties included because tied axes step together.  (Counting the crossings of a from 0,
    the numerator reads (2 k + 1) n_b + n_a.)"""
    n = [abs(e[a] - o[a]) for a in range(3)]
    a = n.index(max(n))
    assert 1 <= k <= n[a]
    return [k if b == a else min(n[b], ((2 * k - 1) * n[b] + n[a]) // (2 * n[a])) for b in range(3)]


def geometric(o, e):
    """The cells c != o, e whose OPEN box meets the segment between the centres of o and e, as a set; exact rationals."""
    if tuple(o) == tuple(e):
        return set()
    d = [e[a] - o[a] for a in range(3)]
    half = Fraction(1, 2)
    out = set()
    box = [range(min(o[a], e[a]), max(o[a], e[a]) + 1) for a in range(3)]
    for cx in box[0]:
        for cy in box[1]:
            for cz in box[2]:
                c = (cx, cy, cz)
                if c == tuple(o) or c == tuple(e):
                    continue
                lo, hi = Fraction(0), Fraction(1)          # the closed parameter range of the segment
                inside = True
                for a in range(3):
                    if d[a] == 0:
                        inside &= c[a] == o[a]             # |o_a - c_a| < 1/2 over integers
                        continue
                    t0, t1 = (c[a] - o[a] - half) / d[a], (c[a] - o[a] + half) / d[a]
                    lo, hi = max(lo, min(t0, t1)), min(hi, max(t0, t1))
                # the open intervals' intersection (lo, hi) is non-empty iff lo < hi; lo >= 0 and hi <= 1 already, so it lies on the segment
                if inside and lo < hi:
                    out.add(c)
    return out


def chebyshev(a, b):
    return max(abs(a[i] - b[i]) for i in range(3))


def origin_cell(origin, pose, inv_h):
    """The origin's cell under the pose, or None: a map point's arithmetic and acceptance test."""
    ok, key, _, _ = SM.point_terms(np.asarray(origin, dtype=F).reshape(1, 3), None, pose, inv_h)
    return cell_of_key(key[0]) if ok[0] else None


class RefCarve:
    """The carve block over a RefMap (or anything with inv_h, id_of {key: id}, V and dead)."""

    def __init__(self, ref):
        self.ref = ref
        self.clear()

    def clear(self):
        self.hits, self.misses, self.last_hit, self.last_missed = {}, {}, {}, {}
        self.carves, self.stamp = 0, 0

    def carve(self, xyz, origin, pose=None, margin=1, stamp=None):
        """-> (rays, accepted, rejected, hit_voxels, missed_voxels, crossed, origin_has_cell); stamp None = carves so far + 1."""
        ref = self.ref
        stamp = self.carves + 1 if stamp is None else stamp
        ok, key, _, _ = SM.point_terms(xyz, None, pose, ref.inv_h)
        ends = sorted({int(k) for k in key[ok]})
        o = origin_cell(origin, pose, ref.inv_h)
        if stamp > self.stamp:
            self.stamp, self.carves = stamp, self.carves + 1
        hit = missed = crossed = rays = 0
        if not ref.dead:
            for k in ends:
                v = ref.id_of.get(k)
                if v is not None and self.last_hit.get(v, 0) < stamp:
                    self.hits[v] = self.hits.get(v, 0) + 1
                    self.last_hit[v] = stamp
                    hit += 1
        for k in ends:
            e = cell_of_key(k)
            if o is None or e == o:
                continue
            rays += 1
            if ref.dead:
                continue
            for c in walk(o, e):
                if chebyshev(c, e) <= margin:
                    continue
                crossed += 1
                v = ref.id_of.get(key_of_cell(c))
                if v is None or self.last_hit.get(v, 0) == stamp:
                    continue
                if self.last_missed.get(v, 0) < stamp:
                    self.misses[v] = self.misses.get(v, 0) + 1
                    self.last_missed[v] = stamp
                    missed += 1
        return rays, int(ok.sum()), int(len(ok) - ok.sum()), hit, missed, crossed, int(o is not None)

    def fields(self, V=None):
        """(hits, misses, last_hit, last_missed), each int32 [V]"""
        V = self.ref.V if V is None else V
        return tuple(np.array([d.get(v, 0) for v in range(V)], dtype=np.int32).reshape(V) for d in (self.hits, self.misses, self.last_hit, self.last_missed))


def occupied(hits, misses, min_misses=2, num=1, den=1):
    h, m = hits.astype(np.int64), misses.astype(np.int64)
    return ~((m >= min_misses) & (m * den > h * num))
