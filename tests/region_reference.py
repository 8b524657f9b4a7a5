"""Plain numpy / scipy reference of the connected-component kernels, written from the definitions and independent of the package.

    cells       per axis c = floor((x - origin) * inv_h) in fp32, every operation rounded on its own, inv_h = fl32(1) / fl32(h), origin (-1, -1, -1)
                (tests/scene_reference.py)
    graph       points i and j are adjacent iff their cells differ by at most 1 on every axis
    rank        inv[i] of scene_reference.downsample: voxels ranked by their lowest point index
    components  of a point set S: those of the subgraph induced by S; id = the lowest inv[] among the members, size = the number of POINTS
    clean       (1) complement components below min_hole points join the mask, (2) components of the result below min_island points leave it, except
                the largest (size tie: lowest id), (3) if a seed is a member after (2), only the components holding such a seed stay.  An empty
                mask stays empty.
"""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

import scene_reference as SR

OFFSETS = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]      # dz slowest, centre skipped
AXIS_LIMIT = 1 << SR.AXIS_BITS


class Graph:
    """cells [V, 3] int64 (x, y, z) of the occupied voxels in rank order, keep_idx [V], inv [N], nbr [V, 26] int32, adj: scipy CSR [V, V]."""

    def __init__(self, xyz, h):
        xyz = np.asarray(xyz, dtype=np.float32)
        self.n_points = len(xyz)
        self.keep_idx, self.inv = SR.downsample(xyz, h)
        c, bad = SR.cells(xyz[self.keep_idx], h)
        assert not bad.any()
        self.cells = c.astype(np.int64)
        V = len(self.keep_idx)
        # key -> rank by a sorted table (a dict in effect: the keys of distinct voxels differ); one look-up per (voxel, offset)
        key = lambda c: c[:, 0] | (c[:, 1] << SR.AXIS_BITS) | (c[:, 2] << (2 * SR.AXIS_BITS))
        keys = key(self.cells)
        order = np.argsort(keys)
        self.nbr = np.full((V, 26), -1, dtype=np.int32)
        for o, (dz, dy, dx) in enumerate(OFFSETS):
            n = self.cells + np.array([dx, dy, dz], dtype=np.int64)
            ok = ((n >= 0) & (n < AXIS_LIMIT)).all(1)
            want = key(n)
            pos = np.minimum(np.searchsorted(keys[order], want), V - 1)
            hit = ok & (keys[order][pos] == want)
            self.nbr[hit, o] = order[pos][hit]
        rows, cols = np.nonzero(self.nbr >= 0)
        cols = self.nbr[rows, cols]
        self.adj = sp.csr_matrix((np.ones(len(rows), dtype=np.int8), (rows, cols)), shape=(V, V))


def components(g, member):
    """member [N] bool -> (labels [N] int32: the component's id per member point, -1 elsewhere; sizes {id: points})."""
    member = np.asarray(member, dtype=bool)
    labels = np.full(g.n_points, -1, dtype=np.int32)
    counts = np.bincount(g.inv[member], minlength=len(g.keep_idx))
    occ = np.flatnonzero(counts > 0)
    if len(occ) == 0:
        return labels, {}
    _, comp = connected_components(g.adj[occ][:, occ], directed=False)
    ids = np.full(comp.max() + 1, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(ids, comp, occ)                       # id = the lowest voxel rank = the lowest inv[] among the members
    vox_id = np.full(len(g.keep_idx), -1, dtype=np.int64)
    vox_id[occ] = ids[comp]
    labels[member] = vox_id[g.inv[member]]
    sizes = {}
    for v in occ:
        sizes[int(vox_id[v])] = sizes.get(int(vox_id[v]), 0) + int(counts[v])
    return labels, sizes


def clean_row(g, mask, min_island=0, min_hole=0, seeds=()):
    """mask [N] bool -> (mask [N] bool, trace): trace counts what each step did (the tests assert that their inputs exercise every branch)."""
    mask = np.asarray(mask, dtype=bool).copy()
    trace = dict(filled=0, removed=0, kept_small_largest=False, tie=False, seeded=False, seed_dropped=0)
    if not mask.any():
        return mask, trace
    if min_hole > 0:
        lab, sizes = components(g, ~mask)
        for cid, size in sizes.items():
            if size < min_hole:
                mask |= lab == cid
                trace["filled"] += 1
    lab, sizes = components(g, mask)
    if min_island > 0:
        top = max(sizes.values())
        largest = min(cid for cid, size in sizes.items() if size == top)
        trace["tie"] = sum(1 for size in sizes.values() if size == top) > 1
        trace["kept_small_largest"] = top < min_island
        for cid, size in sizes.items():
            if size < min_island and cid != largest:
                mask &= lab != cid
                trace["removed"] += 1
    hit = sorted({int(lab[s]) for s in seeds if 0 <= s < g.n_points and mask[s]})
    if hit:
        trace["seeded"] = True
        trace["seed_dropped"] = len({int(c) for c in lab[mask]}) - len(hit)
        mask &= np.isin(lab, hit)
    return mask, trace


def clean(g, masks, min_island=0, min_hole=0, select=None, seeds=None):
    """masks [K, N] bool, select [K] or None, seeds [K, S] int or None -> (masks [K, N] bool, area [K] int32, changed [K] uint8, traces)."""
    masks = np.asarray(masks, dtype=bool)
    out = masks.copy()
    traces = []
    for k in range(len(masks)):
        if select is not None and not select[k]:
            traces.append(None)
            continue
        out[k], t = clean_row(g, masks[k], min_island, min_hole, () if seeds is None else [int(s) for s in seeds[k]])
        traces.append(t)
    return out, out.sum(1).astype(np.int32), (out != masks).any(1).astype(np.uint8), traces
