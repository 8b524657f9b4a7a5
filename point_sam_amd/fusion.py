"""Multi-view label fusion: the 2-D segmentations of many views of one cloud -- the frames of a ``views.FrameSet``, or rendered ``views.View``s of one
size -- become ONE 3-D instance labelling of the cloud (``predictor.fuse_labels``).  The definition is in include/pointsam_hip.h ("label fusion"), the
kernels are csrc/fusion.hip.

Region ids of different views do not correspond.  Every (view, region) is lifted to a packed row of the points visible with that label
(``ops.fuse_region_bits``); two regions of different views are LINKED when, among the points BOTH views see, they cover each other:
with n the points they share, ca the points of a that b's view sees at all and cb likewise, min(ca, cb) >= min_points and n >= overlap * max(ca, cb).
Only co-visible points count on purpose: two frames see different sides of an object, so an intersection over the smaller AREA stays small between the
same object's regions.  The instances are the connected components of the links; every point then votes over its observations' instances
(``ops.fuse_vote``).
"""
import dataclasses

import numpy as np
import torch

from . import ops


@dataclasses.dataclass(frozen=True)
class FusionConfig:
    """tau: how far behind its pixel's winner a point may lie and still be visible (ops.view_lift_bits' tau, in the cloud's units); overlap in (0, 1]:
    the co-visible containment two regions need in both directions to be linked; min_points >= 1: the co-visible points both must have for a link to be
    considered at all; min_votes >= 1: the votes a point's winner needs; max_regions: the most (view, region) rows one call may make.
    NONE of the defaults has been tuned on real data: they are the values the synthetic ring fixture of the tests was measured with."""
    tau: float
    overlap: float = 0.5
    min_points: int = 20
    min_votes: int = 1
    max_regions: int = 8192

    def __post_init__(self):
        def number(v):
            return not isinstance(v, bool) and isinstance(v, (int, float))

        def integer(v, lo, hi):
            return not isinstance(v, bool) and isinstance(v, int) and lo <= v <= hi
        if not number(self.tau) or not self.tau >= 0:
            raise ValueError(f"FusionConfig: tau must be a number >= 0, got {self.tau!r}")
        if not number(self.overlap) or not 0 < self.overlap <= 1:
            raise ValueError(f"FusionConfig: overlap must lie in (0, 1], got {self.overlap!r}")
        if not integer(self.min_points, 1, 1 << 28):
            raise ValueError(f"FusionConfig: min_points must be an integer in 1 .. 2^28, got {self.min_points!r}")
        if not integer(self.min_votes, 1, ops.FUSE_MAX_VIEWS):
            raise ValueError(f"FusionConfig: min_votes must be an integer in 1 .. {ops.FUSE_MAX_VIEWS}, got {self.min_votes!r}")
        if not integer(self.max_regions, 1, ops.FUSE_MAX_ROWS):
            raise ValueError(f"FusionConfig: max_regions must be an integer in 1 .. {ops.FUSE_MAX_ROWS}, got {self.max_regions!r}")

    @classmethod
    def from_overrides(cls, data: dict) -> "FusionConfig":
        """A config from a dict of fields (a request's body): an unknown field is a ValueError, like a bad value."""
        names = {f.name for f in dataclasses.fields(cls)}
        if not isinstance(data, dict) or set(data) - names or "tau" not in data:
            raise ValueError(f"FusionConfig takes tau and optionally {sorted(names - {'tau'})}, got {sorted(data) if isinstance(data, dict) else data!r}")
        return cls(**data)


def _row_base(row_base) -> np.ndarray:
    rb = np.asarray(row_base.detach().cpu().numpy() if isinstance(row_base, torch.Tensor) else row_base)
    if rb.ndim != 1 or rb.size < 2 or rb.dtype.kind not in "iu" or rb[0] != 0 or (np.diff(rb.astype(np.int64)) < 0).any():
        raise ValueError(f"link_regions: row_base must be V + 1 integers starting at 0 that never decrease, got {row_base!r}")
    return rb.astype(np.int64)


def link_edges(inter, row_base, cfg: FusionConfig) -> np.ndarray:
    """inter [R + V, R + V] int32 (ops.mask_intersections of fuse_region_bits' rows with themselves; a tensor on any device, or an array) ->
    the links [E, 2] int64 on the host, a < b.  The products and compares are in fp64 where the tensor lives; the edge list is the one host read."""
    rb = _row_base(row_base)
    V, R = rb.size - 1, int(rb[-1])
    inter = torch.as_tensor(inter)
    if inter.dim() != 2 or tuple(inter.shape) != (R + V, R + V) or inter.dtype != torch.int32:
        raise ValueError(f"link_regions: inter must be int32 [{R + V}, {R + V}] for {R} regions of {V} views, got {inter.dtype} {tuple(inter.shape)}")
    if R == 0:
        return np.zeros((0, 2), dtype=np.int64)
    view_of = torch.from_numpy(np.repeat(np.arange(V), np.diff(rb))).to(inter.device)
    n = inter[:R, :R]
    ca = inter[:R, R:].index_select(1, view_of)                    # ca[a, b]: the points of a that b's view sees at all
    cb = ca.t()                                                    # cb[a, b]: the points of b that a's view sees
    area = torch.diagonal(n)
    link = (view_of[:, None] < view_of[None, :]) & (area[:, None] > 0) & (area[None, :] > 0)      # regions are in view order: u < v is a < b
    link &= torch.minimum(ca, cb) >= cfg.min_points
    link &= n.double() >= cfg.overlap * torch.maximum(ca, cb).double()
    return torch.nonzero(link).cpu().numpy().astype(np.int64)


def components(nonempty, edges) -> np.ndarray:
    """nonempty [R] bool, edges [E, 2] -> remap [R] int32: the connected components of the edges over the non-empty regions, numbered by their smallest
    row in ascending order; -1 for an empty region.  A union-find whose root is always the smallest row: the answer does not depend on the edge order."""
    nonempty = np.asarray(nonempty, dtype=bool)
    parent = list(range(len(nonempty)))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a, b in np.asarray(edges, dtype=np.int64).reshape(-1, 2).tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    roots = np.array([find(r) for r in range(len(parent))], dtype=np.int64)
    remap = np.full(len(parent), -1, dtype=np.int32)
    if nonempty.any():
        _, number = np.unique(roots[nonempty], return_inverse=True)      # ascending roots = ascending smallest rows
        remap[nonempty] = number.astype(np.int32)
    return remap


def link_regions(inter, row_base, cfg: FusionConfig) -> np.ndarray:
    """-> remap [R] int32 on the host: the global instance of every (view, region) row, -1 for an empty region (link_edges, then components)."""
    edges = link_edges(inter, row_base, cfg)
    R = int(_row_base(row_base)[-1])
    area = torch.diagonal(torch.as_tensor(inter))[:R].cpu().numpy()
    return components(area > 0, edges)


class Fused:
    """The fused labelling: ``labels`` [N] int32, per point of the cloud its instance or -1; ``votes`` the winner's count; ``seen`` / ``labelled`` /
    ``dropped`` the point's visible, labelled and refused observations (a point sees at most 8 distinct instances); ``num_instances``; ``remap`` [R]
    int32, the instance of every (view, region) row and ``row_base`` [V + 1] that addresses it (both None with consistent ids)."""
    __slots__ = ("labels", "votes", "seen", "labelled", "dropped", "num_instances", "remap", "row_base")

    def __init__(self, labels, votes, seen, labelled, dropped, num_instances: int, remap=None, row_base=None):
        self.labels, self.votes, self.seen, self.labelled, self.dropped = labels, votes, seen, labelled, dropped
        self.num_instances, self.remap, self.row_base = int(num_instances), remap, row_base

    def bits(self, ids=None):
        """-> (bits [k, W] int64 words of mask_pack's layout, area [k] int32), one row per instance (ids None: all of them, in order; else the listed
        ones): the format mask_geometry, set_crop_to_mask and mask_images take."""
        N, dev = self.labels.shape[0], self.labels.device
        if ids is not None:
            ids = [int(i) for i in ids]
            if any(not 0 <= i < self.num_instances for i in ids):
                raise ValueError(f"Fused.bits: ids must lie in 0 .. {self.num_instances - 1}, got {ids}")
        if self.num_instances == 0 or (ids is not None and not ids):
            return torch.zeros(0, ops.mask_words(N), dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
        bits, area = ops.label_bits(self.labels, self.num_instances)
        if ids is None:
            return bits, area
        sel = torch.as_tensor(ids, dtype=torch.int64, device=dev)
        return bits.index_select(0, sel), area.index_select(0, sel)


def check_labels(labels, shape, device, what: str) -> torch.Tensor:
    """labels: a tensor or a numpy array of int32 [V, height, width] -> the tensor on `device`, contiguous."""
    t = torch.from_numpy(np.ascontiguousarray(labels)) if isinstance(labels, np.ndarray) else labels
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
        raise TypeError(f"{what}: labels must be an int32 tensor or array, got {getattr(t, 'dtype', type(t).__name__)}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: labels must be {list(shape)} (views, height, width), got {list(t.shape)}")
    return t.to(device).contiguous()


def fuse(xyz: torch.Tensor, link_xyz: torch.Tensor, cameras, keys: torch.Tensor, labels: torch.Tensor, cfg: FusionConfig, consistent: bool = False) -> Fused:
    """The pipeline: region rows and links on link_xyz (a subset of xyz that keeps the row matrix small, or xyz itself), the vote on every point of
    xyz.  consistent: the labels are global ids already -- the vote only.  Host reads: the views' label maxima and the edge list (consistent: the
    largest winning label)."""
    if not isinstance(cfg, FusionConfig):
        raise TypeError(f"fuse_labels: cfg must be a fusion.FusionConfig, got {type(cfg).__name__}")
    if not isinstance(consistent, bool):
        raise ValueError(f"fuse_labels: consistent must be True or False, got {consistent!r}")
    if consistent:
        out = ops.fuse_vote(xyz, cameras, keys, labels, cfg.tau, min_votes=cfg.min_votes)
        return Fused(*out, num_instances=int(out[0].max()) + 1)
    V = labels.shape[0]
    counts = (labels.reshape(V, -1).amax(1).long() + 1).clamp_min(0).cpu().numpy()      # one host read
    rb = np.concatenate([[0], np.cumsum(counts)])
    if rb[-1] > cfg.max_regions:
        raise ValueError(f"fuse_labels: the {V} views hold {int(rb[-1])} regions (largest label + 1, summed), more than max_regions = {cfg.max_regions}")
    bits, _ = ops.fuse_region_bits(link_xyz, cameras, keys, labels, rb, cfg.tau)
    remap = link_regions(ops.mask_intersections(bits, bits), rb, cfg)
    remap_dev = torch.from_numpy(remap).to(xyz.device)
    out = ops.fuse_vote(xyz, cameras, keys, labels, cfg.tau, rb, remap_dev, cfg.min_votes)
    return Fused(*out, num_instances=int(remap.max()) + 1 if remap.size else 0, remap=remap_dev, row_base=rb.astype(np.int32))
