"""Connected components of masks: which points of a mask hang together, and the clean-up built on it.

A thresholded mask of a point cloud nearly always has stray islands and pin-holes.  Points are adjacent when their voxel cells (the cells of
``ops.voxel_downsample``) touch -- the same cell or one of the 26 around it -- and the components of a mask are those of the graph it induces
(``csrc/regions.hip``: a union-find over the occupied voxels, per mask row, on the device).  Everything is an integer or a bit: results are exact.

    g = build_graph(xyz)                                        # once per cloud
    bits, area, changed = clean_bits(g, bits, cfg=RegionConfig(min_island=30, min_hole=30))
    labels = components(g, bits)                                # [K, N] int32: component id per point, -1 outside the mask
"""
from dataclasses import dataclass
from typing import Optional

import torch

from . import ops

WORKSPACE_LIMIT = 256 << 20      # bytes of workspace per call: the rows are cleaned / labelled in chunks that stay under it
MAX_ROWS = 65535                 # rows per call of the library


@dataclass
class PointGraph:
    """The neighbourhood graph of one cloud at one voxel size.  ``inv[keep_idx[v]] == v``; a point's voxel rank is ``inv[i]``."""
    voxel_size: float
    keep_idx: torch.Tensor          # [V] int64: the lowest point index of every occupied voxel, increasing
    inv: torch.Tensor               # [N] int64: the voxel rank of every point
    nbr: torch.Tensor               # [V, 26] int32: the ranks of the 26 surrounding voxels, -1 where none is occupied
    n_points: int


@dataclass
class RegionConfig:
    """``min_island`` / ``min_hole``: components of the mask / of its complement with fewer points are removed / filled (0 = off); the largest
    component of a mask is never removed.  ``keep_clicked`` (PointSAMPredictor.clean_masks): only the components that hold a positive click stay.
    ``voxel_size`` None: chosen by ``build_graph`` from ``points_per_voxel``.  That rule is geometric and has NOT been tuned on real data."""
    min_island: int = 0
    min_hole: int = 0
    voxel_size: Optional[float] = None
    points_per_voxel: int = 4
    keep_clicked: bool = False

    def validate(self) -> "RegionConfig":
        for name in ("min_island", "min_hole", "points_per_voxel"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"RegionConfig.{name} must be an integer, got {v!r}")
        if self.min_island < 0 or self.min_hole < 0:
            raise ValueError("RegionConfig: min_island and min_hole must not be negative")
        if self.points_per_voxel < 1:
            raise ValueError("RegionConfig.points_per_voxel must be at least 1")
        v = self.voxel_size
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 < v < float("inf")):
            raise ValueError(f"RegionConfig.voxel_size must be None or a finite positive number, got {v!r}")
        if not isinstance(self.keep_clicked, bool):
            raise ValueError(f"RegionConfig.keep_clicked must be a bool, got {self.keep_clicked!r}")
        return self


def build_graph(xyz: torch.Tensor, voxel_size: Optional[float] = None, points_per_voxel: int = 4) -> PointGraph:
    """xyz [N, 3] (or [1, N, 3]) f32 on the device, coordinates in [-1, 1] -> the cloud's `PointGraph`.

    voxel_size None: the smallest size of ``scene.choose_voxel_size``'s ladder that leaves at most ``max(1, N // points_per_voxel)`` occupied voxels,
    so that a voxel holds `points_per_voxel` points on average and neighbouring surface points fall into touching cells.  This rule is geometric and
    has NOT been tuned on real data: give the voxel size where the sampling density of the clouds is known.

    The host synchronises here (the count of occupied voxels, once per ladder step and once for the downsample) and nowhere else in this module."""
    if xyz.dim() == 3 and xyz.shape[0] == 1:
        xyz = xyz[0]
    if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] < 1:
        raise ValueError(f"build_graph: xyz must be [N, 3] (one cloud), got {tuple(xyz.shape)}")
    if isinstance(points_per_voxel, bool) or not isinstance(points_per_voxel, int) or points_per_voxel < 1:
        raise ValueError(f"build_graph: points_per_voxel must be a positive integer, got {points_per_voxel!r}")
    xyz = xyz.contiguous()
    N = xyz.shape[0]
    if voxel_size is None:
        from .scene import choose_voxel_size
        voxel_size = choose_voxel_size(xyz, max(1, N // points_per_voxel))
    keep_idx, inv = ops.voxel_downsample(xyz, voxel_size)
    keep_idx = keep_idx.contiguous()
    return PointGraph(float(voxel_size), keep_idx, inv, ops.region_neighbors(xyz, keep_idx, voxel_size), N)


def _check(graph: PointGraph, bits: torch.Tensor, what: str):
    if bits.dim() != 2 or bits.shape[1] != ops.mask_words(graph.n_points):
        raise ValueError(f"{what}: bits {tuple(bits.shape)} do not fit the graph's {graph.n_points} points ({ops.mask_words(graph.n_points)} words per row)")


def rows_per_call(graph: PointGraph, n_seeds: int = 0) -> int:
    """Rows whose workspace (a few [rows, V] int32 arrays) stays under WORKSPACE_LIMIT."""
    per_row = 4 * graph.keep_idx.numel() * (4 if n_seeds > 0 else 3) + 64
    return max(1, min(MAX_ROWS, WORKSPACE_LIMIT // per_row))


def clean_bits(graph: PointGraph, bits: torch.Tensor, select: torch.Tensor = None, seeds: torch.Tensor = None, cfg: RegionConfig = None,
               chunk: int = None):
    """bits [K, W] int64 -> (bits [K, W] int64, area [K] int32, changed [K] uint8): `ops.region_clean` with cfg.min_island / cfg.min_hole, in chunks
    of rows (chunk None: rows_per_call).  select [K] uint8: rows with 0 are copied; seeds [K, S] int32: see ops.region_clean.  No host
    synchronisation."""
    cfg = (cfg or RegionConfig()).validate()
    _check(graph, bits, "clean_bits")
    K = bits.shape[0]
    S = 0 if seeds is None else seeds.shape[1]
    step = chunk or rows_per_call(graph, S)
    out = torch.empty_like(bits)
    area = torch.empty(K, dtype=torch.int32, device=bits.device)
    changed = torch.empty(K, dtype=torch.uint8, device=bits.device)
    for k0 in range(0, K, step):
        k1 = min(K, k0 + step)
        b, a, c = ops.region_clean(bits[k0:k1], graph.inv, graph.nbr, cfg.min_island, cfg.min_hole, None if select is None else select[k0:k1],
                                   None if seeds is None or S == 0 else seeds[k0:k1].contiguous())
        out[k0:k1], area[k0:k1], changed[k0:k1] = b, a, c
    return out, area, changed


def components(graph: PointGraph, bits: torch.Tensor, complement: bool = False, chunk: int = None) -> torch.Tensor:
    """bits [K, W] int64 -> [K, N] int32: per point the id of its component within the row's mask (the lowest voxel rank, ``graph.inv``, among the
    component's points), -1 outside the mask.  complement: the components of the points NOT in the mask."""
    _check(graph, bits, "components")
    K = bits.shape[0]
    step = chunk or rows_per_call(graph)
    out = torch.empty(K, graph.n_points, dtype=torch.int32, device=bits.device)
    for k0 in range(0, K, step):
        k1 = min(K, k0 + step)
        out[k0:k1] = ops.region_labels(bits[k0:k1], graph.inv, graph.nbr, complement)
    return out
