"""Point normals and superpoints: a geometric over-segmentation of a cloud into small, roughly planar patches, and masks snapped to whole patches.

Masks copied from a voxel working cloud follow voxel cells at their edges, and labels voted per point are speckled along object borders; the usual
remedy is to snap both to superpoints found from the surface normals.  Everything runs on the voxel graph of ``regions.build_graph``
(``csrc/normals.hip``, ``csrc/superpoints.hip``); results are exact and identical from run to run, and do not depend on the order of the points.

    g = regions.build_graph(xyz)                                # once per cloud
    sp = build_superpoints(g, xyz, SuperpointConfig())          # sp.labels [N] int32, sp.num superpoints
    bits, area, changed = snap_bits(sp, bits)                   # every row becomes a union of superpoints
    normals = estimate_normals(g, xyz).per_point()              # [N, 3] f32
"""
import math
from dataclasses import dataclass
from typing import Optional

import torch

from . import ops, regions

Q16_ONE = 65536


@dataclass
class SuperpointConfig:
    """Touching voxels join when both have at least ``min_points`` points in their neighbourhood, a curvature of at most ``max_curvature``, and
    normals within ``angle_deg`` of each other (either sign); superpoints below ``min_size`` points are then absorbed, voxel by voxel, by the large
    neighbouring superpoint with the most parallel normal, ``absorb_rounds`` times.  ``voxel_size`` None: chosen by ``regions.build_graph`` from
    ``points_per_voxel``.  These defaults are geometric and have NOT been tuned on real data."""
    angle_deg: float = 15.0
    max_curvature: float = 0.08
    min_points: int = 5
    min_size: int = 50
    absorb_rounds: int = 2
    voxel_size: Optional[float] = None
    points_per_voxel: int = 4

    def validate(self) -> "SuperpointConfig":
        for name, lo, hi in (("min_points", 1, 2 ** 31 - 1), ("min_size", 0, 2 ** 31 - 1), ("absorb_rounds", 0, 64), ("points_per_voxel", 1, 2 ** 31 - 1)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError(f"SuperpointConfig.{name} must be an integer in {lo} .. {hi}, got {v!r}")
        for name, lo, hi in (("angle_deg", 0.0, 180.0), ("max_curvature", 0.0, 1.0)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not lo <= v <= hi:      # NaN compares false
                raise ValueError(f"SuperpointConfig.{name} must be a number in [{lo}, {hi}], got {v!r}")
        v = self.voxel_size
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 < v < float("inf")):
            raise ValueError(f"SuperpointConfig.voxel_size must be None or a finite positive number, got {v!r}")
        return self

    @property
    def cos_angle(self) -> float:
        return math.cos(math.radians(self.angle_deg))

    def key(self):
        return (self.angle_deg, self.max_curvature, self.min_points, self.min_size, self.absorb_rounds, self.voxel_size, self.points_per_voxel)


@dataclass
class VoxelNormals:
    """Per occupied voxel of ``graph``: the points of its neighbourhood, the unit normal ((0, 0, 0) below ``min_points``) and the curvature."""
    graph: regions.PointGraph
    count: torch.Tensor             # [V] int32
    normal: torch.Tensor            # [V, 3] f32
    curvature: torch.Tensor         # [V] f32
    scatter: Optional[torch.Tensor] = None      # [V, 6] f64, on request

    def per_point(self):
        """(normal [N, 3] f32, curvature [N] f32): every point takes its voxel's."""
        return self.normal[self.graph.inv], self.curvature[self.graph.inv]


@dataclass
class Superpoints:
    labels: torch.Tensor            # [N] int32: the superpoint of every point, -1 without a cell
    voxel_labels: torch.Tensor      # [V] int32
    size: torch.Tensor              # [num] int32: points per superpoint
    num: int
    normals: VoxelNormals


def _cloud(graph: regions.PointGraph, xyz: torch.Tensor, what: str) -> torch.Tensor:
    if xyz.dim() == 3 and xyz.shape[0] == 1:
        xyz = xyz[0]
    if xyz.dim() != 2 or tuple(xyz.shape) != (graph.n_points, 3):
        raise ValueError(f"{what}: xyz {tuple(xyz.shape)} does not fit the graph's {graph.n_points} points")
    return xyz.contiguous()


def estimate_normals(graph: regions.PointGraph, xyz: torch.Tensor, cfg: SuperpointConfig = None, viewpoint=None, scatter: bool = False) -> VoxelNormals:
    """Normals and curvature of every occupied voxel of ``graph`` (``ops.voxel_normals``); viewpoint: three numbers the normals should face."""
    cfg = (cfg or SuperpointConfig()).validate()
    xyz = _cloud(graph, xyz, "estimate_normals")
    count, normal, curvature, S = ops.voxel_normals(xyz, graph.inv, graph.nbr, cfg.min_points, viewpoint, scatter)
    return VoxelNormals(graph, count, normal, curvature, S)


def build_superpoints(graph: regions.PointGraph, xyz: torch.Tensor, cfg: SuperpointConfig = None, normals: VoxelNormals = None) -> Superpoints:
    """The superpoints of the cloud behind ``graph``.  One host read (the number of superpoints), and it is the only one."""
    cfg = (cfg or SuperpointConfig()).validate()
    if normals is None:
        normals = estimate_normals(graph, xyz, cfg)
    voxel_label, point_label, size, num = ops.superpoint_labels(graph.inv, graph.nbr, normals.count, normals.normal, normals.curvature, cfg.cos_angle,
                                                                cfg.max_curvature, cfg.min_points, cfg.min_size, cfg.absorb_rounds)
    S = int(num.item())
    return Superpoints(point_label, voxel_label, size[:S].contiguous(), S, normals)


def q16_of(min_fraction: float) -> int:
    """The integer threshold of ``ops.superpoint_snap``: a superpoint is selected when MORE than q16 / 65536 of its points are in the row."""
    if isinstance(min_fraction, bool) or not isinstance(min_fraction, (int, float)) or not 0.0 <= min_fraction <= 1.0:
        raise ValueError(f"min_fraction must be a number in [0, 1], got {min_fraction!r}")
    return min(Q16_ONE - 1, int(math.floor(min_fraction * Q16_ONE)))


def rows_per_call(num: int) -> int:
    """Rows whose [rows, num] int32 table stays under regions.WORKSPACE_LIMIT."""
    return max(1, min(regions.MAX_ROWS, regions.WORKSPACE_LIMIT // (4 * max(1, num) + 16)))


def snap_bits(sp: Superpoints, bits: torch.Tensor, min_fraction: float = 0.5, chunk: int = None):
    """bits [K, W] int64 -> (bits [K, W] int64, area [K] int32, changed [K] uint8): every row becomes the union of the superpoints of which it
    holds more than ``min_fraction`` (``ops.superpoint_snap``), in chunks of rows (chunk None: rows_per_call).  From 0.5 on, rows that were
    disjoint stay disjoint.  No host synchronisation."""
    if bits.dim() != 2 or bits.shape[1] != ops.mask_words(sp.labels.numel()):
        raise ValueError(f"snap_bits: bits {tuple(bits.shape)} do not fit the superpoints' {sp.labels.numel()} points")
    if chunk is not None and (isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1):
        raise ValueError(f"snap_bits: chunk must be a positive integer, got {chunk!r}")
    q16 = q16_of(min_fraction)
    K = bits.shape[0]
    step = min(chunk or regions.MAX_ROWS, rows_per_call(sp.num))
    out = torch.empty_like(bits)
    area = torch.empty(K, dtype=torch.int32, device=bits.device)
    changed = torch.empty(K, dtype=torch.uint8, device=bits.device)
    for k0 in range(0, K, step):
        k1 = min(K, k0 + step)
        out[k0:k1], area[k0:k1], changed[k0:k1] = ops.superpoint_snap(bits[k0:k1], sp.labels, sp.size, q16)
    return out, area, changed
