"""Masks carried from one scan to the next (csrc/transfer.hip, predictor.snapshot / transfer_masks / propagate).

Everything the predictor knows belongs to one cloud; a sequence -- LiDAR sweeps, repeated captures of a room, a re-scan after something moved -- would
need every object clicked again in every scan.  A `Snapshot` keeps a scan's working cloud and the logits of its objects; in the next scan a
`TransferPlan` gives every point the up to three nearest snapshot points within a radius, in the (idx3, w3) format of the interpolated scene masks, so
ops.scene_interp_rows / ops.scene_interp_bits apply it unchanged.  The format is shared on purpose.

Both scans must have been normalised with the SAME centre and scale; `pose` is the rigid motion that remains in those coordinates (new scan -> the
snapshot's scan).  Where it is not known, or only roughly (odometry), align.py estimates it by ICP on the same index (predictor.align).

No default here -- the radius a caller picks, `clicks = 1`, `fill = None` (the object's own minimum logit) -- has been tuned on a trained checkpoint
(none exists offline).
"""
from dataclasses import dataclass

import torch

from . import ops


@dataclass
class TransferPlan:
    idx3: torch.Tensor        # [M, 3] int32: indices into the source cloud, -1 = unused
    w3: torch.Tensor          # [M, 3] float32
    num_source: int


@dataclass
class Snapshot:
    """What predictor.snapshot keeps of a scan: `coords` [Nw, 3] the working cloud as encoded, `logits` [K, Nw] the objects' logits at working width (the
    representatives' own words), `num_masks` = K; `normals` [Nw, 3] f32, the voxel normal at every working point, or None: kept on request
    (predictor.snapshot(normals=True)) for point-to-plane alignment (predictor.align(plane=...))."""
    coords: torch.Tensor
    logits: torch.Tensor
    num_masks: int
    normals: torch.Tensor = None


@dataclass
class Propagated:
    """predictor.propagate's answer for K snapshot objects in a scan of M points with a working cloud of Nw."""
    logits: torch.Tensor              # [K, M] float32 at the scan's width; the rows of lost objects are -inf
    scores: torch.Tensor              # [K] the decoder's IoU prediction; NaN for lost objects
    lost: torch.Tensor                # [K] bool: the carried mask was empty, the object took no part in the decode
    prior_area: torch.Tensor          # [K] int64: working points with a carried logit > 0
    covered: float                    # the share of working points with a snapshot point within the radius
    click_points: torch.Tensor        # [K, clicks, 3] the simulated clicks; NaN for lost objects
    click_labels: torch.Tensor        # [K, clicks] bool; False for lost objects


def check_snapshot(snap, what: str) -> Snapshot:
    if not isinstance(snap, Snapshot):
        raise TypeError(f"{what}: snap must be a Snapshot (predictor.snapshot), got {type(snap).__name__}")
    c, l = snap.coords, snap.logits
    if c.dim() != 2 or c.shape[1] != 3 or l.dim() != 2 or l.shape[1] != c.shape[0] or l.shape[0] != snap.num_masks or snap.num_masks < 1:
        raise ValueError(f"{what}: a snapshot holds coords [Nw, 3] and logits [K, Nw] with K >= 1, got {tuple(c.shape)}, {tuple(l.shape)}, K = {snap.num_masks}")
    n = snap.normals
    if n is not None and (not isinstance(n, torch.Tensor) or tuple(n.shape) != (c.shape[0], 3) or n.dtype != torch.float32):
        raise ValueError(f"{what}: a snapshot's normals are None or [Nw, 3] float32 with Nw = {c.shape[0]}, got "
                         f"{(tuple(n.shape), n.dtype) if isinstance(n, torch.Tensor) else type(n).__name__}")
    return snap


def check_snapshot_logits(logits, widths, what: str) -> torch.Tensor:
    """logits [K, n], n one of `widths` (the scan's and the working cloud's) -> the tensor; raises before any device work."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.shape[0] < 1:
        raise ValueError(f"{what}: logits must be a [K, n] tensor with K >= 1, got {tuple(logits.shape) if isinstance(logits, torch.Tensor) else type(logits).__name__}")
    if logits.dtype != torch.float32:
        raise TypeError(f"{what}: logits of float32, got {logits.dtype}")
    if logits.shape[1] not in widths:
        raise ValueError(f"{what}: logits have width {logits.shape[1]}: neither the scan's nor the working cloud's ({' / '.join(str(w) for w in sorted(set(widths)))})")
    return logits


def check_propagate_arguments(clicks, fill) -> None:
    if isinstance(clicks, bool) or not isinstance(clicks, int) or clicks < 1:
        raise ValueError(f"propagate: clicks must be an integer >= 1, got {clicks!r}")
    if fill is not None and (isinstance(fill, bool) or not isinstance(fill, (int, float)) or fill != fill):
        raise ValueError(f"propagate: fill must be None (the object's minimum logit) or a number, got {fill!r}")


def check_threshold(threshold, what: str) -> float:
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or threshold != threshold:
        raise ValueError(f"{what}: threshold must be a number, got {threshold!r}")
    return float(threshold)


def build_plan(src_xyz: torch.Tensor, xyz: torch.Tensor, radius, pose=None, eps: float = 1e-8) -> TransferPlan:
    """The plan from the sources `src_xyz` [N, 3] to the queries `xyz` [M, 3]: one index build, one plan launch."""
    index = ops.transfer_index(src_xyz, radius)
    idx3, w3 = ops.transfer_plan(index, xyz, pose, eps)
    return TransferPlan(idx3, w3, index.num_source)


def _check_rows(plan: TransferPlan, rows: torch.Tensor, what: str) -> None:
    if not isinstance(plan, TransferPlan):
        raise TypeError(f"{what}: plan must be a TransferPlan, got {type(plan).__name__}")
    if not isinstance(rows, torch.Tensor) or rows.dim() < 1 or rows.shape[-1] != plan.num_source:
        raise ValueError(f"{what}: rows must be [..., {plan.num_source}] (the source cloud's width), got {tuple(rows.shape) if isinstance(rows, torch.Tensor) else type(rows).__name__}")


def covered(plan: TransferPlan) -> torch.Tensor:
    """[M] bool: the query has a source within the radius."""
    return plan.idx3[:, 0] >= 0


def transfer_rows(plan: TransferPlan, rows: torch.Tensor, fill=None) -> torch.Tensor:
    """rows [..., N] f32 over the source cloud -> [..., M]: the blend of each query's sources, a lone source or an exact hit copied bit for bit, `fill`
    (None: 0.0) where no source is in reach."""
    _check_rows(plan, rows, "transfer_rows")
    return ops.scene_interp_rows(rows, plan.idx3, plan.w3, fill)


def transfer_bits(plan: TransferPlan, rows: torch.Tensor, thr: float = 0.0):
    """-> (bits [K, ceil(M / 64)] int64, area [K] int32): `transfer_rows(...) > thr` packed, an uncovered query 0, without the [K, M] floats."""
    _check_rows(plan, rows, "transfer_bits")
    return ops.scene_interp_bits(rows, plan.idx3, plan.w3, thr)
