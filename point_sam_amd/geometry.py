"""Instance geometry: where a packed mask is, how big it is and what colour it has.

``mask_geometry(xyz, bits)`` turns the rows of ``Proposals.bits`` (or any packed masks of ``ops.mask_pack``'s layout) into a centroid, an
axis-aligned box, a covariance, a mean colour, an oriented box and a bounding radius per mask.  The two passes over the points are HIP kernels
(csrc/geometry.hip: ``ops.mask_moments``, ``ops.mask_extents``) whose work follows the set bits; between them the host solves one 3 x 3
symmetric eigenproblem per mask in fp64 on ``K x 19`` numbers.

Frame.  The box axes are the covariance's eigenvectors by descending eigenvalue.  Signs: the component of largest magnitude of axis 0 and of
axis 1 is positive (the first such component on a tie), axis 2 = axis 0 x axis 1, so the frame is right-handed.  The oriented box is the tight box
of the members IN THAT FRAME, evaluated in fp32 exactly as the header states; it is not the minimum-volume box.

Degenerate masks.  With fewer than three members, or members on a line or in a plane, or equal eigenvalues (a cube, a sphere), some axes are
not determined by the points: the frame returned is then an arbitrary orthonormal one (whatever the eigensolver gives, with the sign rule above),
and the box is still tight in it.  An empty mask has ``valid == False`` and NaN everywhere but ``count`` (0).

Precision.  The covariance is formed from raw second moments, ``cov = sum(xx) / n - c c^T`` in fp64.  Each sum carries an error of at most
``n 2^-53 sum|t|`` (any summation order), so an entry of the covariance is off by at most about ``n 2^-53 m``, m = the mask's mean squared coordinate
(<= 1 in the unit ball): 1.1e-9 at ``n = 10^7``, a length of 3.3e-5.  The smallest voxel of the ladder is ``2^-19 = 1.9e-6`` wide (variance
``h^2 / 12 = 3e-13``), so nothing at that scale survives a mask of 10^7 points; an eigenvalue is meaningful only while it is far above
``n 2^-53 m`` -- thicknesses well above 1.1e-4 at ``n = 10^7``, 1.1e-5 at ``10^5``, 1.1e-6 at ``10^3`` -- and below that it is rounding noise (it can be
negative) and its axis arbitrary.  Centroid, boxes and radius have no such cancellation.  DESIGN.md, section 4.10.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import ops


@dataclass
class InstanceGeometry:
    """One entry per mask, tensors on the CPU.  Rows with ``valid == False`` (empty masks) are NaN except ``count``."""
    count: torch.Tensor                  # [k] int32
    centroid: torch.Tensor               # [k, 3] f64
    aabb_lo: torch.Tensor                # [k, 3] f32
    aabb_hi: torch.Tensor                # [k, 3] f32
    covariance: torch.Tensor             # [k, 3, 3] f64, symmetric
    mean_rgb: Optional[torch.Tensor]     # [k, 3] f64, None without colours
    axes: torch.Tensor                   # [k, 3, 3] f32: row i is box axis i
    obb_center: torch.Tensor             # [k, 3] f64
    obb_half: torch.Tensor               # [k, 3] f64: half sides along the axes
    radius: torch.Tensor                 # [k] f32: distance from the (fp32) centroid to the farthest member
    valid: torch.Tensor                  # [k] bool = count > 0

    def __len__(self) -> int:
        return int(self.count.numel())


def centroid_covariance(count: np.ndarray, sums: np.ndarray):
    """count [k], sums [k, 12] f64 (ops.mask_moments) -> (centroid [k, 3], covariance [k, 3, 3], mean of the last three columns [k, 3]) in fp64; NaN rows
    where count == 0."""
    n = count.astype(np.float64)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        c = sums[:, 0:3] / n
        m2 = sums[:, 3:9] / n
        mean_rgb = sums[:, 9:12] / n
    xx, xy, xz, yy, yz, zz = (m2[:, i] for i in range(6))
    raw = np.stack([np.stack([xx, xy, xz], -1), np.stack([xy, yy, yz], -1), np.stack([xz, yz, zz], -1)], -2)
    cov = raw - c[:, :, None] * c[:, None, :]
    cov = 0.5 * (cov + cov.transpose(0, 2, 1))
    return c, cov, mean_rgb


def principal_axes(cov: np.ndarray) -> np.ndarray:
    """cov [k, 3, 3] f64 symmetric (finite) -> axes [k, 3, 3] f64, rows = eigenvectors by descending eigenvalue; the largest-magnitude component of
    rows 0 and 1 is positive, row 2 = row 0 x row 1."""
    _, vec = np.linalg.eigh(cov)                         # ascending eigenvalues, eigenvectors in columns
    ax = vec[:, :, ::-1].transpose(0, 2, 1).copy()       # rows, descending
    for i in (0, 1):
        big = np.argmax(np.abs(ax[:, i, :]), axis=1)
        sign = np.where(np.take_along_axis(ax[:, i, :], big[:, None], 1)[:, 0] < 0, -1.0, 1.0)
        ax[:, i, :] *= sign[:, None]
    ax[:, 2, :] = np.cross(ax[:, 0, :], ax[:, 1, :])
    return ax


@torch.no_grad()
def mask_geometry(xyz: torch.Tensor, bits: torch.Tensor, rgb: torch.Tensor = None, oriented: bool = True) -> InstanceGeometry:
    """xyz [N, 3] f32 on the GPU, bits [k, W] int64 words of ops.mask_pack's layout, rgb [N, 3] f32 or None -> InstanceGeometry.

    oriented=False skips the eigen step: the axes are the identity, the oriented box is the axis-aligned one, and the second pass only measures the
    radius.  One device-to-host copy after each of the two kernels."""
    if not isinstance(oriented, bool):
        raise ValueError(f"mask_geometry: oriented must be True or False, got {oriented!r}")
    if bits.dim() == 2 and bits.shape[0] == 0:
        z3, z33 = torch.zeros(0, 3, dtype=torch.float64), torch.zeros(0, 3, 3, dtype=torch.float64)
        return InstanceGeometry(torch.zeros(0, dtype=torch.int32), z3, z3.float(), z3.float(), z33, None if rgb is None else z3.clone(), z33.float(),
                                z3.clone(), z3.clone(), torch.zeros(0, dtype=torch.float32), torch.zeros(0, dtype=torch.bool))
    count, sums, lo, hi = ops.mask_moments(xyz, bits, rgb)
    k = count.shape[0]
    # one copy: K x (1 + 12 + 6) numbers, all exactly representable in fp64
    packed = torch.cat([count.to(torch.float64)[:, None], sums, lo.to(torch.float64), hi.to(torch.float64)], 1).cpu().numpy()
    cnt = packed[:, 0].astype(np.int64)
    valid = cnt > 0
    centroid, cov, mean_rgb = centroid_covariance(cnt, packed[:, 1:13])
    aabb_lo, aabb_hi = packed[:, 13:16].astype(np.float32), packed[:, 16:19].astype(np.float32)
    aabb_lo[~valid], aabb_hi[~valid] = np.nan, np.nan
    axes = np.tile(np.eye(3), (k, 1, 1))
    if oriented and valid.any():
        axes[valid] = principal_axes(cov[valid])
    axes32 = axes.astype(np.float32)
    origin32 = np.where(valid[:, None], centroid, 0.0).astype(np.float32)          # an empty row's origin is never used: no member
    dev = bits.device
    elo, ehi, r2 = ops.mask_extents(xyz, bits, torch.from_numpy(origin32).to(dev), torch.from_numpy(axes32).to(dev) if oriented else None)
    ext = torch.cat([elo, ehi, r2[:, None]], 1).cpu().numpy()
    elo, ehi, r2 = ext[:, 0:3].astype(np.float64), ext[:, 3:6].astype(np.float64), ext[:, 6]
    with np.errstate(invalid="ignore"):
        mid, half = (elo + ehi) / 2, (ehi - elo) / 2
        center = origin32.astype(np.float64) + np.einsum("ki,kij->kj", mid, axes32.astype(np.float64))
        radius = np.sqrt(r2.astype(np.float32))
        if not oriented:                                   # the axis-aligned box of the first pass IS the box: exact, no second rounding
            blo, bhi = packed[:, 13:16], packed[:, 16:19]
            center, half = (blo + bhi) / 2, (bhi - blo) / 2
    bad = ~valid
    for a in (centroid, cov, mean_rgb, center, half):
        a[bad] = np.nan
    axes32[bad] = np.nan
    radius[bad] = np.nan
    t = torch.from_numpy
    return InstanceGeometry(count=t(cnt.astype(np.int32)), centroid=t(centroid), aabb_lo=t(aabb_lo), aabb_hi=t(aabb_hi), covariance=t(cov),
                            mean_rgb=None if rgb is None else t(mean_rgb), axes=t(axes32), obb_center=t(center), obb_half=t(half),
                            radius=t(radius.astype(np.float32)), valid=t(valid))
