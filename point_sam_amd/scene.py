"""Full-resolution scenes: a scan of M points (one to several million) served by the model through a voxel-grid working cloud.

One real point per occupied voxel is kept (the one with the lowest index), the model runs on those, and every point of the scan receives the result of
its voxel's representative.  The reduction and the transfer are ``csrc/scene.hip``: a device hash of the scan and gathers of 32-bit words or of single
bits, all integer work or bit-for-bit copies, so a result at full resolution is exactly the working cloud's result indexed by ``inv``.

    pred.set_scene(xyz, rgb, max_points=131072)          # xyz [M, 3] in [-1, 1], rgb as for set_pointcloud
    logits, scores, _ = pred.predict_masks(points, labels)   # logits [M', C, M]
    pred.scene.keep_idx, pred.scene.inv, pred.scene.num_working

A crop zooms into a ball of the scan (``csrc/crops.hip``): its points, normalised to the unit ball, get a finer working cloud and an encoder pass of
their own, and the results come back per scan point, with -inf logits / zero bits / label -1 off the ball.

    pred.set_crop(center, radius, max_points=32768)          # scan coordinates; after set_scene
    logits, scores, _ = pred.predict_masks(points, labels)   # points in scan coordinates, inside the ball; logits [M', C, M]
    pred.crop.keep_idx, pred.crop.inv, pred.crop.num_members; pred.clear_crop()
"""
from dataclasses import dataclass
from typing import Callable, Optional

import torch

from . import ops

LADDER_STEPS = 80                                         # voxel sizes 2 ** (1 - k / 4), k = 0 .. 80: from the whole cube down to 2^-19


def ladder(k: int) -> float:
    return 2.0 ** (1.0 - k / 4.0)


def choose_voxel_size(xyz: torch.Tensor, max_points: int, count: Optional[Callable[[int], int]] = None) -> float:
    """The smallest voxel size of the ladder ``h_k = 2 ** (1 - k / 4)``, k = 0 .. 80, found by bisection, that leaves at most `max_points` occupied
    voxels (origin (-1, -1, -1)).  The procedure is the definition: ``lo, hi = 0, 80``; while ``hi - lo > 1``: ``mid = (lo + hi) // 2``, ``lo = mid`` if
    ``count(mid) <= max_points`` else ``hi = mid``; the result is ``h_lo``.  ValueError if even h_0 leaves more than `max_points`.  About seven
    count-only passes over the scan.  count: k -> occupied voxels at h_k (default: ops.voxel_count on `xyz`)."""
    if isinstance(max_points, bool) or not isinstance(max_points, int) or max_points < 1:
        raise ValueError(f"max_points must be a positive integer, got {max_points!r}")
    if count is None:
        count = lambda k: ops.voxel_count(xyz, ladder(k))
    n0 = count(0)
    if n0 > max_points:
        raise ValueError(f"the coarsest voxel size {ladder(0)} still leaves {n0} points, more than max_points = {max_points}")
    lo, hi = 0, LADDER_STEPS
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if count(mid) <= max_points:
            lo = mid
        else:
            hi = mid
    return ladder(lo)


@dataclass
class Scene:
    """The mapping between a scan and its working cloud.  ``inv[keep_idx[j]] == j``; ``keep_idx`` is strictly increasing."""
    num_points: int                 # M
    num_working: int
    keep_idx: torch.Tensor          # [num_working] int64: the scan indices of the working cloud's points
    inv: torch.Tensor               # [M] int64: the working-cloud row of each scan point's representative
    voxel_size: Optional[float]     # None: the scene is its own working cloud
    identity: bool                  # keep_idx == inv == arange(M): nothing is gathered or expanded


def check_scene_arguments(xyz, rgb, voxel_size, max_points):
    """-> (xyz [M, 3], rgb [M, 3]).  One cloud; exactly one of voxel_size / max_points."""
    if (voxel_size is None) == (max_points is None):
        raise ValueError("set_scene: give exactly one of voxel_size and max_points")
    if voxel_size is not None and (isinstance(voxel_size, bool) or not isinstance(voxel_size, (int, float)) or not 0 < voxel_size < float("inf")):
        raise ValueError(f"set_scene: voxel_size must be a finite positive number, got {voxel_size!r}")
    if max_points is not None and (isinstance(max_points, bool) or not isinstance(max_points, int) or max_points < 1):
        raise ValueError(f"set_scene: max_points must be a positive integer, got {max_points!r}")
    if xyz.dim() == 3:
        if xyz.shape[0] != 1:
            raise ValueError(f"set_scene: a scene is one cloud (B = 1), got a batch of {xyz.shape[0]}")
        xyz = xyz[0]
    if rgb.dim() == 3:
        if rgb.shape[0] != 1:
            raise ValueError(f"set_scene: a scene is one cloud (B = 1), got a batch of {rgb.shape[0]}")
        rgb = rgb[0]
    if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] < 1 or tuple(rgb.shape) != tuple(xyz.shape):
        raise ValueError(f"set_scene: xyz and rgb must both be [M, 3], got {tuple(xyz.shape)} and {tuple(rgb.shape)}")
    return xyz, rgb


def build_scene(xyz: torch.Tensor, voxel_size: Optional[float], max_points: Optional[int]) -> Scene:
    """xyz [M, 3] on the device.  With max_points and M <= max_points the scene is its own working cloud and no kernel runs."""
    M = xyz.shape[0]
    if max_points is not None:
        if M <= max_points:
            ar = torch.arange(M, dtype=torch.int64, device=xyz.device)
            return Scene(M, M, ar, ar, None, True)
        voxel_size = choose_voxel_size(xyz, max_points)
    keep_idx, inv = ops.voxel_downsample(xyz, voxel_size)
    return Scene(M, keep_idx.numel(), keep_idx, inv, float(voxel_size), False)


@dataclass
class Crop:
    """A ball of a scan as a cloud of its own: the members (|x - center| <= radius, in the kernel's fp32 arithmetic) normalised to (x - center) / radius
    and reduced to one real member per occupied voxel.  ``inv[keep_idx[j]] == j``; ``keep_idx`` is strictly increasing; ``inv == -1`` exactly off the ball."""
    center: tuple                   # three floats (fp32 values), scan coordinates
    radius: float                   # an fp32 value, scan units
    num_points: int                 # M, the scan's
    num_members: int                # points of the scan inside the ball
    num_working: int
    keep_idx: torch.Tensor          # [num_working] int64: the scan indices of the crop cloud's points
    inv: torch.Tensor               # [M] int64: the crop-cloud row of each member's representative, -1 off the ball
    voxel_size: Optional[float]     # in crop units (the ball has radius 1); None: every member is a point of the crop cloud
    identity = False                # a crop is never its scan: outputs are always expanded


def _f32(v) -> float:
    import numpy as np
    return float(np.float32(v))


def build_crop(xyz: torch.Tensor, rgb: torch.Tensor, center, radius: float, voxel_size: Optional[float] = None, max_points: Optional[int] = None):
    """-> (Crop, wxyz [n, 3], wrgb [n, 3]): the crop cloud of the ball (center, radius) of the scan xyz / rgb [M, 3] (ops.crop_downsample).  At most one of
    `voxel_size` (crop units) and `max_points`; neither: every member is kept.  With max_points and no more members than that there is no reduction;
    otherwise the voxel size is choose_voxel_size's, on the ladder, counting the ball's occupied voxels (about seven count-only passes).  ValueError
    for an empty ball."""
    if voxel_size is not None and max_points is not None:
        raise ValueError("build_crop: give at most one of voxel_size and max_points")
    if voxel_size is not None and (isinstance(voxel_size, bool) or not isinstance(voxel_size, (int, float)) or not 0 < voxel_size < float("inf")):
        raise ValueError(f"build_crop: voxel_size must be a finite positive number, got {voxel_size!r}")
    if max_points is not None and (isinstance(max_points, bool) or not isinstance(max_points, int) or max_points < 1):
        raise ValueError(f"build_crop: max_points must be a positive integer, got {max_points!r}")
    if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] < 1 or tuple(rgb.shape) != tuple(xyz.shape):
        raise ValueError(f"build_crop: xyz and rgb must both be [M, 3], got {tuple(xyz.shape)} and {tuple(rgb.shape)}")
    center = tuple(float(v) for v in center)
    if len(center) != 3:
        raise ValueError(f"build_crop: center must be three numbers, got {center!r}")
    if max_points is not None:
        _, members = ops.crop_count(xyz, center, radius, None)
        if members > max_points:
            voxel_size = choose_voxel_size(xyz, max_points, count=lambda k: ops.crop_count(xyz, center, radius, ladder(k))[0])
    keep_idx, inv, wxyz, wrgb, members = ops.crop_downsample(xyz, rgb, center, radius, voxel_size)
    if members == 0:
        raise ValueError(f"build_crop: no point of the scan lies in the ball of radius {radius} around {center}")
    crop = Crop(tuple(_f32(v) for v in center), _f32(radius), xyz.shape[0], members, keep_idx.numel(), keep_idx, inv,
                None if voxel_size is None else float(voxel_size))
    return crop, wxyz, wrgb


def crop_prompts(crop: Crop, points: torch.Tensor) -> torch.Tensor:
    """Prompt points [..., 3] in scan coordinates -> crop coordinates, with the kernel's arithmetic (fp32, one rounded operation at a time):
    d = p - c, u = clamp(d * fl32(1 / r), -1, 1).  ValueError for a prompt outside the ball (q = (dx dx + dy dy) + dz dz > fl32(r) * fl32(r), or NaN)."""
    import numpy as np
    r = np.float32(crop.radius)
    r2, inv_r = float(r * r), float(np.float32(1) / r)
    p = points.to(torch.float32)
    d = p - torch.tensor(crop.center, dtype=torch.float32, device=p.device)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    q = (dx * dx + dy * dy) + dz * dz
    if not bool((q <= r2).all()):
        raise ValueError(f"a prompt point lies outside the crop (centre {crop.center}, radius {crop.radius}): prompts are scan coordinates inside the ball")
    return torch.clamp(d * inv_r, -1.0, 1.0)


def crop_shell_bits(crop: Crop, xyz: torch.Tensor, edge_frac: float) -> torch.Tensor:
    """-> [1, ceil(num_working / 64)] int64: the crop cloud's points in the ball's outer shell, q > rs * rs with rs = fl32((1 - edge_frac) * r) and q
    as in the membership test, from the scan coordinates xyz [M, 3]."""
    import numpy as np
    rs = np.float32((1.0 - edge_frac) * crop.radius)
    d = xyz.index_select(0, crop.keep_idx) - torch.tensor(crop.center, dtype=torch.float32, device=xyz.device)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    q = (dx * dx + dy * dy) + dz * dz
    return ops.mask_pack(q[None].contiguous(), float(rs * rs), 0.0)[0]


@dataclass
class InterpPlan:
    """Smooth edges: per scan point up to three working points and their weights (``csrc/scene_interp.hip``).  Geometry only: one plan serves every click."""
    idx3: torch.Tensor              # [M, 3] int32: working-cloud rows, -1 = unused (all three off a crop's ball)
    w3: torch.Tensor                # [M, 3] float32: the weights; (1, 0, 0) where a single source is copied


def build_interp_plan(mapping, xyz: torch.Tensor, wxyz: torch.Tensor) -> Optional[InterpPlan]:
    """The plan that carries a working cloud's logits to the scan by a 3-NN inverse-distance blend over each point's 27-cell voxel neighbourhood.
    mapping: a `Scene` or a `Crop`; xyz [M, 3] the scan; wxyz [num_working, 3] the working cloud as it was encoded (the scan's points for a scene,
    the normalised ones for a crop).  The neighbour table is the grid's the working cloud was built on: the scene's voxel size from origin -1 on the
    scan, the crop's (crop units) from origin -1 on the crop cloud, every crop point its own voxel.  None for an identity scene and for a crop
    without a voxel size: every point is its own representative, there is nothing to blend.  24 bytes per scan point."""
    if mapping.identity or mapping.voxel_size is None:
        return None
    if isinstance(mapping, Crop):
        ranks = torch.arange(mapping.num_working, dtype=torch.int64, device=wxyz.device)
        nbr = ops.region_neighbors(wxyz, ranks, mapping.voxel_size)
        return InterpPlan(*ops.scene_interp_plan(xyz, mapping.inv, wxyz, nbr, center=mapping.center, radius=mapping.radius))
    nbr = ops.region_neighbors(xyz, mapping.keep_idx, mapping.voxel_size)
    return InterpPlan(*ops.scene_interp_plan(xyz, mapping.inv, wxyz, nbr))


def reduce_prompt_mask(scene, prompt_mask: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """A mask prompt of the scan's width -> the working cloud's width: the representatives' own values (exact: inv[keep_idx[j]] == j).  A mask of
    the working cloud's width passes unchanged.  scene: a `Scene` or a `Crop` (whose cloud is narrower than the scan: points off the ball drop out)."""
    if prompt_mask is None or scene.identity or prompt_mask.shape[-1] == scene.num_working:
        return prompt_mask
    if prompt_mask.shape[-1] != scene.num_points:
        raise ValueError(f"prompt_mask has width {prompt_mask.shape[-1]}: neither the scene's {scene.num_points} points nor its {scene.num_working} working points")
    return prompt_mask.to(scene.keep_idx.device).index_select(-1, scene.keep_idx)


def expand_proposals(scene, p):
    """A working-cloud `Proposals` -> the same proposals at full resolution: bits, area and labels per scan point; scores, candidates, stability and the
    order are the working cloud's (filtering and suppression were decided there).  For a `Crop` the points off the ball get zero bits and label -1."""
    import dataclasses
    if scene.identity:
        return p
    crop = isinstance(scene, Crop)
    if len(p) > 0:
        bits, area = (ops.crop_expand_bits if crop else ops.scene_expand_bits)(p.bits.contiguous(), scene.inv, scene.num_working)
    else:
        bits, area = p.bits.new_zeros(0, ops.mask_words(scene.num_points)), p.area
    labels = ops.crop_expand_rows(p.labels, scene.inv, -1) if crop else ops.scene_expand_rows(p.labels, scene.inv)
    return dataclasses.replace(p, n_points=scene.num_points, bits=bits, area=area, labels=labels)
