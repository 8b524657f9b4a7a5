"""Automatic mask proposals: segment a whole cloud with no prompts from a person.

The SAM recipe on the cached encoder state: a grid of prompt points (farthest point sampling, as Point-SAM's zero-shot object proposals),
three candidate masks per prompt from the existing ``decode``, a filter on predicted IoU and on stability, greedy non-maximum suppression
on mask IoU, one instance label per point.  Everything after the logits runs on bit-packed masks (``csrc/masks.hip``: 64 points per
64-bit word, and + popcount), so every count is an exact integer, and on the device: the host synchronises once per cloud, after the last
kernel, to compact the kept rows.

    state = model.encode(xyz, rgb)
    for p in generate_proposals(model, state, ProposalConfig(num_prompts=1024)):
        p.labels            # [N] int32: rank of the best kept mask containing the point, -1 = unlabelled
        p.masks()           # [k, N] bool, best first
"""
import dataclasses
import math
from dataclasses import dataclass
from typing import List, Optional

import torch

from . import ops

MAX_CANDIDATES = 16384      # psam_mask_nms (the walk keeps the removed set in one wave's registers)


@dataclass
class ProposalConfig:
    """Defaults: ``pred_iou_thresh`` 0.88, ``stability_thresh`` 0.95, ``stability_offset`` 1.0 and ``nms_thresh`` 0.7 are the published defaults of
    SAM's automatic mask generator, whose IoU head and stability score Point-SAM's decoder mirrors; they have NOT been tuned on a trained Point-SAM
    checkpoint.  ``min_points`` / ``max_area_frac`` are the reference's own instance filter (at least 25 points, under 90 % of the cloud).  With random
    weights nearly every candidate fails the two score cuts: set them to 0 to see the machinery work.

    ``min_region_points`` > 0 (SAM's ``min_mask_region_area``): every candidate that passes the score and stability cuts is cleaned before the area
    filter and the suppression -- complement components (holes) with fewer points are filled, then mask components (islands) with fewer points are
    removed, the largest always kept (point_sam_amd/regions.py).  ``region_voxel_size`` is the cell size of the neighbourhood graph, 0 = chosen so that
    a voxel holds ``region_points_per_voxel`` points on average: a geometric rule that has NOT been tuned on real data either.

    ``snap``: a `superpoints.SuperpointConfig` (or, in from_overrides, a dict of its fields) -- after the clean-up and before the area filter and the
    suppression every candidate becomes the union of the superpoints of which it holds a strict majority (point_sam_amd/superpoints.py).  None: off,
    nothing is built."""
    num_prompts: int = 1024        # FPS-sampled prompt points per cloud
    prompt_chunk: int = 64         # prompts per decode() call and cloud
    mask_threshold: float = 0.0
    pred_iou_thresh: float = 0.88
    stability_thresh: float = 0.95
    stability_offset: float = 1.0
    nms_thresh: float = 0.7
    min_points: int = 25
    max_area_frac: float = 0.9
    min_region_points: int = 0     # 0 = no clean-up, no graph is built
    region_voxel_size: float = 0.0  # 0 = automatic
    region_points_per_voxel: int = 4
    snap: Optional["SuperpointConfig"] = None      # None = no snapping, no superpoints are built

    def validate(self) -> "ProposalConfig":
        if self.snap is not None:
            from .superpoints import SuperpointConfig
            if not isinstance(self.snap, SuperpointConfig):
                raise ValueError(f"ProposalConfig.snap must be None or a SuperpointConfig, got {self.snap!r}")
            self.snap.validate()
        for name in ("num_prompts", "prompt_chunk", "min_points", "min_region_points", "region_points_per_voxel"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"ProposalConfig.{name} must be an integer, got {v!r}")
        for name in ("mask_threshold", "pred_iou_thresh", "stability_thresh", "stability_offset", "nms_thresh", "max_area_frac", "region_voxel_size"):
            v = getattr(self, name)
            # the three cuts may be infinite (-inf = no cut); everything else is finite
            if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v) or (
                    math.isinf(v) and name not in ("mask_threshold", "pred_iou_thresh", "stability_thresh")):
                raise ValueError(f"ProposalConfig.{name} must be a number (finite, except the three thresholds), got {v!r}")
        if self.num_prompts < 1 or self.prompt_chunk < 1:
            raise ValueError("ProposalConfig: num_prompts and prompt_chunk must be at least 1")
        if self.min_points < 0 or self.stability_offset < 0 or self.max_area_frac <= 0:
            raise ValueError("ProposalConfig: min_points and stability_offset must not be negative, max_area_frac must be positive")
        if self.min_region_points < 0 or self.region_voxel_size < 0 or self.region_points_per_voxel < 1:
            raise ValueError("ProposalConfig: min_region_points and region_voxel_size must not be negative, region_points_per_voxel must be at least 1")
        if not 0.0 <= self.nms_thresh <= 1.0:
            raise ValueError(f"ProposalConfig.nms_thresh is an IoU: it must lie in [0, 1], got {self.nms_thresh}")
        return self

    @classmethod
    def from_overrides(cls, overrides: dict) -> "ProposalConfig":
        """The defaults with the given fields replaced; an unknown field is a ValueError (the demo's 400)."""
        names = {f.name for f in dataclasses.fields(cls)}
        unknown = sorted(set(overrides) - names)
        if unknown:
            raise ValueError(f"unknown ProposalConfig field(s) {unknown}; known: {sorted(names)}")
        if isinstance(overrides.get("snap"), dict):
            from .superpoints import SuperpointConfig
            try:
                overrides = dict(overrides, snap=SuperpointConfig(**overrides["snap"]))
            except TypeError as e:
                raise ValueError(f"ProposalConfig.snap: {e}") from None
        return cls(**overrides).validate()


@dataclass
class DeviceProposals:
    """One cloud's candidates and decisions, all on the device and not yet compacted (nothing here has synchronised with the host)."""
    n_points: int
    masks_per_prompt: int
    bits: torch.Tensor          # [K, W] int64 words
    score: torch.Tensor         # [K] f32: the decoder's IoU prediction
    area: torch.Tensor          # [K] int32 at mask_threshold
    area_hi: torch.Tensor       # [K] int32 at mask_threshold + stability_offset
    area_lo: torch.Tensor       # [K] int32 at mask_threshold - stability_offset
    order: torch.Tensor         # [K] int32: candidates by descending score, ties by index
    valid: torch.Tensor         # [K] uint8
    keep: torch.Tensor          # [K] uint8
    labels: torch.Tensor        # [N] int32
    changed: Optional[torch.Tensor] = None      # [K] uint8: the clean-up or the snap altered the row; None with min_region_points == 0 and no snap (bits / area are then raw)


@dataclass
class Proposals:
    """The kept masks of one cloud, best first.  All tensors live on the device."""
    n_points: int
    bits: torch.Tensor          # [k, W] int64: 64 points per word (the library's uint64_t words, carried as torch.int64)
    candidate: torch.Tensor     # [k] int64: masks_per_prompt * prompt + mask
    prompt_index: torch.Tensor  # [k] int64
    score: torch.Tensor         # [k] f32
    area: torch.Tensor          # [k] int32
    stability: torch.Tensor     # [k] f32: area_hi / area_lo
    labels: torch.Tensor        # [N] int32: row of the best kept mask that contains the point, -1 if none
    # [k] int64, multi-crop proposals only: the crop a mask came from, -1 = the whole scene (merge_proposals).  Keyword-only, so the positional
    # constructor still ends with `changed`
    crop_index: Optional[torch.Tensor] = dataclasses.field(default=None, kw_only=True)
    changed: Optional[torch.Tensor] = None      # [k] uint8: the clean-up or the snap altered the mask; None with min_region_points == 0 and no snap

    def __len__(self) -> int:
        return self.bits.shape[0]

    def masks(self) -> torch.Tensor:
        """[k, N] bool, unpacked on demand."""
        return ops.mask_unpack(self.bits, self.n_points)


@dataclass
class CropLayerConfig:
    """Multi-crop proposals (``predictor.generate_masks(cfg, crops=...)``, SAM's ``crop_n_layers`` for a scan): after the proposals of the whole
    scene, ``num_crops`` balls of radius ``radius`` (scan units) around the first FPS samples of the scene's working cloud each get a crop cloud of at
    most ``max_points`` points, their own encoder pass and their own proposals; a crop's mask that touches the ball's outer shell (a point farther
    than ``(1 - edge_frac) * radius`` from the centre) is dropped as probably truncated, and the rest is merged with the scene's by one more
    suppression at ``nms_thresh``."""
    num_crops: int
    radius: float
    max_points: int = 32768
    edge_frac: float = 0.05
    nms_thresh: float = 0.7

    def validate(self) -> "CropLayerConfig":
        for name in ("num_crops", "max_points"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"CropLayerConfig.{name} must be a positive integer, got {v!r}")
        for name in ("radius", "edge_frac", "nms_thresh"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v) or math.isinf(v):
                raise ValueError(f"CropLayerConfig.{name} must be a finite number, got {v!r}")
        if self.radius <= 0:
            raise ValueError(f"CropLayerConfig.radius must be positive, got {self.radius}")
        if not 0.0 <= self.edge_frac < 1.0:
            raise ValueError(f"CropLayerConfig.edge_frac is a fraction of the radius: it must lie in [0, 1), got {self.edge_frac}")
        if not 0.0 <= self.nms_thresh <= 1.0:
            raise ValueError(f"CropLayerConfig.nms_thresh is an IoU: it must lie in [0, 1], got {self.nms_thresh}")
        return self

    @classmethod
    def from_overrides(cls, overrides: dict) -> "CropLayerConfig":
        """The defaults with the given fields replaced (num_crops and radius have none); an unknown or missing field is a ValueError."""
        names = {f.name for f in dataclasses.fields(cls)}
        unknown = sorted(set(overrides) - names)
        if unknown:
            raise ValueError(f"unknown CropLayerConfig field(s) {unknown}; known: {sorted(names)}")
        missing = sorted({"num_crops", "radius"} - set(overrides))
        if missing:
            raise ValueError(f"CropLayerConfig needs {missing}")
        return cls(**overrides).validate()


@torch.no_grad()
def merge_proposals(layers, n_points: int, nms_thresh: float) -> Proposals:
    """Proposals of the whole scene and of crops, all already at the scan's width, -> one `Proposals`.  layers: [(crop index, Proposals)] in the order
    base (-1), crop 0, crop 1, ...; the rows are concatenated in that order, ordered by score (descending, stable: on a tie the earlier layer wins),
    all taken as valid (every layer applied its own filters), suppressed greedily on mask IoU at `nms_thresh` and painted.  ``crop_index`` names each
    kept mask's layer; ``candidate`` / ``prompt_index`` stay those of its own layer.  Holds K * n_points / 8 bytes of bits and a K x K int32
    intersection matrix for the K concatenated rows; ValueError when K exceeds MAX_CANDIDATES."""
    if not layers:
        raise ValueError("merge_proposals: no layer")
    K = sum(len(p) for _, p in layers)
    if K > MAX_CANDIDATES:
        raise ValueError(f"{K} masks over {len(layers)} layers exceed the {MAX_CANDIDATES} one suppression handles")
    W = ops.mask_words(n_points)
    for _, p in layers:
        if p.n_points != n_points or p.bits.shape[1] != W:
            raise ValueError(f"merge_proposals: a layer of {p.n_points} points among layers of {n_points}")
    first = layers[0][1]
    dev = first.bits.device
    cat = lambda name: torch.cat([getattr(p, name) for _, p in layers])
    bits, score, area = cat("bits").contiguous(), cat("score").contiguous(), cat("area").contiguous()
    origin = torch.cat([torch.full((len(p),), int(ci), dtype=torch.int64, device=dev) for ci, p in layers])
    changed = cat("changed") if all(p.changed is not None for _, p in layers) else None
    if K == 0:
        return Proposals(n_points, bits, cat("candidate"), cat("prompt_index"), score, area, cat("stability"),
                         torch.full((n_points,), -1, dtype=torch.int32, device=dev), changed, crop_index=origin)
    order = torch.sort(score, descending=True, stable=True).indices.to(torch.int32)
    valid = torch.ones(K, dtype=torch.uint8, device=dev)
    inter = ops.mask_intersections(bits)
    keep = ops.mask_nms(order, valid, area, inter, nms_thresh)
    labels = ops.mask_paint(bits, order, keep, n_points)
    sel = order.long()
    sel = sel[keep[sel].bool()]
    return Proposals(n_points, bits[sel], cat("candidate")[sel], cat("prompt_index")[sel], score[sel], area[sel], cat("stability")[sel], labels,
                     None if changed is None else changed[sel], crop_index=origin[sel])


@torch.no_grad()
def build_region_graphs(state, cfg: ProposalConfig):
    """One `regions.PointGraph` per cloud of the state (None with min_region_points == 0).  Synchronises with the host: the voxel counts."""
    if cfg.min_region_points == 0:
        return None
    from .regions import build_graph
    return [build_graph(state.coords[b], cfg.region_voxel_size or None, cfg.region_points_per_voxel) for b in range(state.coords.shape[0])]


@torch.no_grad()
def build_snap_superpoints(state, cfg: ProposalConfig):
    """One `superpoints.Superpoints` per cloud of the state (None with cfg.snap None).  Synchronises with the host: voxel and superpoint counts."""
    if cfg.snap is None:
        return None
    from .regions import build_graph
    from .superpoints import build_superpoints
    out = []
    for b in range(state.coords.shape[0]):
        xyz = state.coords[b].contiguous()
        out.append(build_superpoints(build_graph(xyz, cfg.snap.voxel_size, cfg.snap.points_per_voxel), xyz, cfg.snap))
    return out


@torch.no_grad()
def propose_on_device(model, state, cfg: ProposalConfig, graphs=None, superpoints=None) -> List[DeviceProposals]:
    """Every kernel of generate_proposals, no host synchronisation: capturable in a HIP graph.  graphs: build_region_graphs(state, cfg), needed
    (ValueError without) when cfg.min_region_points > 0 -- building them reads voxel counts on the host, so it is not done here.  superpoints:
    build_snap_superpoints(state, cfg), needed likewise when cfg.snap is set."""
    cfg.validate()
    coords = state.coords
    B, N, _ = coords.shape
    if cfg.snap is not None and (superpoints is None or len(superpoints) != B):
        raise ValueError(f"snap needs the superpoints of every cloud (build_snap_superpoints): got "
                         f"{'none' if superpoints is None else len(superpoints)} for {B} cloud(s)")
    if cfg.min_region_points > 0 and (graphs is None or len(graphs) != B):
        raise ValueError(f"min_region_points = {cfg.min_region_points} needs one region graph per cloud (build_region_graphs): got "
                         f"{'none' if graphs is None else len(graphs)} for {B} cloud(s)")
    P, chunk = cfg.num_prompts, cfg.prompt_chunk
    if P > N:
        raise ValueError(f"num_prompts {P} exceeds the cloud's {N} points")
    dev = coords.device
    _, prompts = ops.fps(coords, P)                       # [B, P, 3]; FPS from index 0, the tokenizer's own sampler
    bufs, scores, C = None, None, None
    for m0 in range(0, P, chunk):
        c = min(chunk, P - m0)
        pts = prompts[:, m0:m0 + c].reshape(B * c, 1, 3)  # cloud-major: row = b * c + m
        logits, iou = model.decode(state, pts, torch.ones(B * c, 1, dtype=torch.int64, device=dev), None, True)
        if bufs is None:
            C = logits.shape[1]
            K = C * P
            if K > MAX_CANDIDATES:
                raise ValueError(f"{K} candidates per cloud ({P} prompts x {C} masks) exceed {MAX_CANDIDATES}")
            W = ops.mask_words(N)
            bufs = [(torch.empty(K, W, dtype=torch.int64, device=dev),) + tuple(torch.empty(K, dtype=torch.int32, device=dev) for _ in range(3))
                    for _ in range(B)]
            scores = torch.empty(B, K, dtype=torch.float32, device=dev)
        for b in range(B):      # cloud b's [c, C, N] slice of the chunk -> rows C * m0 .. of its bit buffer; the logits are dropped after this
            ops.mask_pack(logits[b * c:(b + 1) * c], cfg.mask_threshold, cfg.stability_offset, out=bufs[b], row=C * m0)
        scores[:, C * m0:C * (m0 + c)] = iou.reshape(B, c * C)
        del logits, iou
    out = []
    for b in range(B):
        bits, area, area_hi, area_lo = bufs[b]
        score = scores[b]
        order = torch.sort(score, descending=True, stable=True).indices.to(torch.int32)
        changed = None
        if cfg.min_region_points > 0:      # only rows that pass the score and stability cuts are worth cleaning; the others are copied
            from .regions import RegionConfig, clean_bits
            select = ops.mask_valid(area, area_hi, area_lo, score, N, 0, 2.0, cfg.pred_iou_thresh, cfg.stability_thresh)
            bits, area, changed = clean_bits(graphs[b], bits, select=select,
                                             cfg=RegionConfig(min_island=cfg.min_region_points, min_hole=cfg.min_region_points))
        if cfg.snap is not None:
            from .superpoints import snap_bits
            bits, area, snapped = snap_bits(superpoints[b], bits)
            changed = snapped if changed is None else changed | snapped
        valid = ops.mask_valid(area, area_hi, area_lo, score, N, cfg.min_points, cfg.max_area_frac, cfg.pred_iou_thresh, cfg.stability_thresh)
        inter = ops.mask_intersections(bits)
        keep = ops.mask_nms(order, valid, area, inter, cfg.nms_thresh)
        labels = ops.mask_paint(bits, order, keep, N)
        out.append(DeviceProposals(N, C, bits, score, area, area_hi, area_lo, order, valid, keep, labels, changed))
    return out


def compact(d: DeviceProposals) -> Proposals:
    """The kept rows, best first.  The boolean index is the one host synchronisation of a cloud."""
    order = d.order.long()
    cand = order[d.keep[order].bool()]
    return Proposals(d.n_points, d.bits[cand], cand, cand // d.masks_per_prompt, d.score[cand], d.area[cand],
                     d.area_hi[cand].float() / d.area_lo[cand].float(), d.labels, None if d.changed is None else d.changed[cand])


@torch.no_grad()
def generate_proposals(model, state, cfg: ProposalConfig = None) -> List[Proposals]:
    """One `Proposals` per cloud of the encoder state.  Peak memory: one chunk of logits ([B * prompt_chunk, 3, N] f32), K * N / 8 bytes of
    bits and the K x K int32 intersection matrix per cloud (K = 3 * num_prompts) -- never K * N floats."""
    cfg = (cfg or ProposalConfig()).validate()
    dev = propose_on_device(model, state, cfg, build_region_graphs(state, cfg), build_snap_superpoints(state, cfg))
    out = [compact(d) for d in dev]
    model.check_coordinate_range()
    return out
