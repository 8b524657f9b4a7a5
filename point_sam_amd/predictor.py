"""The predictor the reference's demo calls but never defines (demo/app.py:198-205; README.md:41 points at a
sibling repo): ``set_pointcloud`` / ``set_prompts`` / ``predict_masks``.

Contract inferred from the call sites:
    sam.set_pointcloud(pc_xyz[B,N,3], pc_rgb[B,N,3])
    mask, scores, logits = sam.predict_masks(prompt_points[B,P,3], prompt_labels[B,P], prompt_mask|None, multimask: bool)
    prompt_mask = logits[0][argmax(scores[0])][None]; segment = mask[0][argmax(scores[0])] > 0

The encoder state is cached per cloud (the demo calls set_pointcloud on EVERY click, app.py:199), so clicks after
the first run the decoder only -- BASELINE config #5's "encoder cached, decoder-only loop".
"""
from typing import Optional

import torch

from . import ops
from .config import ModelConfig, get_config
from .model import EncoderState, PointCloudSAM
from .weights import load_safetensors, random_state_dict


class PointSAMPredictor:
    def __init__(self, model: PointCloudSAM):
        self.model = model
        self._state: Optional[EncoderState] = None
        self._key = None
        self._prompts = None
        self.scene = None               # set_scene(): the scan <-> working-cloud mapping (point_sam_amd/scene.py); None after set_pointcloud()
        self._graphs = None             # clean_masks(): (key, [regions.PointGraph per cloud]) of the cached cloud and voxel settings

    @classmethod
    def from_config(cls, name: str, ckpt_path: str = None, num_groups: int = None, group_size: int = None, seed: int = 42,
                    device="cuda", precision: str = "f16x3") -> "PointSAMPredictor":
        cfg: ModelConfig = get_config(name, num_groups, group_size)
        sd = load_safetensors(cfg, ckpt_path) if ckpt_path else random_state_dict(cfg, seed)
        from .variants import build_model      # cfg.variant: PointCloudSAM | PointCloudSAMNN (voronoi) | PointCloudSAMHier
        return cls(build_model(cfg, sd, device, precision=precision))

    # -- state ---------------------------------------------------------------------------------------------
    @staticmethod
    def _cloud_key(xyz, rgb):
        return (xyz.data_ptr(), rgb.data_ptr(), tuple(xyz.shape), xyz._version, rgb._version)

    @torch.no_grad()
    def set_pointcloud(self, xyz: torch.Tensor, rgb: torch.Tensor) -> None:
        """Runs the encoder unless this exact cloud tensor is already cached."""
        if xyz.dim() == 2:
            xyz, rgb = xyz[None], rgb[None]
        g = self.model.pc_encoder.patch_embed.grouper
        key = self._cloud_key(xyz, rgb) + (g.num_groups, g.group_size)
        if key != self._key:
            self._state = self.model.encode(xyz, rgb)
            self._key = key
            self._keepalive = (xyz, rgb)  # the cache key uses data_ptr: keep the tensors alive
            self.scene = None

    @torch.no_grad()
    def set_scene(self, xyz: torch.Tensor, rgb: torch.Tensor, voxel_size: float = None, max_points: int = None) -> None:
        """A full-resolution scan, xyz / rgb [M, 3] normalised as for set_pointcloud, served through a voxel-grid working cloud: one real point per
        occupied voxel of size `voxel_size`, or of the smallest ladder size that leaves at most `max_points` (scene.choose_voxel_size); a scan of at
        most `max_points` points is its own working cloud.  predict_masks / generate_masks then answer per point of the scan.  Cached like
        set_pointcloud; `self.scene` holds keep_idx, inv and num_working."""
        from . import scene as S
        xyz, rgb = S.check_scene_arguments(xyz, rgb, voxel_size, max_points)
        g = self.model.pc_encoder.patch_embed.grouper
        key = self._cloud_key(xyz, rgb) + (g.num_groups, g.group_size, "scene", voxel_size, max_points)
        if key != self._key:
            sc = S.build_scene(xyz, voxel_size, max_points)
            wx, wr = (xyz, rgb) if sc.identity else (xyz.index_select(0, sc.keep_idx), rgb.index_select(0, sc.keep_idx))
            self._state = self.model.encode(wx[None], wr[None])
            self._key = key
            self._keepalive = (xyz, rgb)
            self.scene = sc

    def set_prompts(self, prompt_points, prompt_labels, prompt_mask=None) -> None:
        self._prompts = (prompt_points, prompt_labels, prompt_mask)

    @torch.no_grad()
    def predict_masks(self, prompt_points=None, prompt_labels=None, prompt_mask=None, multimask_output: bool = True):
        """-> (masks [BM,C,N] logits, scores [BM,C], logits [BM,C,N]); masks and logits are the same tensor, the
        caller thresholds at 0 (demo/app.py:203-205).  After set_scene: N = the scan's points; a prompt_mask may have the scan's or the working
        cloud's width."""
        if self._state is None:
            raise RuntimeError("call set_pointcloud() first")
        if prompt_points is None:
            if self._prompts is None:
                raise RuntimeError("no prompts: pass them or call set_prompts() first")
            prompt_points, prompt_labels, prompt_mask = self._prompts
        sc = self.scene
        if sc is not None:
            from .scene import reduce_prompt_mask
            prompt_mask = reduce_prompt_mask(sc, prompt_mask)
        logits, scores = self.model.decode(self._state, prompt_points, prompt_labels, prompt_mask, multimask_output)
        self.model.check_coordinate_range()
        if sc is not None and not sc.identity:
            logits = ops.scene_expand_rows(logits, sc.inv)       # [M', C, num_working] -> [M', C, M]: each point takes its representative's logit
        return logits, scores, logits

    @torch.no_grad()
    def generate_masks(self, cfg=None):
        """Automatic mask proposals for the cached cloud(s), no prompts needed (point_sam_amd/proposals.py): a list with one `Proposals` per
        cloud -- kept masks best first, bit-packed, and one instance label per point.  cfg: a `ProposalConfig` (None = its defaults).
        Works for every model variant (voronoi, hierarchical): only the public `decode` is called, with single-point prompts and no mask prompt."""
        if self._state is None:
            raise RuntimeError("call set_pointcloud() first")
        from .proposals import generate_proposals
        out = generate_proposals(self.model, self._state, cfg)
        if self.scene is not None:
            from .scene import expand_proposals
            out = [expand_proposals(self.scene, p) for p in out]
        return out

    # -- connected-component clean-up ------------------------------------------------------------------------
    def _region_graphs(self, cfg):
        """One neighbourhood graph per cached cloud, rebuilt when the cloud or the voxel settings change."""
        from .regions import build_graph
        key = (self._key, cfg.voxel_size, cfg.points_per_voxel)
        if self._graphs is None or self._graphs[0] != key:
            coords = self._state.coords
            self._graphs = (key, [build_graph(coords[b], cfg.voxel_size, cfg.points_per_voxel) for b in range(coords.shape[0])])
        return self._graphs[1]

    @torch.no_grad()
    def clean_masks(self, logits: torch.Tensor, cfg, prompt_points=None, prompt_labels=None, threshold: float = 0.0):
        """Masks ``logits > threshold`` of the cached cloud with small holes filled, small islands removed and, with ``cfg.keep_clicked``, only the
        parts that hang together with a positive click kept (point_sam_amd/regions.py; cfg: a `RegionConfig`).

        logits [BM, C, N] as predict_masks returns them -> (bits [K, W] int64 words, area [K] int32, changed [K] uint8), K = BM * C rows in the
        logits' order; ``ops.mask_unpack(bits, N)`` gives booleans.  keep_clicked: the seeds of a row are the cloud points nearest to the positive
        prompts (label 1) of its prompt set, prompt_points [BM, P, 3] / prompt_labels [BM, P] (default: those of set_prompts); the C masks of a
        prompt set share them.  After set_scene, logits of the scan's width are reduced to the working cloud (the representatives' values), cleaned
        there and expanded, so every scan point has its representative's bit; logits of the working cloud's width are returned at that width."""
        if self._state is None:
            raise RuntimeError("call set_pointcloud() first")
        from .regions import RegionConfig, clean_bits
        if not isinstance(cfg, RegionConfig):
            raise TypeError(f"clean_masks: cfg must be a RegionConfig, got {type(cfg).__name__}")
        cfg.validate()
        coords = self._state.coords
        B, Nw, _ = coords.shape
        if logits.dim() != 3 or logits.shape[0] % B != 0:
            raise ValueError(f"clean_masks: logits must be [BM, C, N] with BM a multiple of the {B} cached cloud(s), got {tuple(logits.shape)}")
        sc = self.scene if self.scene is not None and not self.scene.identity else None
        expand = sc is not None and logits.shape[-1] == sc.num_points and sc.num_points != Nw
        if expand:
            logits = logits.index_select(-1, sc.keep_idx)
        if logits.shape[-1] != Nw:
            raise ValueError(f"clean_masks: logits of width {logits.shape[-1]} do not fit the cached cloud's {Nw} points")
        BM, C, _ = logits.shape
        Mp = BM // B
        seeds = None
        if cfg.keep_clicked:
            if prompt_points is None:
                if self._prompts is None:
                    raise RuntimeError("keep_clicked needs the prompts: pass them or call set_prompts() first")
                prompt_points, prompt_labels = self._prompts[0], self._prompts[1]
            P = prompt_points.shape[-2]
            pts = prompt_points.to(coords.device, torch.float32).reshape(B, Mp * P, 3).contiguous()
            near = ops.knn(pts, coords.contiguous(), 1).reshape(BM, P)                      # the nearest cloud point of every prompt
            positive = prompt_labels.to(coords.device).reshape(BM, P) == 1
            seeds = torch.where(positive, near, torch.full_like(near, -1)).to(torch.int32)
            seeds = seeds.repeat_interleave(C, dim=0).contiguous()                          # every mask of a prompt set shares its seeds
        bits, _, _, _ = ops.mask_pack(logits.float().contiguous(), threshold, 0.0)
        graphs = self._region_graphs(cfg)
        rows = Mp * C
        out = [clean_bits(graphs[b], bits[b * rows:(b + 1) * rows], seeds=None if seeds is None else seeds[b * rows:(b + 1) * rows], cfg=cfg)
               for b in range(B)]
        bits, area, changed = (torch.cat([o[i] for o in out]) if B > 1 else out[0][i] for i in range(3))
        if expand:
            bits, area = ops.scene_expand_bits(bits.contiguous(), sc.inv, Nw)
        return bits, area, changed
