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

import numpy as np
import torch

from . import ops
from .config import ModelConfig, get_config
from .model import EncoderState, PointCloudSAM
from .weights import load_safetensors, random_state_dict


_UNBUILT = object()      # an interpolation plan not asked for yet (None is a built answer: the mapping has nothing to blend)


def _check_smooth(smooth, what: str, allow_none: bool = False):
    if not (isinstance(smooth, bool) or (allow_none and smooth is None)):
        raise ValueError(f"{what}: smooth must be True or False{' or None' if allow_none else ''}, got {smooth!r}")
    return smooth


class PointSAMPredictor:
    def __init__(self, model: PointCloudSAM):
        self.model = model
        self._state: Optional[EncoderState] = None
        self._key = None
        self._prompts = None
        self.scene = None               # set_scene(): the scan <-> working-cloud mapping (point_sam_amd/scene.py); None after set_pointcloud()
        self.crop = None                # set_crop(): the scan <-> crop-cloud mapping of the active ball (scene.Crop); None = the whole scene answers
        self._crop_state: Optional[EncoderState] = None      # the crop cloud's encoder state; self._state stays the scene's, so clear_crop() re-encodes nothing
        self._crop_key = None
        self._crop_cache = None         # [key, Crop, state, plan] of the last crop built: survives clear_crop() and a set_scene() of the same scene
        self._smooth = False            # set_scene(smooth=): scan points receive a 3-NN blend of working logits, not their representative's
        self._crop_smooth = False       # the same for the active crop (set_crop(smooth=None) takes the scene's setting)
        self._scene_plan = _UNBUILT     # scene.InterpPlan of the cached scene (None: nothing to blend), built by the first predict that needs it
        self._graphs = None             # clean_masks(): (key, [regions.PointGraph per cloud]) of the cached cloud and voxel settings
        self._superpoints = (None, {})  # superpoints(): (the cloud's key, {(cloud, settings): PointGraph or Superpoints}) -- dropped with the cloud

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
            self._crop_cache = None
            self._scene_plan = _UNBUILT
        self._smooth = False
        self._deactivate_crop()

    @torch.no_grad()
    def set_scene(self, xyz: torch.Tensor, rgb: torch.Tensor, voxel_size: float = None, max_points: int = None, smooth: bool = False) -> None:
        """A full-resolution scan, xyz / rgb [M, 3] normalised as for set_pointcloud, served through a voxel-grid working cloud: one real point per
        occupied voxel of size `voxel_size`, or of the smallest ladder size that leaves at most `max_points` (scene.choose_voxel_size); a scan of at
        most `max_points` points is its own working cloud.  predict_masks / generate_masks then answer per point of the scan.  Cached like
        set_pointcloud; `self.scene` holds keep_idx, inv and num_working.

        smooth: predict_masks / predict_mask_bits give every scan point the inverse-distance blend of the up to three nearest working points among
        its voxel's and the 26 surrounding voxels' representatives (scene.build_interp_plan) instead of its representative's logit; the
        representatives themselves keep their logits bit for bit.  Not part of the cache key: toggling it encodes nothing; the plan (24 bytes per
        scan point) is built by the first prediction that needs it and kept with the scene."""
        from . import scene as S
        _check_smooth(smooth, "set_scene")
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
            self._crop_cache = None
            self._scene_plan = _UNBUILT
        self._smooth = smooth
        self._deactivate_crop()

    def _deactivate_crop(self) -> None:
        self.crop, self._crop_state, self._crop_key, self._crop_smooth = None, None, None, False

    @torch.no_grad()
    def set_crop(self, center, radius: float, voxel_size: float = None, max_points: int = None, smooth: bool = None) -> None:
        """Zoom into the ball (center, radius) of the scan given to set_scene (scan coordinates): its points, normalised to (x - center) / radius, get
        a working cloud of their own -- one real point per voxel of size `voxel_size` (crop units), or of the smallest ladder size that leaves at most
        `max_points`; neither: every point of the ball -- and their own encoder pass (scene.build_crop).  Until clear_crop(), predict_masks /
        generate_masks / clean_masks answer from the crop cloud, still per point of the scan and with prompts in scan coordinates: -inf logits, zero
        bits and label -1 outside the ball.  The scene's encoder state is kept.  set_scene and set_pointcloud drop the crop.  The last crop built is
        cached on (scene, center, radius, voxel_size, max_points): setting it again, also after clear_crop() or a set_scene() of the same scene,
        builds and encodes nothing.  `self.crop` holds keep_idx, inv, num_members and num_working.

        smooth: as for set_scene, over the crop's own voxel grid (None: the scene's setting); not part of the crop's cache key, and the plan is
        cached with the crop."""
        _check_smooth(smooth, "set_crop", allow_none=True)
        if self.scene is None or self._state is None:
            raise RuntimeError("set_crop() zooms into a scene: call set_scene() first")
        from . import scene as S
        key = (self._key, tuple(float(v) for v in center), float(radius), voxel_size, max_points)
        if self._crop_cache is None or self._crop_cache[0] != key:
            xyz, rgb = self._keepalive
            crop, wxyz, wrgb = S.build_crop(xyz, rgb, center, radius, voxel_size, max_points)
            self._crop_cache = [key, crop, self.model.encode(wxyz[None], wrgb[None]), _UNBUILT]
        self._crop_key, self.crop, self._crop_state = self._crop_cache[:3]
        self._crop_smooth = self._smooth if smooth is None else smooth

    def clear_crop(self) -> None:
        """Back to the whole scene: its encoder state was kept, nothing is encoded again."""
        self._deactivate_crop()

    def _active(self):
        """(encoder state, mapping, cache key) that answer now: the crop's while one is set, else the scene's (mapping None after set_pointcloud)."""
        if self.crop is not None:
            return self._crop_state, self.crop, self._crop_key
        return self._state, self.scene, self._key

    def _interp_plan(self):
        """The active mapping's interpolation plan if smooth edges are on and there is something to blend, else None.  Built on first use."""
        from .scene import build_interp_plan
        xyz = self._keepalive[0]
        if self.crop is not None:
            if not self._crop_smooth:
                return None
            if self._crop_cache[3] is _UNBUILT:
                self._crop_cache[3] = build_interp_plan(self.crop, xyz, self._crop_state.coords[0].contiguous())
            return self._crop_cache[3]
        if self.scene is None or not self._smooth:
            return None
        if self._scene_plan is _UNBUILT:
            self._scene_plan = build_interp_plan(self.scene, xyz, self._state.coords[0].contiguous())
        return self._scene_plan

    def _decode(self, prompt_points, prompt_labels, prompt_mask, multimask_output):
        """-> (working-width logits, scores, mapping or None, crop?): the part predict_masks and predict_mask_bits share."""
        if self._state is None:
            raise RuntimeError("call set_pointcloud() first")
        if prompt_points is None:
            if self._prompts is None:
                raise RuntimeError("no prompts: pass them or call set_prompts() first")
            prompt_points, prompt_labels, prompt_mask = self._prompts
        state, sc, _ = self._active()
        crop = self.crop is not None
        if sc is not None:
            from .scene import crop_prompts, reduce_prompt_mask
            prompt_mask = reduce_prompt_mask(sc, prompt_mask)
            if crop:
                prompt_points = crop_prompts(sc, prompt_points)     # scan coordinates -> the crop's unit ball; a prompt off the ball is a ValueError
        logits, scores = self.model.decode(state, prompt_points, prompt_labels, prompt_mask, multimask_output)
        self.model.check_coordinate_range()
        return logits, scores, sc, crop

    def set_prompts(self, prompt_points, prompt_labels, prompt_mask=None) -> None:
        self._prompts = (prompt_points, prompt_labels, prompt_mask)

    @torch.no_grad()
    def predict_masks(self, prompt_points=None, prompt_labels=None, prompt_mask=None, multimask_output: bool = True):
        """-> (masks [BM,C,N] logits, scores [BM,C], logits [BM,C,N]); masks and logits are the same tensor, the
        caller thresholds at 0 (demo/app.py:203-205).  After set_scene: N = the scan's points; a prompt_mask may have the scan's or the working
        cloud's width.  Under set_crop: the prompts are still scan coordinates (one outside the ball is a ValueError), the logits are the crop
        cloud's indexed by crop.inv, -inf outside the ball; a prompt_mask may have the scan's or the crop cloud's width.  With smooth edges
        (set_scene / set_crop smooth=True) the logits are the 3-NN blend of the working cloud's; at the representatives they are the working
        cloud's bit for bit, so they serve as the next click's prompt_mask exactly like the working-width logits."""
        logits, scores, sc, crop = self._decode(prompt_points, prompt_labels, prompt_mask, multimask_output)
        logits = self._expand_logits(logits, sc, crop)
        return logits, scores, logits

    def _expand_logits(self, logits, sc, crop):
        """Working-width logits [..., num_working] -> the scan's width [..., M] through the active mapping `sc` (None after set_pointcloud: unchanged)."""
        plan = self._interp_plan()
        if plan is not None:
            logits = ops.scene_interp_rows(logits, plan.idx3, plan.w3, float("-inf") if crop else None)      # [M', C, num_working] -> [M', C, M]
        elif crop:
            logits = ops.crop_expand_rows(logits, sc.inv, float("-inf"))      # [M', C, num_working] -> [M', C, M]; -inf off the ball
        elif sc is not None and not sc.identity:
            logits = ops.scene_expand_rows(logits, sc.inv)       # [M', C, num_working] -> [M', C, M]: each point takes its representative's logit
        return logits

    @torch.no_grad()
    def predict_mask_bits(self, prompt_points=None, prompt_labels=None, prompt_mask=None, multimask_output: bool = True, threshold: float = 0.0):
        """predict_masks for a caller that wants the masks, not the logits: -> (bits [BM * C, W] int64 words of ``logit > threshold`` in mask_pack's
        layout, W = ceil(N / 64); area [BM * C] int32; scores [BM, C]).  The same bits as mask_pack of predict_masks' logits, without the
        [BM, C, N] floats of a scan: with smooth edges the blend is thresholded in registers (ops.scene_interp_bits), otherwise the working
        cloud's packed rows are expanded (scene_expand_bits / crop_expand_bits); after set_pointcloud it is mask_pack alone."""
        logits, scores, sc, crop = self._decode(prompt_points, prompt_labels, prompt_mask, multimask_output)
        logits = logits.float().contiguous()
        plan = self._interp_plan()
        if plan is not None:
            bits, area = ops.scene_interp_bits(logits, plan.idx3, plan.w3, threshold)
            return bits, area, scores
        bits, area, _, _ = ops.mask_pack(logits, threshold, 0.0)
        if crop:
            bits, area = ops.crop_expand_bits(bits, sc.inv, sc.num_working)
        elif sc is not None and not sc.identity:
            bits, area = ops.scene_expand_bits(bits, sc.inv, sc.num_working)
        return bits, area, scores

    # -- from one scan to the next (point_sam_amd/transfer.py) ------------------------------------------------
    def _transfer_cloud(self, what: str):
        """(encoder state, scene or None) of the one cloud that snapshot / transfer_masks / propagate work on."""
        if self._state is None:
            raise RuntimeError(f"{what}: call set_scene() or set_pointcloud() first")
        if self.crop is not None:
            raise RuntimeError(f"{what}: not under a crop (crops are neither source nor destination of a transfer): call clear_crop() first")
        if self._state.coords.shape[0] != 1:
            raise ValueError(f"{what}: one cloud at a time, the cached batch holds {self._state.coords.shape[0]}")
        return self._state, self.scene

    @torch.no_grad()
    def snapshot(self, logits: torch.Tensor, normals=False):
        """What the next scan needs of this one: -> transfer.Snapshot of the working cloud's coordinates as encoded and the K objects' logits at working
        width.  logits [K, n] f32, n the scan's or the working cloud's width; of a scan-width row the representatives' own words are kept (exact, as
        for a prompt_mask).  normals: True, or a superpoints.SuperpointConfig (its voxel settings and min_points), also keeps the voxel normal of
        every working point -- point_normals(cfg=...)[0] at the representatives (scene.keep_idx), or the cloud's own rows without a scene -- which
        align(plane=...) needs; no host read beyond point_normals'.  RuntimeError before any cloud is set and under an active crop."""
        from . import transfer as T
        from .scene import reduce_prompt_mask
        state, sc = self._transfer_cloud("snapshot")
        Nw = state.coords.shape[1]
        logits = T.check_snapshot_logits(logits, (Nw,) if sc is None else (Nw, sc.num_points), "snapshot")
        if sc is not None:
            logits = reduce_prompt_mask(sc, logits)
        kept = None
        if normals is not False and normals is not None:
            kept = self.point_normals(cfg=None if normals is True else normals)[0]      # a TypeError for anything but a SuperpointConfig
            kept = (kept if sc is None else kept.index_select(0, sc.keep_idx)).contiguous()
        return T.Snapshot(state.coords[0].contiguous(), logits.to(self.model.device).contiguous(), logits.shape[0], kept)

    def _scan_xyz(self, state, sc):
        return state.coords[0].contiguous() if sc is None else self._keepalive[0]

    @torch.no_grad()
    def transfer_masks(self, snap, radius: float, pose=None, threshold: float = 0.0):
        """The snapshot's masks at every point of the CURRENT cloud (after set_scene / set_pointcloud of the next scan), without the model: each point
        receives the inverse-distance blend of the up to three snapshot points within `radius` of it (a lone one or an exact hit is copied), a point
        with none is off.  -> (bits [K, W] int64 words of ``blend > threshold`` in mask_pack's layout, W = ceil(M / 64); area [K] int32;
        covered_count, a 0-d int64 device tensor: the points with a snapshot point in reach).  pose: 3 x 4 or 4 x 4, this scan's coordinates -> the
        snapshot's; both scans normalised with the same centre and scale.  No host synchronisation beyond the index build's read of the bounds."""
        from . import transfer as T
        T.check_snapshot(snap, "transfer_masks")
        threshold = T.check_threshold(threshold, "transfer_masks")
        state, sc = self._transfer_cloud("transfer_masks")
        plan = T.build_plan(snap.coords, self._scan_xyz(state, sc), radius, pose)
        bits, area = T.transfer_bits(plan, snap.logits, threshold)
        return bits, area, T.covered(plan).sum()

    @torch.no_grad()
    def align(self, snap, cfg, init=None, mask=None, search=None, plane=None):
        """The pose from the CURRENT cloud to the snapshot's, estimated by ICP (point_sam_amd/align.py) -> align.Alignment; its `pose` is what
        transfer_masks / propagate take.  The sources are the snapshot's working cloud, the queries this cloud's working coordinates as encoded;
        cfg: an align.AlignConfig (its radius is the index's cell size); init: the pose to refine (None: the identity; e.g. odometry); mask: an
        optional packed row [ceil(Nw / 64)] int64 at working width restricting the queries to one object (a re-scan after something moved).
        Exactly align.icp(ops.transfer_index(snap.coords, cfg.radius), working coordinates, cfg, init, mask).  One 160-byte host read per step
        besides the index build's; both scans normalised with the same centre and scale.
        search: None, or an align.SearchConfig for a caller without even a rough pose: a grid of candidate poses is scored in one launch and the best
        few are refined by the same ICP -- exactly align.search(the same index, working coordinates, search, cfg, mask); the Alignment's `search`
        says what was tried.  Its scoring radius may not exceed cfg.radius, and it takes no `init` (ValueError): the search IS the start.
        plane: None, an align.PlaneConfig, or True for its defaults: point-to-plane ICP on the snapshot's normals (snapshot(..., normals=True); a
        ValueError without them) -- exactly align.icp / align.search on the same index with normals=snap.normals, plane=the config: far fewer steps
        where the scans are floors and walls, one 256-byte host read per step."""
        from . import align as A
        from . import transfer as T
        T.check_snapshot(snap, "align")
        if not isinstance(cfg, A.AlignConfig):
            raise TypeError(f"align: cfg must be an align.AlignConfig, got {type(cfg).__name__}")
        normals = None
        if plane is not None:
            plane = A.PlaneConfig() if plane is True else plane
            if not isinstance(plane, A.PlaneConfig):
                raise TypeError(f"align: plane must be an align.PlaneConfig, True or None, got {type(plane).__name__}")
            if snap.normals is None:
                raise ValueError("align: plane needs the snapshot's normals: take it with snapshot(..., normals=True)")
            normals = snap.normals
        if search is not None:
            if not isinstance(search, A.SearchConfig):
                raise TypeError(f"align: search must be an align.SearchConfig or None, got {type(search).__name__}")
            if init is not None:
                raise ValueError("align: init and search exclude each other: a search starts from its own candidates")
            if search.radius is not None and search.radius > cfg.radius:
                raise ValueError(f"align: search.radius {search.radius} exceeds cfg.radius {cfg.radius}, the cell size of the index")
        state, _ = self._transfer_cloud("align")
        if search is not None:
            return A.search(ops.transfer_index(snap.coords, cfg.radius), state.coords[0].contiguous(), search, cfg, mask, normals=normals, plane=plane)
        return A.icp(ops.transfer_index(snap.coords, cfg.radius), state.coords[0].contiguous(), cfg, init, mask, normals=normals, plane=plane)

    @torch.no_grad()
    def propagate(self, snap, radius: float, pose=None, clicks: int = 1, fill=None):
        """The model re-segments every snapshot object in the CURRENT cloud -> transfer.Propagated.  The carried logits (`prior`: the blend of the
        snapshot's logits at this working cloud's points; where no snapshot point is within `radius`, `fill`, or with fill=None the object's own
        minimum snapshot logit -- the model's "most certainly background" for that object) serve as the mask prompt and, thresholded at 0, in place of
        the ground truth of the reference's evaluation loop (pc_sam.py:139-194): click 0 is the deepest point of the carried mask, click i > 0 the
        deepest point of the error of the previous output against it; every decode sees all clicks so far and the previous output (the prior for the
        first) as mask prompt, single-mask output.  An object whose carried mask is empty is `lost`: -inf logits, NaN score, no part in the decode.
        One host read (K + 1 counts) besides the index build's.  pose and normalisation as for transfer_masks.  Nothing here has been tuned on a
        trained checkpoint (none exists offline)."""
        from . import transfer as T
        T.check_snapshot(snap, "propagate")
        T.check_propagate_arguments(clicks, fill)
        state, sc = self._transfer_cloud("propagate")
        model, dev = self.model, self.model.device
        K, Nw = snap.num_masks, state.coords.shape[1]
        plan = T.build_plan(snap.coords, state.coords[0].contiguous(), radius, pose)
        cov = T.covered(plan)
        prior = T.transfer_rows(plan, snap.logits, 0.0)
        outside = snap.logits.amin(dim=1, keepdim=True) if fill is None else torch.full((K, 1), float(fill), dtype=torch.float32, device=dev)
        prior = torch.where(cov[None, :], prior, outside).contiguous()
        gt = prior > 0
        counts = torch.cat([gt.sum(1), cov.sum()[None]]).cpu()                     # the one host read
        prior_area, lost = counts[:K].to(dev), (counts[:K] == 0).to(dev)
        keep = torch.nonzero(counts[:K] > 0)[:, 0].to(dev)
        M = Nw if sc is None else sc.num_points
        out = torch.full((K, M), float("-inf"), dtype=torch.float32, device=dev)
        scores = torch.full((K,), float("nan"), dtype=torch.float32, device=dev)
        points = torch.full((K, clicks, 3), float("nan"), dtype=torch.float32, device=dev)
        labels = torch.zeros(K, clicks, dtype=torch.bool, device=dev)
        if keep.numel() > 0:
            Z = keep.numel()
            truth = gt.index_select(0, keep)[None]                                 # [1, Z, Nw]
            prompt_mask, previous = prior.index_select(0, keep), None
            pc = torch.empty(Z, 0, 3, dtype=torch.float32, device=dev)
            pl = torch.empty(Z, 0, dtype=torch.bool, device=dev)
            for _ in range(clicks):
                nc, nl = model.sample_prompts(state.coords, truth, previous)
                pc, pl = torch.cat([pc, nc], dim=1), torch.cat([pl, nl], dim=1)
                masks, iou = model.decode(state, pc, pl, prompt_mask, multimask_output=False)
                prompt_mask = previous = masks[:, 0].contiguous()
            model.check_coordinate_range()
            out[keep] = self._expand_logits(previous, sc, False)
            scores[keep] = iou[:, 0].float()
            points[keep], labels[keep] = pc, pl
        return T.Propagated(out, scores, lost, prior_area, float(counts[K]) / Nw, points, labels)

    # -- the map the scans accumulate into (point_sam_amd/scanmap.py) ------------------------------------------
    def _map_scan(self, m, what: str):
        """(xyz, rgb) [M, 3] of the CURRENT scan: after set_scene its full-resolution points and colours, otherwise the cloud as encoded."""
        from .scanmap import ScanMap
        if not isinstance(m, ScanMap):
            raise TypeError(f"{what}: m must be a scanmap.ScanMap, got {type(m).__name__}")
        state, sc = self._transfer_cloud(what)
        if sc is not None:
            return self._keepalive[0], self._keepalive[1]
        return state.coords[0].contiguous(), state.features[0].contiguous()

    def new_map(self, voxel_size, max_voxels: int, max_pairs: int = None):
        """An empty scanmap.ScanMap on the model's device."""
        from .scanmap import ScanMap
        return ScanMap(voxel_size, max_voxels, max_pairs, device=self.model.device)

    @torch.no_grad()
    def map_add(self, m, labels: torch.Tensor = None, pose=None):
        """Adds the CURRENT scan to the scanmap.ScanMap `m` -> scanmap.AddResult.  labels [M] int32 at the scan's width (e.g.
        scanmap.labels_from_logits of propagate()'s logits) or None; pose: 3 x 4 or 4 x 4 from this scan's coordinates to the map's (align()'s `pose`
        where the map was begun with the snapshot's scan), None = the identity.  RuntimeError before any cloud is set and under an active crop;
        scanmap.MapOverflow past the map's capacities.  One host read, the map's header."""
        xyz, rgb = self._map_scan(m, "map_add")
        return m.add(xyz, rgb, labels, pose)

    @torch.no_grad()
    def map_carve(self, m, origin, pose=None, margin: int = 1):
        """Carves the free space the CURRENT scan saw through out of `m` (ScanMap.carve) -> scanmap.CarveResult.  origin: the sensor's position in
        this scan's coordinates (three numbers); pose as map_add's.  Call it after map_add of the same scan, from the map's first scan on: hits
        count carves.  One 64-byte host read."""
        xyz, _ = self._map_scan(m, "map_carve")
        return m.carve(xyz, origin, pose, margin)

    @torch.no_grad()
    def map_carve_frames(self, m, fs, pose=None, margin: int = 1) -> list:
        """One carve per frame of a views.FrameSet (set_frames) over that frame's own points -> a list of scanmap.CarveResult, None for a frame
        that kept no pixel.  A frame's points are contiguous in fs.xyz and fs.index[f] names them; its origin is the camera's centre in the
        normalised frame, -R^T t of fs.views[f].camera in fp64, rounded to fp32 once.  One host read for the frames' ranges, then one per carve."""
        from .scanmap import ScanMap
        from .views import FrameSet
        if not isinstance(m, ScanMap):
            raise TypeError(f"map_carve_frames: m must be a scanmap.ScanMap, got {type(m).__name__}")
        if not isinstance(fs, FrameSet):
            raise TypeError(f"map_carve_frames: fs must be a views.FrameSet (set_frames), got {type(fs).__name__}")
        F = fs.index.shape[0]
        idx = fs.index.reshape(F, -1)
        lo = torch.where(idx >= 0, idx, torch.full_like(idx, fs.num_points)).amin(1)
        span = torch.stack([lo, idx.amax(1)]).cpu().tolist()                       # the one host read of the ranges
        out = []
        for f in range(F):
            first, last = span[0][f], span[1][f]
            if last < 0:
                out.append(None)
                continue
            P = fs.views[f].camera.pose.astype(np.float64)
            centre = (-P[:, :3].T @ P[:, 3]).astype(np.float32)
            out.append(m.carve(fs.xyz[first:last + 1], centre, pose, margin))
        return out

    @torch.no_grad()
    def map_lookup(self, m, pose=None, min_votes: int = 1) -> torch.Tensor:
        """Per point of the CURRENT scan the map's voted label at its voxel -> [M] int32, -1 where the map has no voxel there or the voxel no label
        with min_votes votes; all -1 for an empty map.  No host read."""
        xyz, _ = self._map_scan(m, "map_lookup")
        if isinstance(min_votes, bool) or not isinstance(min_votes, int) or not 1 <= min_votes <= 2 ** 31 - 1:
            raise ValueError(f"map_lookup: min_votes must be an integer in 1 .. 2^31 - 1, got {min_votes!r}")
        ids = m.locate(xyz, pose)
        if m.num_voxels == 0:                                      # an empty map has no voxel anywhere: locate's -1 for every point
            return ids
        label = m.labels(min_votes)[0]
        return torch.where(ids >= 0, label.index_select(0, ids.clamp(min=0).long()), torch.full_like(ids, -1))

    @torch.no_grad()
    def map_align(self, m, cfg, init=None, mask=None, occupied=None, min_count: int = 1, normals=None, plane=None):
        """The pose of the CURRENT scan against the scanmap.ScanMap `m` itself, by ICP on the map's own voxels (ScanMap.track) -> align.Alignment; its
        `pose` is what map_add and map_carve take.  The coordinates are the ones map_add would add (after set_scene the full-resolution points).
        Exactly m.track(those, cfg, init, mask, occupied, min_count): cfg an align.AlignConfig with a radius of at most 4 voxels, init the pose to
        refine (odometry, the previous scan's pose, align()'s frame-to-frame estimate), mask an optional packed row [ceil(M / 64)] int64 at the
        scan's width, occupied None / True / a [V] bool tensor.  normals (None, True or a [V, 3] tensor) and plane (an align.PlaneConfig) are
        ScanMap.track's: point-to-plane against the map's own voxel normals.  Frame to model: the error of one scan's pose does not enter the next one's.
        (For a scan without a pose to refine: map_relocalize.)"""
        xyz, _ = self._map_scan(m, "map_align")
        return m.track(xyz, cfg, init, mask, occupied, min_count, normals, plane)

    @torch.no_grad()
    def map_relocalize(self, m, cfg, search, mask=None, occupied=None, min_count: int = 1, normals=None, plane=None):
        """The pose of the CURRENT scan in the scanmap.ScanMap `m` WITHOUT a pose to refine (odometry dropped out, a second session, a scan from
        elsewhere in the map) -> align.Alignment, its `search` the align.SearchRecord.  map_align's arguments with `search`, an align.SearchConfig,
        in the place of `init`: exactly m.relocalize(the coordinates map_add would add, cfg, search, mask, occupied, min_count, normals, plane) -- a
        grid of poses scored on the map's own voxels in one call, the best refined by map_align's loop."""
        from . import align as A
        if not isinstance(search, A.SearchConfig):
            raise TypeError(f"map_relocalize: search must be an align.SearchConfig, got {type(search).__name__}")
        xyz, _ = self._map_scan(m, "map_relocalize")
        return m.relocalize(xyz, cfg, search, mask, occupied, min_count, normals, plane)

    @torch.no_grad()
    def map_view(self, m, camera, occupied=True, min_count: int = 1):
        """The scanmap.ScanMap `m` as `camera` (views.Camera, pose from the map's frame to the camera's, its centre inside [-1, 1]^3) sees it from
        inside -> views.View over the map's voxel ids (ScanMap.view): ray cast through the map's voxels, so without the holes of render_view on
        m.cloud().  occupied=True (the default here) leaves out what carving voted free; None shows every voxel.  Needs no cloud to be set."""
        from .scanmap import ScanMap
        if not isinstance(m, ScanMap):
            raise TypeError(f"map_view: m must be a scanmap.ScanMap, got {type(m).__name__}")
        return m.view(camera, occupied, min_count)

    @torch.no_grad()
    def map_nearest(self, m, pose=None, radius=None, min_votes: int = 1) -> torch.Tensor:
        """map_lookup through the NEAREST voxel within `radius` (None: the voxel size) instead of the point's own: per point of the CURRENT scan the
        voted label of the map voxel whose mean lies nearest to the posed point -> [M] int32, -1 where no voxel is in reach or that voxel has no label
        with min_votes votes.  One ScanMap.track_step(return_nearest=True); ValueError for an empty map.  No host read."""
        xyz, _ = self._map_scan(m, "map_nearest")
        if isinstance(min_votes, bool) or not isinstance(min_votes, int) or not 1 <= min_votes <= 2 ** 31 - 1:
            raise ValueError(f"map_nearest: min_votes must be an integer in 1 .. 2^31 - 1, got {min_votes!r}")
        _, ids = m.track_step(xyz, pose, radius, return_nearest=True)
        label = m.labels(min_votes)[0]
        return torch.where(ids >= 0, label.index_select(0, ids.clamp(min=0).long()), torch.full_like(ids, -1))

    @torch.no_grad()
    def generate_masks(self, cfg=None, crops=None):
        """Automatic mask proposals for the cached cloud(s), no prompts needed (point_sam_amd/proposals.py): a list with one `Proposals` per
        cloud -- kept masks best first, bit-packed, and one instance label per point.  cfg: a `ProposalConfig` (None = its defaults).
        Works for every model variant (voronoi, hierarchical): only the public `decode` is called, with single-point prompts and no mask prompt.
        Under set_crop: the crop cloud's proposals at the scan's width, zero bits and label -1 off the ball.  Proposals keep bits, not logits:
        they stay at voxel granularity whatever `smooth` says.

        crops: a `CropLayerConfig` -- multi-crop proposals of a scene (set_scene, no active crop).  The scene's own proposals first; then, for each
        of the first `num_crops` FPS samples of the scene's working cloud (index 0 first: every centre is a real point), the crop cloud of the ball
        of `crops.radius` around it (at most `crops.max_points` points), its encoder pass and its proposals under the same `cfg`; a crop's mask
        with a point in the ball's outer shell (scene.crop_shell_bits) is dropped -- a truncated object is the scene's or another crop's to find
        -- and the others are expanded to the scan; proposals.merge_proposals then orders all rows by score, suppresses at `crops.nms_thresh` and
        paints.  The result's `crop_index` names each mask's origin (-1 = the scene).  The merge holds K * M / 8 bytes of bits and a K x K int32
        matrix for the K rows of all layers together (at most proposals.MAX_CANDIDATES, else ValueError); the crops' encoder states are not kept."""
        if self._state is None:
            raise RuntimeError("call set_pointcloud() first")
        from .proposals import generate_proposals
        from .scene import expand_proposals
        if crops is not None:
            return [self._generate_masks_multicrop(cfg, crops)]
        state, sc, _ = self._active()
        out = generate_proposals(self.model, state, cfg)
        if sc is not None:
            out = [expand_proposals(sc, p) for p in out]
        return out

    def _generate_masks_multicrop(self, cfg, crops):
        import dataclasses
        from . import scene as S
        from .proposals import CropLayerConfig, generate_proposals, merge_proposals
        if not isinstance(crops, CropLayerConfig):
            raise TypeError(f"generate_masks: crops must be a CropLayerConfig, got {type(crops).__name__}")
        crops.validate()
        if self.scene is None:
            raise RuntimeError("multi-crop proposals need a scene: call set_scene() first")
        if self.crop is not None:
            raise RuntimeError("multi-crop proposals run on the whole scene: call clear_crop() first")
        sc = self.scene
        if crops.num_crops > sc.num_working:
            raise ValueError(f"num_crops {crops.num_crops} exceeds the scene's {sc.num_working} working points")
        xyz, rgb = self._keepalive
        layers = [(-1, S.expand_proposals(sc, generate_proposals(self.model, self._state, cfg)[0]))]
        _, centers = ops.fps(self._state.coords.contiguous(), crops.num_crops)             # [1, num_crops, 3]: points of the working cloud, hence of the scan
        for ci, center in enumerate(centers[0].cpu().tolist()):
            crop, wxyz, wrgb = S.build_crop(xyz, rgb, center, crops.radius, max_points=crops.max_points)
            p = generate_proposals(self.model, self.model.encode(wxyz[None], wrgb[None]), cfg)[0]
            if len(p) > 0:
                touches = ops.mask_intersections(p.bits.contiguous(), S.crop_shell_bits(crop, xyz, crops.edge_frac))[:, 0] > 0
                inside = torch.nonzero(~touches)[:, 0]
                p = dataclasses.replace(p, **{name: getattr(p, name).index_select(0, inside)
                                              for name in ("bits", "candidate", "prompt_index", "score", "area", "stability", "changed")
                                              if getattr(p, name) is not None})
            layers.append((ci, S.expand_proposals(crop, p)))
        return merge_proposals(layers, sc.num_points, crops.nms_thresh)

    # -- connected-component clean-up ------------------------------------------------------------------------
    def _region_graphs(self, cfg):
        """One neighbourhood graph per cached cloud, rebuilt when the cloud or the voxel settings change."""
        from .regions import build_graph
        state, _, cloud_key = self._active()                         # under set_crop the graph is the crop cloud's: its key names the crop
        key = (cloud_key, cfg.voxel_size, cfg.points_per_voxel)
        if self._graphs is None or self._graphs[0] != key:
            coords = state.coords
            self._graphs = (key, [build_graph(coords[b], cfg.voxel_size, cfg.points_per_voxel) for b in range(coords.shape[0])])
        return self._graphs[1]

    @torch.no_grad()
    def clean_masks(self, logits: torch.Tensor, cfg, prompt_points=None, prompt_labels=None, threshold: float = 0.0):
        """Masks ``logits > threshold`` of the cached cloud with small holes filled, small islands removed and, with ``cfg.keep_clicked``, only the
        parts that hang together with a positive click kept (point_sam_amd/regions.py; cfg: a `RegionConfig`).

        logits [BM, C, N] as predict_masks returns them -> (bits [K, W] int64 words, area [K] int32, changed [K] uint8), K = BM * C rows in the
        logits' order; ``ops.mask_unpack(bits, N)`` gives booleans.  keep_clicked: the seeds of a row are the cloud points nearest to the positive
        prompts (label 1) of its prompt set, prompt_points [BM, P, 3] / prompt_labels [BM, P] (default: those of set_prompts); the C masks of a
        prompt set share them.  After set_scene (and under set_crop, where the working cloud is the crop's and the points off the ball come back as zero
        bits), logits of the scan's width are reduced to the working cloud (the representatives' values), cleaned
        there and expanded, so every scan point has its representative's bit; logits of the working cloud's width are returned at that width.
        The clean-up works on the voxel graph: its result is at voxel granularity also for smooth logits (only the representatives' values count)."""
        if self._state is None:
            raise RuntimeError("call set_pointcloud() first")
        from .regions import RegionConfig, clean_bits
        if not isinstance(cfg, RegionConfig):
            raise TypeError(f"clean_masks: cfg must be a RegionConfig, got {type(cfg).__name__}")
        cfg.validate()
        state, mapping, _ = self._active()
        crop = self.crop is not None
        coords = state.coords
        B, Nw, _ = coords.shape
        if logits.dim() != 3 or logits.shape[0] % B != 0:
            raise ValueError(f"clean_masks: logits must be [BM, C, N] with BM a multiple of the {B} cached cloud(s), got {tuple(logits.shape)}")
        sc = mapping if mapping is not None and not mapping.identity else None
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
            if crop:
                from .scene import crop_prompts
                prompt_points = crop_prompts(sc, prompt_points.to(coords.device))       # the clicks are scan coordinates, the crop cloud's are the unit ball's
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
            bits, area = (ops.crop_expand_bits if crop else ops.scene_expand_bits)(bits.contiguous(), sc.inv, Nw)
        return bits, area, changed

    # -- instance geometry -------------------------------------------------------------------------------------
    def _geometry_cloud(self, what: str, cloud: int = 0):
        """(xyz [N, 3], rgb [N, 3]) the user gave: the scan after set_scene (with or without a crop), cloud `cloud` of the batch after set_pointcloud."""
        if self._state is None:
            raise RuntimeError("call set_pointcloud() first")
        xyz, rgb = self._keepalive
        if self.scene is not None:
            return xyz, rgb
        if isinstance(cloud, bool) or not isinstance(cloud, int) or not 0 <= cloud < xyz.shape[0]:
            raise ValueError(f"{what}: cloud must be an index into the {xyz.shape[0]} cached cloud(s), got {cloud!r}")
        return xyz[cloud], rgb[cloud]

    @staticmethod
    def _geometry_bits(masks, n_points: int, what: str, whose: str):
        bits = masks.bits if hasattr(masks, "bits") else masks
        if not isinstance(bits, torch.Tensor) or bits.dim() != 2 or bits.dtype != torch.int64:
            raise ValueError(f"{what}: masks must be a Proposals or packed bits [k, W] int64, got {type(masks).__name__}"
                             + (f" {tuple(bits.shape)} {bits.dtype}" if isinstance(bits, torch.Tensor) else ""))
        if bits.shape[1] != ops.mask_words(n_points):
            raise ValueError(f"{what}: masks of {bits.shape[1]} words do not fit {whose}'s {n_points} points ({ops.mask_words(n_points)} words); "
                             "rows of a working cloud's width are the caller's to expand (ops.scene_expand_bits / crop_expand_bits)")
        return bits.contiguous()

    @torch.no_grad()
    def mask_geometry(self, masks, cloud: int = 0, oriented: bool = True):
        """Where the masks are: -> geometry.InstanceGeometry (count, centroid, axis-aligned and oriented box, covariance, mean colour, radius per
        mask) in the coordinates the user gave.  masks: a `Proposals` or packed bits [k, W].  After set_scene (with or without an active crop) W
        must be the scan's width and the scan's xyz / rgb are used; after set_pointcloud W must be the cloud's and cloud `cloud` of the batch is
        used.  Any other width is a ValueError."""
        from .geometry import mask_geometry
        xyz, rgb = self._geometry_cloud("mask_geometry", cloud)
        bits = self._geometry_bits(masks, xyz.shape[0], "mask_geometry", "the scan" if self.scene is not None else "the cloud")
        return mask_geometry(xyz.contiguous(), bits, rgb.contiguous(), oriented)

    # -- normals and superpoints (point_sam_amd/superpoints.py) -----------------------------------------------------
    def _superpoint_cache(self):
        if self._superpoints[0] != self._key:                         # another cloud since: set_pointcloud / set_scene / set_frames
            self._superpoints = (self._key, {})
        return self._superpoints[1]

    def _superpoint_graph(self, what: str, cfg, cloud: int):
        """(xyz [N, 3], its regions.PointGraph at cfg's voxel settings) for the cloud the user gave, the graph cached with the cloud."""
        from .regions import build_graph
        from .superpoints import SuperpointConfig
        if cfg is not None and not isinstance(cfg, SuperpointConfig):
            raise TypeError(f"{what}: cfg must be a SuperpointConfig, got {type(cfg).__name__}")
        cfg = (cfg or SuperpointConfig()).validate()
        xyz = self._geometry_cloud(what, cloud)[0].contiguous()
        cache, key = self._superpoint_cache(), ("graph", 0 if self.scene is not None else cloud, cfg.voxel_size, cfg.points_per_voxel)
        if key not in cache:
            cache[key] = build_graph(xyz, cfg.voxel_size, cfg.points_per_voxel)
        return cfg, xyz, cache[key]

    @torch.no_grad()
    def point_normals(self, viewpoint=None, cfg=None, cloud: int = 0):
        """(normal [N, 3] f32, curvature [N] f32) per point of the cloud the user gave (the scan after set_scene): the unit normal of the point's
        voxel neighbourhood, (0, 0, 0) where it holds fewer than ``cfg.min_points`` points, and the surface variation l0 / (l0 + l1 + l2).
        viewpoint: three numbers in the cloud's coordinates that every normal should face; None: the component of largest magnitude is positive.
        cfg: a `superpoints.SuperpointConfig` (its voxel settings and min_points count here)."""
        from .superpoints import estimate_normals
        cfg, xyz, graph = self._superpoint_graph("point_normals", cfg, cloud)
        return estimate_normals(graph, xyz, cfg, viewpoint).per_point()

    @torch.no_grad()
    def superpoints(self, cfg=None, cloud: int = 0):
        """The `superpoints.Superpoints` of the cloud the user gave (the scan after set_scene, at its full width): small, roughly planar patches
        grown from the normals.  Cached per configuration until the next set_pointcloud, set_scene or set_frames of another cloud."""
        from .superpoints import build_superpoints
        cfg, xyz, graph = self._superpoint_graph("superpoints", cfg, cloud)
        cache, key = self._superpoint_cache(), ("superpoints", 0 if self.scene is not None else cloud) + cfg.key()
        if key not in cache:
            cache[key] = build_superpoints(graph, xyz, cfg)
        return cache[key]

    @torch.no_grad()
    def snap_masks(self, masks, cfg=None, min_fraction: float = 0.5, cloud: int = 0):
        """Masks snapped to whole superpoints: -> (bits [k, W] int64, area [k] int32, changed [k] uint8), every row the union of the superpoints of
        which it held more than ``min_fraction``.  masks: a `Proposals` or packed bits [k, W] of the width `mask_geometry` takes."""
        from .superpoints import snap_bits
        sp = self.superpoints(cfg, cloud)
        bits = self._geometry_bits(masks, sp.labels.numel(), "snap_masks", "the scan" if self.scene is not None else "the cloud")
        return snap_bits(sp, bits, min_fraction)

    @torch.no_grad()
    def set_crop_to_mask(self, bits_row, margin: float = 0.1, voxel_size: float = None, max_points: int = None, smooth: bool = None):
        """Zoom into an object: set_crop() on the ball around one mask of the scan -- centre = the mask's centroid, radius = the distance to its
        farthest member times (1 + margin).  bits_row: [W] or [1, W] int64 words of the scan's width.  -> (center, radius) as given to set_crop
        (a tuple of three floats, a float).  An empty mask, or one whose members all coincide (radius 0), is a ValueError and leaves the state alone."""
        if self.scene is None or self._state is None:
            raise RuntimeError("set_crop_to_mask() zooms into a scene: call set_scene() first")
        if isinstance(margin, bool) or not isinstance(margin, (int, float)) or not 0 <= margin < float("inf"):
            raise ValueError(f"set_crop_to_mask: margin must be a finite number >= 0, got {margin!r}")
        _check_smooth(smooth, "set_crop_to_mask", allow_none=True)
        row = bits_row[None] if isinstance(bits_row, torch.Tensor) and bits_row.dim() == 1 else bits_row
        if isinstance(row, torch.Tensor) and row.dim() == 2 and row.shape[0] != 1:
            raise ValueError(f"set_crop_to_mask: one mask at a time, got {row.shape[0]} rows")
        from .geometry import mask_geometry
        xyz, _ = self._keepalive
        bits = self._geometry_bits(row, xyz.shape[0], "set_crop_to_mask", "the scan")
        geo = mask_geometry(xyz, bits, None, oriented=False)
        if not bool(geo.valid[0]):
            raise ValueError("set_crop_to_mask: the mask is empty")
        # The centroid as fp32 is the origin the radius was measured from, and what the crop's membership test subtracts.  One fp32 ulp on the
        # radius covers the rounding of the square root and of the crop's r * r, so the farthest member is inside also at margin 0.
        if not float(geo.radius[0]) > 0:                   # a single point, or coinciding ones: set_crop has no ball of radius 0 to build
            raise ValueError("set_crop_to_mask: the mask's members coincide (radius 0): there is no ball to zoom into")
        center = tuple(float(v) for v in geo.centroid[0].float().tolist())
        radius = float(np.nextafter(np.float32(float(geo.radius[0]) * (1.0 + float(margin))), np.float32(np.inf)))
        self.set_crop(center, radius, voxel_size, max_points, smooth)
        return center, radius

    # -- camera views (point_sam_amd/views.py) -------------------------------------------------------------------
    def _view_cloud(self, what: str, view=None, cloud: int = 0):
        """xyz [N, 3] contiguous of the cloud a view shows: the scan after set_scene (also under a crop: a view is of the scan), cloud `cloud` of the batch
        after set_pointcloud.  With a view: it must have been rendered from a cloud of that many points."""
        from .views import check_view
        if view is not None and isinstance(getattr(view, "cloud", None), int):
            cloud = view.cloud
        xyz = self._geometry_cloud(what, cloud)[0]
        if view is not None:
            check_view(view, xyz.shape[0], what)
        return xyz.contiguous()

    @torch.no_grad()
    def render_view(self, camera, splat: int = 1, cloud: int = 0):
        """The cached cloud as `camera` sees it -> views.View: a z-buffer of point splats, every in-view point drawn into the (2 splat + 1)^2 pixels
        around its own, the nearest point winning a pixel (ties: the lower index).  After set_scene the scan's points are drawn, with or without an
        active crop; after set_pointcloud cloud `cloud` of the batch.  One pass over the points, no host synchronisation."""
        from .views import Camera, View
        if not isinstance(camera, Camera):
            raise TypeError(f"render_view: camera must be a views.Camera, got {type(camera).__name__}")
        xyz = self._view_cloud("render_view", None, cloud)
        return View(ops.view_splat(xyz, camera, splat), camera, xyz.shape[0], splat, 0 if self.scene is not None else cloud)

    @torch.no_grad()
    def pick(self, view, pixels, window: int = 2):
        """The points under pixel clicks: pixels [P, 2] integers (x, y) -> (point_index [P] int32, xyz [P, 3]): per click the point shown by the
        non-empty pixel nearest to it within `window` pixels on both axes (ties in distance: the nearer point); -1 and NaN coordinates where the window
        is empty.  No host synchronisation."""
        from .views import check_pixels
        xyz = self._view_cloud("pick", view)
        idx = ops.view_pick(view.keys, check_pixels(pixels, xyz.device, "pick"), window)
        pts = xyz.index_select(0, idx.clamp_min(0).long())
        return idx, torch.where((idx < 0)[:, None], torch.full_like(pts, float("nan")), pts)

    @torch.no_grad()
    def click_pixels(self, view, pixels, labels, window: int = 2):
        """Pixel clicks as point prompts: -> (prompt_points [1, P, 3], prompt_labels [1, P]) for predict_masks / predict_mask_bits, the coordinates those
        of the picked points (pick).  A click that hits nothing is a ValueError naming the pixel; finding out costs the call's one host read."""
        from .views import check_pixels
        xyz = self._view_cloud("click_pixels", view)
        pix = check_pixels(pixels, xyz.device, "click_pixels")
        lab = torch.as_tensor(labels, device=xyz.device).reshape(-1)
        if lab.numel() != pix.shape[0]:
            raise ValueError(f"click_pixels: {pix.shape[0]} pixels but {lab.numel()} labels")
        idx = ops.view_pick(view.keys, pix, window)
        missed = torch.nonzero(idx < 0)[:, 0].cpu()                                  # the one host read
        if missed.numel() > 0:
            x, y = pix[int(missed[0])].tolist()
            raise ValueError(f"click_pixels: the click at pixel ({x}, {y}) hits no point within {window} pixels")
        return xyz.index_select(0, idx.long())[None], lab[None]

    @torch.no_grad()
    def mask_images(self, view, masks, rows: bool = False):
        """Packed masks as pictures of the view: masks a `Proposals` or bits [K, W] int64 words of the viewed cloud's width (checked as mask_geometry
        does) -> ids [height, width] int32, per pixel the first (best) mask that holds the point shown there, -1 for none or an empty pixel; with
        rows=True -> [K, height, width] uint8, one binary image per mask."""
        if not isinstance(rows, bool):
            raise ValueError(f"mask_images: rows must be True or False, got {rows!r}")
        xyz = self._view_cloud("mask_images", view)
        bits = self._geometry_bits(masks, xyz.shape[0], "mask_images", "the scan" if self.scene is not None else "the cloud")
        return (ops.view_paint_rows if rows else ops.view_paint_ids)(view.keys, bits, xyz.shape[0])

    @torch.no_grad()
    def lift_masks(self, view, images, tau: float):
        """Image masks back to the cloud: images [K, height, width] (or one [height, width]) uint8 / bool, non-zero = inside -> (bits [K, W] int64
        words of mask_pack's layout, area [K] int32): a point gets bit k iff it is VISIBLE in the view -- in the image, and at most `tau` behind the
        point that won its pixel -- and images[k] is set at its pixel.  The format mask_geometry, set_crop_to_mask, the NMS and snapshot / transfer
        take.  (Turning a lifted mask into a prompt mask would need a logit magnitude tuned on a trained checkpoint: not done here.)"""
        xyz = self._view_cloud("lift_masks", view)
        if not isinstance(images, torch.Tensor):
            raise TypeError(f"lift_masks: images must be a tensor, got {type(images).__name__}")
        if images.dim() == 2:
            images = images[None]
        if images.dtype == torch.bool:
            images = images.to(torch.uint8)
        return ops.view_lift_bits(xyz, view.camera, view.keys, images.to(xyz.device).contiguous(), tau)

    @torch.no_grad()
    def visible_bits(self, view, tau: float):
        """The points visible in the view -> (bits [1, W], area [1]): lift_masks of an all-ones image."""
        xyz = self._view_cloud("visible_bits", view)
        return ops.view_lift_bits(xyz, view.camera, view.keys, None, tau)

    # -- RGB-D frames (views.FrameSet) ---------------------------------------------------------------------------
    @torch.no_grad()
    def set_frames(self, depth, rgb, cameras, far, edge=0.05, depth_scale=None, center=None, scale=None, voxel_size: float = None,
                   max_points: int = None, smooth: bool = False):
        """From pictures to a scan: depth [F, height, width] (float32, or uint16 with `depth_scale`) and rgb [F, height, width, 3] (uint8, or float32
        in the trained convention) with one views.Camera per frame (pose world -> camera, rotation orthonormal) are unprojected into one scan -- the
        pixels with near <= depth <= far that the edge filter keeps (edge None: all of them), in ascending (frame, y, x) -- normalised to
        (p - center) / scale, and handed to set_scene(xyz, rgb, voxel_size, max_points, smooth).  center / scale None: the mean of the kept points and
        their largest distance from it; both are returned, so that the next batch of frames can be normalised identically (what transfer_masks and
        propagate require of two scans).  -> views.FrameSet: ``fs.views[f]`` is frame f as a view of the scan whose every kept pixel shows its own
        point -- pick, click_pixels, mask_images, lift_masks and visible_bits take it as they take a rendered view, on the original photograph;
        lift_masks then tests occlusion against the frame's measured depth.  Tensors or numpy arrays; two host reads (the count, the normalisation)."""
        from .views import build_frames, check_frame_cameras
        _check_smooth(smooth, "set_frames")
        if (voxel_size is None) == (max_points is None):       # set_scene's rule, asked before any device work
            raise ValueError("set_frames: give exactly one of voxel_size and max_points")
        cameras = check_frame_cameras(cameras, "set_frames")
        dev = getattr(self.model, "device", "cuda")
        depth, rgb = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) if isinstance(a, np.ndarray) else a for a in (depth, rgb))      # tensors stay where they are
        fs = build_frames(depth, rgb, cameras, far, edge, depth_scale, center, scale)
        self.set_scene(fs.xyz, fs.rgb, voxel_size, max_points, smooth)
        return fs

    # -- multi-view label fusion (point_sam_amd/fusion.py) ---------------------------------------------------------
    @torch.no_grad()
    def fuse_labels(self, views, labels, cfg, consistent: bool = False):
        """The 2-D segmentations of many views as ONE 3-D instance labelling of the cached cloud: views a views.FrameSet (set_frames) or a list of
        views.View of one size (render_view), labels [V, height, width] int32 (a tensor or a numpy array), a region id per pixel and view; ids below 0
        are "no label"; cfg a fusion.FusionConfig -> fusion.Fused (labels [N] per point of the cloud the user gave, -1 = none; votes, seen,
        labelled, dropped; num_instances; bits()).  consistent=False: ids of different views do not correspond -- every (view, id) is a region
        (count_v = the view's largest id + 1, one host read; more than cfg.max_regions in total is a ValueError), regions of different views are linked
        by co-visible containment and the instances are the links' connected components (fusion.link_regions).  The region rows and links are made on
        the working cloud's points after set_scene (the scan itself where it is its own working cloud), so the row matrix stays small; the vote then
        runs over EVERY point of the scan.  consistent=True: the ids are global already -- the vote only."""
        from . import fusion
        from .views import FrameSet, check_view
        if isinstance(views, FrameSet):
            vs, keys = views.views, views.keys
        elif isinstance(views, (list, tuple)) and len(views) >= 1:
            vs, keys = list(views), None
        else:
            raise TypeError(f"fuse_labels: views must be a views.FrameSet or a non-empty list of views.View, got {type(views).__name__}")
        xyz = self._view_cloud("fuse_labels", vs[0])
        for v in vs[1:]:
            check_view(v, xyz.shape[0], "fuse_labels")
            if tuple(v.keys.shape) != tuple(vs[0].keys.shape) or v.cloud != vs[0].cloud:
                raise ValueError(f"fuse_labels: the views must have one size and show one cloud, got {tuple(v.keys.shape)} of cloud {v.cloud} beside "
                                 f"{tuple(vs[0].keys.shape)} of cloud {vs[0].cloud}")
        if keys is None:
            keys = torch.stack([v.keys for v in vs])
        lab = fusion.check_labels(labels, keys.shape, xyz.device, "fuse_labels")
        sc = self.scene
        link_xyz = xyz if sc is None or sc.identity else xyz.index_select(0, sc.keep_idx)
        return fusion.fuse(xyz, link_xyz, [v.camera for v in vs], keys.contiguous(), lab, cfg, consistent)
