"""Back end of the reference's interactive demo on the HIP predictor.

The reference's ``demo/app.py`` is a Flask app whose routes mutate module-global state and call
``sam.set_pointcloud`` / ``sam.predict_masks`` (demo/app.py:177-206).  Here the same request/response contract is a
plain class (``DemoSession``: one method per route, JSON-shaped dicts in and out, same keys and status strings) and a
thin stdlib ``http.server`` binding -- Flask / flask_cors are not needed (nor installed in this image).  The static three.js
front end (demo/static) is UI and is not rebuilt, but its files are SERVED from ``--static-dir`` exactly as the reference does,
so the reference's front end talks to this server unchanged with no second file server.

Routes (reference line):  GET / (app.py:71-73: index.html) . GET /static/<path> (:76-78) . GET /mesh/<path> (:81-89: models/<path>)
POST /sampled_pointcloud (app.py:92-108) . GET /pointcloud/<name> (:111-141) . POST /clear (:144-150)
POST /next (:153-159) . POST /save (:162-175) . POST /segment (:177-206).
POST /segment_all (not in the reference): automatic mask proposals for the whole cloud, a first pass before the per-object clicks.
POST /crop {center, radius} . POST /crop/clear (not in the reference): zoom into a ball of the loaded cloud -- /segment and /segment_all then answer
from the ball's own working cloud (predictor.set_crop), still per loaded point, until the crop is cleared or another cloud is loaded.
POST /instances (not in the reference): /segment_all plus one box per kept mask (predictor.mask_geometry) . POST /crop/selection {margin}: zoom
into the ball around the current /segment mask (predictor.set_crop_to_mask).
POST /propagate {pointcloud, radius, pose?, align?, search?, plane?} (not in the reference): the next scan of a sequence -- the kept masks are carried over and re-segmented
there (predictor.snapshot / propagate).
POST /view {camera, splat?} (not in the reference): the loaded cloud as a camera sees it, a z-buffered point-splat image (predictor.render_view) .
POST /click_pixel {pixel, label, window?, frame?}: a click on that image, answered exactly as /segment answers a click on the point shown there.
POST /frames {depth, rgb, cameras, far, edge?, depth_scale?} (not in the reference): RGB-D frames fused into the loaded cloud (predictor.set_frames);
/click_pixel with "frame": f then takes a click on photograph f itself.
POST /fuse_labels {labels, tau, overlap?, min_points?, min_votes?, consistent?} (not in the reference): the frames' 2-D segmentations fused into one
instance labelling of that cloud (predictor.fuse_labels).
POST /map/add {pose?, labels?} . POST /map {min_votes?} . POST /map/clear (not in the reference): the loaded cloud, under its pose, is added to the
session's scan map (predictor.map_add, point_sam_amd/scanmap.py), with "track": {AlignConfig fields} after its pose was refined against the map
(predictor.map_align), and with "search": {SearchConfig fields} beside it after the scan was relocalised in the map without a starting pose; /map returns the map's voxels as a cloud with one voted label each.
POST /map/view {camera, min_misses?, min_votes?} (not in the reference): the map as a camera inside it sees it, ray cast through its voxels
(predictor.map_view): colour, voxel id, depth and voted label per pixel.
Every path taken from a URL is resolved INSIDE its root directory (no `..`, no absolute paths, no symlink escape).

    python -m point_sam_amd.demo_server --config large --ckpt model.safetensors --models-dir demo/static/models
"""
import argparse
import json
import os
import threading
from http.server import BaseHTTPRequestHandler, ThreadingHTTPServer

import numpy as np
import torch

from .evaluation import load_ply

MIME = {".html": "text/html; charset=utf-8", ".js": "application/javascript", ".css": "text/css", ".json": "application/json", ".ply": "application/octet-stream",
        ".obj": "text/plain", ".mtl": "text/plain", ".png": "image/png", ".jpg": "image/jpeg", ".jpeg": "image/jpeg", ".svg": "image/svg+xml", ".ico": "image/x-icon"}


def safe_join(root: str, rel: str) -> str:
    """`rel` (a URL path, possibly percent-encoded) resolved under `root`; ValueError if it would leave the directory."""
    from urllib.parse import unquote
    rel = unquote(rel).replace("\\", "/")
    if rel.startswith("/") or "\x00" in rel:
        raise ValueError(f"illegal path {rel!r}")
    base = os.path.realpath(root)
    full = os.path.realpath(os.path.join(base, rel))
    if full != base and not full.startswith(base + os.sep):
        raise ValueError(f"path {rel!r} leaves the served directory")
    return full


class DemoSession:
    """The demo's state machine.  ``predictor`` needs ``set_pointcloud(xyz, rgb)`` and
    ``predict_masks(points, labels, prompt_mask, multimask_output) -> (mask, scores, logits)``; ``/segment_all`` also needs
    ``generate_masks(cfg) -> [Proposals]``; with ``clean_min_points`` ``/segment`` also needs
    ``clean_masks(logits, cfg, points, labels) -> (bits, area, changed)``."""

    def __init__(self, predictor, models_dir: str = ".", pointcloud: str = None, output_dir: str = "results", device="cuda", static_dir: str = None,
                 working_points: int = None, clean_min_points: int = None, crop_points: int = None, smooth_edges: bool = False,
                 snap_superpoints: bool = False, map_voxel_size: float = 2.0 ** -6, map_max_voxels: int = 1 << 20):
        self.predictor = predictor
        from . import ops
        ops.map_inv_h(map_voxel_size)
        ops.map_capacities(map_max_voxels)
        # /map/add: the voxel size and the capacity of the session's scan map (scanmap.ScanMap), created by the first add
        self.map_voxel_size, self.map_max_voxels, self.scan_map = float(map_voxel_size), map_max_voxels, None
        if not isinstance(snap_superpoints, bool):
            raise ValueError(f"snap_superpoints must be True or False, got {snap_superpoints!r}")
        # True: /segment_all and /instances snap every proposal to whole superpoints (ProposalConfig.snap = the default SuperpointConfig, unless the
        # request gives its own "snap")
        self.snap_superpoints = snap_superpoints
        if not isinstance(smooth_edges, bool):
            raise ValueError(f"smooth_edges must be True or False, got {smooth_edges!r}")
        # True: the masks of a voxel working cloud or a crop reach the loaded points by a 3-NN blend, not by the voxel representative's value
        # (predictor.set_scene / set_crop smooth=True).  The keyword is only passed when set: a predictor without it keeps working.
        self.smooth_edges = smooth_edges
        if crop_points is not None and (isinstance(crop_points, bool) or not isinstance(crop_points, int) or crop_points < 1):
            raise ValueError(f"crop_points must be a positive integer or None, got {crop_points!r}")
        self.crop_points = crop_points         # /crop: the crop cloud's max_points; None: every point of the ball
        self.crop = None                       # (center, radius) of the active /crop
        if clean_min_points is not None and (isinstance(clean_min_points, bool) or not isinstance(clean_min_points, int) or clean_min_points < 1):
            raise ValueError(f"clean_min_points must be a positive integer or None, got {clean_min_points!r}")
        # None: /segment answers with the thresholded mask; N: with the part of it that hangs together with the positive clicks, holes and islands
        # below N points filled / removed (predictor.clean_masks)
        self.clean_min_points = clean_min_points
        self.working_points = working_points   # None: the model runs on every loaded point; N: on a voxel working cloud of at most N (predictor.set_scene)
        self.models_dir, self.pointcloud, self.output_dir = models_dir, pointcloud, output_dir
        self.static_dir = static_dir           # the front end's files (reference: demo/static); None = not served
        self.device = torch.device(device)
        self.lock = threading.Lock()          # the reference is single-threaded; requests are serialised here
        self.pc_xyz = self.pc_rgb = None
        self.norm = None                       # (shift, scale) that normalised the loaded cloud; None for a client-side sampled one
        self.obj_path = None
        self.masks = []
        self._reset_prompts()
        self.segment_mask = None
        self.view = None                       # the last /view of the loaded cloud (views.View); another cloud drops it
        self.frames = None                     # /frames: the views.FrameSet the loaded cloud was fused from; another cloud drops it

    def _set_cloud(self):
        smooth = {"smooth": True} if self.smooth_edges else {}
        if self.crop is not None:              # a crop zooms into a scene; without --working-points the scene is the loaded cloud itself
            self.predictor.set_scene(self.pc_xyz, self.pc_rgb, max_points=self.working_points or self.pc_xyz.shape[1], **smooth)
            self.predictor.set_crop(self.crop[0], self.crop[1], max_points=self.crop_points, **smooth)      # cached: built and encoded once per crop
        elif self.working_points is None:
            self.predictor.set_pointcloud(self.pc_xyz, self.pc_rgb)
        else:
            self.predictor.set_scene(self.pc_xyz, self.pc_rgb, max_points=self.working_points, **smooth)

    def _reset_prompts(self):
        self.prompts, self.labels, self.prompt_mask = [], [], None

    # ---- routes -----------------------------------------------------------------------------------------------
    def sampled_pointcloud(self, data: dict) -> dict:
        """Client-side sampled cloud: {"points": {i: v}, "colors": {i: v}} flattened xyz / rgb (app.py:92-108)."""
        pts = np.array(list(data["points"].values()), dtype=np.float64).reshape(-1, 3)
        col = np.array(list(data["colors"].values()), dtype=np.float64).reshape(-1, 3)
        with self.lock:
            self.pc_xyz = torch.from_numpy(pts).to(self.device).float()[None]
            self.pc_rgb = torch.from_numpy(col).to(self.device).float()[None]
            self.crop = None
            self.norm = None
            self.view = None
            self.frames = None
        return {"response": "success"}

    def load_pointcloud(self, path: str) -> dict:
        """Loads an ASCII PLY from models_dir, normalises it into the unit ball, rgb / 255 (app.py:111-141).  As in the
        reference, a configured --pointcloud overrides the requested name."""
        loaded = self._read_pointcloud(path, None)
        with self.lock:
            return self._install_pointcloud(*loaded)

    def _read_pointcloud(self, path: str, norm):
        """-> (name, xyz, rgb, norm).  norm: None, or the (shift, scale) of another cloud to normalise this one with (/propagate)."""
        name = self.pointcloud or path
        pts = load_ply(safe_join(self.models_dir, name))
        xyz, rgb = pts[:, :3], pts[:, 3:6] / 255
        if norm is None:
            shift = xyz.mean(0)
            norm = (shift, np.linalg.norm(xyz - shift, axis=-1).max())
        return name, (xyz - norm[0]) / norm[1], rgb, norm

    def _install_pointcloud(self, name, xyz, rgb, norm) -> dict:
        """The caller holds the lock."""
        self.obj_path = name
        self.pc_xyz = torch.from_numpy(xyz).to(self.device).float()[None]
        self.pc_rgb = torch.from_numpy(rgb).to(self.device).float()[None]
        self.crop = None
        self.norm = norm
        self.view = None
        self.frames = None
        return {"xyz": xyz.flatten().tolist(), "rgb": rgb.flatten().tolist()}

    def static_file(self, rel: str):
        """(bytes, mime type) of a front-end file under static_dir (app.py:71-89)."""
        if self.static_dir is None:
            raise FileNotFoundError("no --static-dir configured: front-end files are not served")
        full = safe_join(self.static_dir, rel)
        if not os.path.isfile(full):
            raise FileNotFoundError(rel)
        with open(full, "rb") as f:
            return f.read(), MIME.get(os.path.splitext(full)[1].lower(), "application/octet-stream")

    def clear(self) -> dict:
        with self.lock:
            self._reset_prompts()
            self.segment_mask = None
        return {"status": "cleared"}

    def next(self) -> dict:
        with self.lock:
            if self.segment_mask is None:
                raise ValueError("/next before any /segment: there is no mask to keep")
            self.masks.append(self.segment_mask.cpu().numpy())
            self._reset_prompts()
        return {"status": "cleared"}

    def save(self) -> dict:
        with self.lock:
            if self.pc_xyz is None or not self.masks:
                raise ValueError("/save needs a point cloud and at least one kept mask")
            os.makedirs(self.output_dir, exist_ok=True)
            stem = os.path.splitext(os.path.basename(self.obj_path or "pointcloud"))[0] or "pointcloud"      # 'sub/x.ply' -> 'x', './x.ply' -> 'x'
            np.save(os.path.join(self.output_dir, f"{stem}.npy"),
                    {"xyz": self.pc_xyz[0].cpu().numpy(), "rgb": self.pc_rgb[0].cpu().numpy(), "mask": np.stack(self.masks)})
            self._reset_prompts()
            self.segment_mask = None
        return {"status": "saved"}

    def segment(self, data: dict) -> dict:
        """One click: append the prompt, run the decoder on the cached cloud, keep the best mask's logits as the next
        dense prompt; multimask only on the first click (app.py:177-206)."""
        with self.lock:
            if self.pc_xyz is None:
                raise ValueError("/segment before a point cloud was set")
            return self._segment(data)

    def _segment(self, data: dict) -> dict:
        """/segment's work; the caller holds the lock and has checked that a cloud is loaded."""
        # the click joins the session only after the predictor accepted it: a malformed point must not poison every later click
        point = np.asarray(data["prompt_point"], dtype=np.float32)
        label = int(data["prompt_label"])
        if point.shape != (3,) or not np.isfinite(point).all():
            raise ValueError("prompt_point must be three finite numbers")
        prompts, labels = self.prompts + [point.tolist()], self.labels + [label]
        pts = torch.from_numpy(np.array(prompts, dtype=np.float32)).to(self.device).float()[None]
        lab = torch.from_numpy(np.array(labels)).to(self.device)[None]
        with torch.no_grad():
            self._set_cloud()
            mask, scores, logits = self.predictor.predict_masks(pts, lab, self.prompt_mask, self.prompt_mask is None)
        self.prompts, self.labels = prompts, labels
        best = torch.argmax(scores[0])
        self.prompt_mask = logits[0][best][None]
        if self.clean_min_points is None:
            self.segment_mask = mask[0][best] > 0
        else:
            from . import ops
            from .regions import RegionConfig
            cfg = RegionConfig(min_island=self.clean_min_points, min_hole=self.clean_min_points, keep_clicked=True)
            with torch.no_grad():
                bits, _, _ = self.predictor.clean_masks(logits[:1, best:best + 1], cfg, pts, lab)
            self.segment_mask = ops.mask_unpack(bits, mask.shape[-1])[0]
        return {"seg": self.segment_mask.cpu().numpy().tolist()}

    @staticmethod
    def _camera(spec):
        """A camera of a request: {"pose", "fx", "fy", "cx", "cy", "width", "height"} or {"eye", "target", "up", "fov_y_degrees", "width", "height"}, and
        optionally "near"."""
        from .views import Camera
        explicit, aimed = {"pose", "fx", "fy", "cx", "cy", "width", "height"}, {"eye", "target", "up", "fov_y_degrees", "width", "height"}
        if isinstance(spec, dict) and set(spec) - {"near"} == explicit:
            return Camera(**spec)
        if isinstance(spec, dict) and set(spec) - {"near"} == aimed:
            return Camera.look_at(**spec)
        raise ValueError(f"camera takes {sorted(explicit)} or {sorted(aimed)}, and optionally near")

    def set_frames(self, data: dict) -> dict:
        """RGB-D frames as the loaded cloud: {"depth": base64 of F * height * width little-endian words, uint16 if "depth_scale" is given and float32
        if not, "rgb": base64 of F * height * width * 3 bytes, "cameras": F cameras as /view takes them (pose world -> camera; they carry width and
        height), "far", "edge" (optional, default 0.05, null = no edge filter), "depth_scale" (optional)}.  The frames are unprojected, fused and
        normalised by predictor.set_frames (colours as /pointcloud/ has them, rgb / 255) and replace the loaded cloud.  -> {"frames", "width",
        "height", "num_points", "center", "scale", "xyz", "rgb"}.  /click_pixel with "frame": f then clicks on photograph f."""
        import base64
        import binascii
        with self.lock:
            need, may = {"depth", "rgb", "cameras", "far"}, {"edge", "depth_scale"}
            if not isinstance(data, dict) or not need <= set(data) or set(data) - need - may:
                raise ValueError('/frames takes {"depth", "rgb", "cameras", "far", "edge" (optional), "depth_scale" (optional)}')
            specs = data["cameras"]
            if not isinstance(specs, list) or not specs:
                raise ValueError("cameras must be a non-empty list, one camera per frame")
            cameras = [self._camera(spec) for spec in specs]
            F, H, W = len(cameras), cameras[0].height, cameras[0].width
            if any((c.height, c.width) != (H, W) for c in cameras):
                raise ValueError("every camera of /frames must have the same width and height")
            for name in ("far", "depth_scale", "edge"):
                v = data.get(name)
                if name in data and not (v is None and name == "edge") and (isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 < v < float("inf")):
                    raise ValueError(f"{name} must be a finite positive number" + (" or null" if name == "edge" else ""))
            depth_scale = data.get("depth_scale")
            try:
                raw_d, raw_c = (base64.b64decode(data[k], validate=True) if isinstance(data[k], str) else None for k in ("depth", "rgb"))
            except binascii.Error:
                raw_d = raw_c = None
            if raw_d is None or raw_c is None:
                raise ValueError("depth and rgb must be base64 strings")
            word = np.dtype("<f4") if depth_scale is None else np.dtype("<u2")
            if len(raw_d) != F * H * W * word.itemsize or len(raw_c) != F * H * W * 3:
                raise ValueError(f"{F} frames of {H} x {W} need {F * H * W * word.itemsize} bytes of {word.name} depth and {F * H * W * 3} bytes of rgb, "
                                 f"got {len(raw_d)} and {len(raw_c)}")
            depth = np.frombuffer(raw_d, dtype=word).reshape(F, H, W).astype(word.newbyteorder("="))
            rgb = np.frombuffer(raw_c, dtype=np.uint8).reshape(F, H, W, 3).astype(np.float32) / np.float32(255)
            smooth = {"smooth": True} if self.smooth_edges else {}
            with torch.no_grad():
                fs = self.predictor.set_frames(depth, rgb, cameras, data["far"], edge=data.get("edge", 0.05), depth_scale=depth_scale,
                                               max_points=self.working_points or F * H * W, **smooth)
            self.obj_path = "frames"
            self.pc_xyz, self.pc_rgb = fs.xyz[None], fs.rgb[None]
            self.crop, self.view, self.frames = None, None, fs
            self.norm = (np.asarray(fs.center, dtype=np.float64), float(fs.scale))
            return {"frames": F, "width": W, "height": H, "num_points": fs.num_points, "center": list(fs.center), "scale": fs.scale,
                    "xyz": fs.xyz.cpu().numpy().flatten().tolist(), "rgb": fs.rgb.cpu().numpy().flatten().tolist()}

    def fuse_labels(self, data: dict) -> dict:
        """The frames' 2-D segmentations as one labelling of the fused cloud: {"labels": base64 of F * height * width little-endian int32 region ids
        (below 0: none), "tau", and optionally "overlap", "min_points", "min_votes" (fusion.FusionConfig), "consistent" (the ids already agree between
        the frames)} -> {"labels": [N ints, -1 = none] as /segment_all has them, "num_instances": k, "sizes": [k point counts]}
        (predictor.fuse_labels).  Before any /frames of the loaded cloud, or with labels of another shape: a 400."""
        import base64
        import binascii
        from .fusion import FusionConfig
        with self.lock:
            if self.frames is None:
                raise ValueError("/fuse_labels before any /frames of this point cloud")
            may = {"labels", "tau", "overlap", "min_points", "min_votes", "consistent"}
            if not isinstance(data, dict) or not {"labels", "tau"} <= set(data) or set(data) - may:
                raise ValueError('/fuse_labels takes {"labels", "tau", "overlap" (optional), "min_points" (optional), "min_votes" (optional), "consistent" (optional)}')
            consistent = data.get("consistent", False)
            if not isinstance(consistent, bool):
                raise ValueError("consistent must be true or false")
            cfg = FusionConfig.from_overrides({k: v for k, v in data.items() if k not in ("labels", "consistent")})
            try:
                raw = base64.b64decode(data["labels"], validate=True) if isinstance(data["labels"], str) else None
            except binascii.Error:
                raw = None
            if raw is None:
                raise ValueError("labels must be a base64 string")
            F, H, W = tuple(self.frames.keys.shape)
            if len(raw) != F * H * W * 4:
                raise ValueError(f"{F} frames of {H} x {W} need {F * H * W * 4} bytes of int32 labels, got {len(raw)}")
            labels = np.frombuffer(raw, dtype="<i4").reshape(F, H, W).astype(np.int32)
            with torch.no_grad():
                fused = self.predictor.fuse_labels(self.frames, labels, cfg, consistent=consistent)
            out = fused.labels.cpu().numpy().astype(int)
            return {"labels": out.tolist(), "num_instances": int(fused.num_instances),
                    "sizes": np.bincount(out[out >= 0], minlength=int(fused.num_instances)).tolist()}

    def render_view(self, data: dict) -> dict:
        """The loaded cloud as a camera sees it: {"camera": {...}, "splat": s (optional, 0 .. 3, default 1)}; the camera is either {"pose": 3 x 4 or
        4 x 4 rows (cloud -> camera), "fx", "fy", "cx", "cy", "width", "height", "near" (optional)} or {"eye", "target", "up", "fov_y_degrees",
        "width", "height", "near" (optional)}, in the loaded cloud's normalised coordinates.  -> {"width", "height", "rgb": the image's
        height * width * 3 bytes, row-major RGB, base64; an empty pixel is black}.  The view is kept for /click_pixel until another cloud is loaded."""
        import base64
        with self.lock:
            if self.pc_xyz is None:
                raise ValueError("/view before a point cloud was set")
            if not isinstance(data, dict) or "camera" not in data or set(data) - {"camera", "splat"} or not isinstance(data["camera"], dict):
                raise ValueError('/view takes {"camera": {...}, "splat": s (optional)}')
            spec, splat = data["camera"], data.get("splat", 1)
            if isinstance(splat, bool) or not isinstance(splat, int) or not 0 <= splat <= 3:
                raise ValueError("splat must be an integer in 0 .. 3")
            camera = self._camera(spec)
            with torch.no_grad():
                self._set_cloud()
                view = self.predictor.render_view(camera, splat)
                img = (view.colour(self.pc_rgb[0], 0.0).clamp(0, 1) * 255).round().to(torch.uint8)
            self.view = view
            return {"width": camera.width, "height": camera.height, "rgb": base64.b64encode(img.cpu().numpy().tobytes()).decode("ascii")}

    def click_pixel(self, data: dict) -> dict:
        """A click on the last /view: {"pixel": [x, y], "label": l, "window": w (optional, 0 .. 16, default 2)}.  The point shown nearest to the pixel
        within the window (predictor.click_pixels) becomes the prompt, and the answer is /segment's for that point, bit for bit; a pixel that shows
        nothing is a 400 that leaves the click state alone.  With "frame": f (after /frames) the click is on photograph f, not on the last /view."""
        with self.lock:
            if self.pc_xyz is None:
                raise ValueError("/click_pixel before a point cloud was set")
            view = self.view
            if isinstance(data, dict) and "frame" in data:
                f = data["frame"]
                if self.frames is None:
                    raise ValueError("/click_pixel with a frame before any /frames of this point cloud")
                if isinstance(f, bool) or not isinstance(f, int) or not 0 <= f < len(self.frames.views):
                    raise ValueError(f"frame must be an integer in 0 .. {len(self.frames.views) - 1}")
                view = self.frames.views[f]
            elif view is None:
                raise ValueError("/click_pixel before any /view of this point cloud")
            if not isinstance(data, dict) or not {"pixel", "label"} <= set(data) or set(data) - {"pixel", "label", "window", "frame"}:
                raise ValueError('/click_pixel takes {"pixel": [x, y], "label": l, "window": w (optional), "frame": f (optional)}')
            pixel, window = data["pixel"], data.get("window", 2)
            if not isinstance(pixel, list) or len(pixel) != 2 or any(isinstance(v, bool) or not isinstance(v, int) for v in pixel):
                raise ValueError("pixel must be two integers [x, y]")
            if isinstance(window, bool) or not isinstance(window, int) or not 0 <= window <= 16:
                raise ValueError("window must be an integer in 0 .. 16")
            label = int(data["label"])
            with torch.no_grad():
                self._set_cloud()
                pts, _ = self.predictor.click_pixels(view, [pixel], [label], window)
            return self._segment({"prompt_point": pts[0, 0].cpu().numpy().tolist(), "prompt_label": label})

    def propagate(self, data: dict) -> dict:
        """The next scan of a sequence: {"pointcloud": name, "radius": r, "pose": 3 x 4 or 4 x 4 rows (optional), "align": {align.AlignConfig fields}
        (optional: the given pose, or the identity, is refined by ICP before the transfer -- predictor.align -- and the response also carries "pose", the
        3 x 4 rows used, and "align": {pairs, coverage, rms, iterations, converged}), "search": {align.SearchConfig fields} (optional, only together
        with "align" and without "pose": no starting pose is known, a grid of candidate poses is scored and the best are refined -- align.search -- and
        the response's "align" also carries "search": {poses, sample, chosen, candidates: [{pose_index, count, pairs, rms, converged}]}), "plane":
        {align.PlaneConfig fields} (optional, only together with "align": the snapshot is taken with its voxel normals and every ICP step is
        point-to-plane -- far fewer steps between scans of floors and walls; the response has the same fields)}.  The kept masks (/next) plus the
        current /segment mask become a snapshot of the loaded cloud (a mask's logits are +1 inside, -1 outside: the session keeps masks, not logits);
        the named cloud is loaded as /pointcloud/ does, but normalised with the SAME shift and scale as the cloud it follows (a transfer compares
        coordinates; a point that leaves the unit ball is the model's ValueError), and predictor.propagate re-segments every object there.  radius
        and pose are in those normalised coordinates, pose from the new cloud to the previous one.  -> {"xyz", "rgb" (the new cloud, as
        /pointcloud/), "objects": [{"seg": [...]} per object, /segment's format], "lost": [bool per object], "scores": [float or null]}.  The
        propagated masks replace the kept ones, the click state is reset and a crop dropped.  Before any mask, or with a bad value: a 400 that
        leaves the previous state."""
        with self.lock:
            if self.pc_xyz is None:
                raise ValueError("/propagate before a point cloud was set")
            masks = list(self.masks) + ([self.segment_mask.cpu().numpy()] if self.segment_mask is not None else [])
            if not masks:
                raise ValueError("/propagate before any /segment: there is no mask to carry over")
            search_fields = None
            if isinstance(data, dict) and "search" in data:
                if "align" not in data or "pose" in data:
                    raise ValueError('/propagate: "search" is valid only together with "align" and without "pose"')
                search_fields = data["search"]
                data = {k: v for k, v in data.items() if k != "search"}
            has_plane = isinstance(data, dict) and "plane" in data
            if has_plane:
                if "align" not in data:
                    raise ValueError('/propagate: "plane" is valid only together with "align"')
                plane_fields = data["plane"]
                data = {k: v for k, v in data.items() if k != "plane"}
            if not isinstance(data, dict) or not {"pointcloud", "radius"} <= set(data) or set(data) - {"pointcloud", "radius", "pose", "align"}:
                raise ValueError('/propagate takes {"pointcloud": name, "radius": r, "pose": rows (optional), "align": {AlignConfig fields} (optional), '
                                 '"search": {SearchConfig fields} and "plane": {PlaneConfig fields} (optional, beside "align")}')
            name, radius, pose = data["pointcloud"], data["radius"], data.get("pose")
            if not isinstance(name, str) or not name:
                raise ValueError("pointcloud must be a file name")
            if isinstance(radius, bool) or not isinstance(radius, (int, float)) or not 0 < radius < float("inf"):
                raise ValueError("radius must be a finite positive number")
            from . import ops
            ops.transfer_pose(pose)                # a bad pose is refused before anything is loaded
            align_cfg = None
            if "align" in data:
                from .align import AlignConfig
                align_cfg = AlignConfig.from_overrides(data["align"])      # and so is a bad align field
            search_cfg = None
            if search_fields is not None:
                from .align import SearchConfig
                search_cfg = SearchConfig.from_overrides(search_fields)    # or a bad search field
            plane_cfg = None
            if has_plane:
                from .align import PlaneConfig
                plane_cfg = PlaneConfig.from_overrides(plane_fields)       # or a bad plane field
            if any(m.shape != (self.pc_xyz.shape[1],) for m in masks):
                raise ValueError("/propagate: a kept mask does not belong to the loaded cloud")
            before = (self.pc_xyz, self.pc_rgb, self.obj_path, self.crop, self.norm)
            try:
                with torch.no_grad():
                    self.crop = None
                    self._set_cloud()
                    inside = torch.from_numpy(np.stack(masks).astype(bool)).to(self.device)
                    logits = torch.where(inside, 1.0, -1.0).float()
                    snap = self.predictor.snapshot(logits) if plane_cfg is None else self.predictor.snapshot(logits, normals=True)
                    cloud = self._install_pointcloud(*self._read_pointcloud(name, self.norm))
                    self._set_cloud()
                    found = None
                    if align_cfg is not None:
                        more = {} if plane_cfg is None else {"plane": plane_cfg}
                        found = (self.predictor.align(snap, align_cfg, pose, **more) if search_cfg is None else
                                 self.predictor.align(snap, align_cfg, search=search_cfg, **more))
                        pose = found.pose.tolist()
                    res = self.predictor.propagate(snap, float(radius), pose)
            except Exception:
                self.pc_xyz, self.pc_rgb, self.obj_path, self.crop, self.norm = before
                raise
            segs = (res.logits > 0).cpu().numpy()
            scores = res.scores.cpu().numpy().astype(float)
            self.masks = [m for m in segs]
            self._reset_prompts()
            self.segment_mask = None
            out = dict(cloud, objects=[{"seg": m.tolist()} for m in segs], lost=res.lost.cpu().numpy().astype(bool).tolist(),
                       scores=[float(v) if np.isfinite(v) else None for v in scores])
            if found is not None:
                out.update(pose=pose, align=dict(pairs=found.pairs, coverage=found.coverage, rms=found.rms if np.isfinite(found.rms) else None,
                                                 iterations=found.iterations, converged=found.converged))
                if search_cfg is not None:
                    rec = found.search
                    out["align"]["search"] = dict(poses=rec.poses, sample=rec.sample, chosen=rec.chosen, candidates=[
                        dict(c, rms=c["rms"] if np.isfinite(c["rms"]) else None) for c in rec.candidates])
            return out

    def set_crop(self, data: dict) -> dict:
        """Zoom: {"center": [x, y, z], "radius": r} in the loaded cloud's coordinates.  The crop is built (and its cloud encoded) now, so an empty
        ball or a bad value is this request's 400 and leaves the previous state; the clicks so far are dropped (they belong to another cloud)."""
        with self.lock:
            if self.pc_xyz is None:
                raise ValueError("/crop before a point cloud was set")
            if not isinstance(data, dict) or set(data) != {"center", "radius"}:
                raise ValueError('/crop takes {"center": [x, y, z], "radius": r}')
            center = np.asarray(data["center"], dtype=np.float64)
            radius = data["radius"]
            if center.shape != (3,) or not np.isfinite(center).all():
                raise ValueError("center must be three finite numbers")
            if isinstance(radius, bool) or not isinstance(radius, (int, float)) or not 0 < radius < float("inf"):
                raise ValueError("radius must be a finite positive number")
            previous = self.crop
            self.crop = (tuple(center.tolist()), float(radius))
            try:
                with torch.no_grad():
                    self._set_cloud()
            except Exception:
                self.crop = previous
                raise
            self._reset_prompts()
            self.segment_mask = None
            crop = getattr(self.predictor, "crop", None)
            return {"status": "cropped", "members": int(getattr(crop, "num_members", 0)), "working_points": int(getattr(crop, "num_working", 0))}

    def clear_crop(self) -> dict:
        with self.lock:
            self.crop = None
            if hasattr(self.predictor, "clear_crop"):
                self.predictor.clear_crop()
            self._reset_prompts()
            self.segment_mask = None
        return {"status": "cleared"}

    def segment_all(self, data: dict) -> dict:
        """"Segment everything": automatic mask proposals on the current cloud.  Optional body keys override `ProposalConfig` fields (an unknown key
        or a bad value is a ValueError -> 400).  {"labels": [N ints, -1 = none], "num_masks": k, "scores": [k floats]}, masks best first.  The
        click state of /segment is not touched."""
        with self.lock:
            return self._segment_all(data, "/segment_all")[1]

    def _segment_all(self, data, route: str):
        """-> (Proposals, the /segment_all response); the caller holds the lock."""
        from .proposals import ProposalConfig
        if self.pc_xyz is None:
            raise ValueError(f"{route} before a point cloud was set")
        if not isinstance(data, dict):
            raise ValueError(f"{route} takes a JSON object of ProposalConfig overrides (or nothing)")
        if self.snap_superpoints and "snap" not in data:
            data = dict(data, snap={})
        cfg = ProposalConfig.from_overrides(data)
        with torch.no_grad():
            self._set_cloud()
            prop = self.predictor.generate_masks(cfg)[0]
        return prop, {"labels": prop.labels.cpu().numpy().astype(int).tolist(), "num_masks": int(len(prop)), "scores": prop.score.cpu().numpy().astype(float).tolist()}

    def superpoints(self, data: dict) -> dict:
        """The geometric over-segmentation of the loaded cloud: {"config": {SuperpointConfig fields}} (optional) -> {"labels": [N ints, -1 = a point
        without a cell], "num_superpoints": S} (predictor.superpoints: small, roughly planar patches grown from the surface normals).  An unknown
        field or a bad value is a 400.  The click state of /segment is not touched."""
        from .superpoints import SuperpointConfig
        with self.lock:
            if self.pc_xyz is None:
                raise ValueError("/superpoints before a point cloud was set")
            if not isinstance(data, dict) or set(data) - {"config"} or not isinstance(data.get("config", {}), dict):
                raise ValueError('/superpoints takes {"config": {...}} (or nothing)')
            try:
                cfg = SuperpointConfig(**data.get("config", {})).validate()
            except TypeError as e:
                raise ValueError(f"bad SuperpointConfig: {e}") from None
            with torch.no_grad():
                self._set_cloud()
                sp = self.predictor.superpoints(cfg)
            return {"labels": sp.labels.cpu().numpy().astype(int).tolist(), "num_superpoints": int(sp.num)}

    def instances(self, data: dict) -> dict:
        """/segment_all plus where every kept mask is: "boxes" = one {center, half, axes (rows), aabb_lo, aabb_hi, count, mean_rgb} per mask, in the
        masks' order, in the loaded cloud's coordinates (predictor.mask_geometry: the oriented box along the mask's principal axes).  A number that
        does not exist (an empty mask has no box) is null."""
        with self.lock:
            prop, out = self._segment_all(data, "/instances")
            boxes = []
            if len(prop) > 0:
                with torch.no_grad():
                    geo = self.predictor.mask_geometry(prop)

                def num(t):
                    a = np.asarray(t.cpu().numpy(), dtype=np.float64)
                    return np.where(np.isfinite(a), a, None).tolist() if not np.isfinite(a).all() else a.tolist()
                for k in range(len(prop)):
                    boxes.append({"center": num(geo.obb_center[k]), "half": num(geo.obb_half[k]), "axes": num(geo.axes[k]), "aabb_lo": num(geo.aabb_lo[k]),
                                  "aabb_hi": num(geo.aabb_hi[k]), "count": int(geo.count[k]), "mean_rgb": None if geo.mean_rgb is None else num(geo.mean_rgb[k])})
            return dict(out, boxes=boxes)

    # ---- the scan map (point_sam_amd/scanmap.py) -----------------------------------------------------------------
    def _map_error(self, call):
        """Runs `call`; a map past its capacities is the client's 400, not a crash of the handler."""
        from .scanmap import MapOverflow
        try:
            return call()
        except MapOverflow as e:
            raise ValueError(str(e)) from None

    def map_add(self, data: dict) -> dict:
        """Adds the loaded cloud to the session's scan map (created by the first add: predictor.new_map(map_voxel_size, map_max_voxels)): {"pose": 3 x
        4 or 4 x 4 rows from the loaded cloud's coordinates to the map's (optional), "labels": [N ints, negative = none] (optional; without it point n
        gets the index of the first kept /next mask or current /segment mask that holds it, -1 outside all)} -> {"new_voxels", "accepted",
        "rejected", "num_voxels", "num_adds"}.  With "origin": [x, y, z] (the sensor's position in the loaded cloud's coordinates) the scan is then carved
        (predictor.map_carve, "margin": cells, optional, default 1) and the answer gains {"rays", "hit_voxels", "missed_voxels", "crossed",
        "num_carves"}.  With "track": {align.AlignConfig fields} the pose is first refined against the map itself (predictor.map_align, the request's
        pose as its start; skipped while the map is empty), the scan is added and carved under the refined pose, and the answer gains {"pose": the 3 x 4
        rows used, "pairs", "coverage", "rms", "converged", "reason"}.  With "search": {align.SearchConfig fields} beside "track" and WITHOUT "pose" (a
        pose is the start, a search starts from its own candidates: both together are a 400) the scan is first relocalised in the map
        (predictor.map_relocalize: a grid of poses scored on the map's voxels, the best refined by the same loop; skipped while the map is empty,
        as the track is) and the answer gains "search": {poses, sample, chosen, candidates: [{pose_index, count, pairs, rms, converged}]}, as
        /propagate returns it.  A bad value or a full map is a 400."""
        with self.lock:
            if self.pc_xyz is None:
                raise ValueError("/map/add before a point cloud was set")
            if not isinstance(data, dict) or set(data) - {"pose", "labels", "origin", "margin", "track", "search"}:
                raise ValueError('/map/add takes {"pose": rows (optional), "labels": [ints] (optional), "origin": [x, y, z] (optional), "margin": n (optional), '
                                 '"track": {AlignConfig fields} (optional), "search": {SearchConfig fields} (optional, beside "track", without "pose")}')
            from . import ops
            pose = data.get("pose")
            ops.transfer_pose(pose)
            track_cfg = None
            if "track" in data:
                from .align import AlignConfig
                track_cfg = AlignConfig.from_overrides(data["track"])      # a bad track field is a 400 before anything is touched
                ops.track_reach(track_cfg.radius, self.map_voxel_size)
            search_cfg = None
            if "search" in data:
                if track_cfg is None or pose is not None:
                    raise ValueError('/map/add: "search" is valid only together with "track" and without "pose": a pose is the start, and a search '
                                     'starts from its own candidates')
                from .align import SearchConfig
                search_cfg = SearchConfig.from_overrides(data["search"])   # a bad search field is a 400 before anything is touched
                if search_cfg.radius is not None:
                    ops.track_reach(search_cfg.radius, self.map_voxel_size)
                    if search_cfg.radius > track_cfg.radius:
                        raise ValueError(f'/map/add: the "search" radius {search_cfg.radius} exceeds the "track" radius {track_cfg.radius}')
            origin, margin = data.get("origin"), data.get("margin", 1)
            if "margin" in data and origin is None:
                raise ValueError('"margin" belongs to a carve: give "origin" too')
            if origin is not None:
                if not isinstance(origin, list) or len(origin) != 3 or any(isinstance(v, bool) or not isinstance(v, (int, float)) for v in origin):
                    raise ValueError('"origin" must be three numbers')
                if isinstance(margin, bool) or not isinstance(margin, int) or not 0 <= margin <= ops.CARVE_MAX_MARGIN:
                    raise ValueError('"margin" must be an integer in 0 .. 2^21 - 1')
                ops.carve_origin(origin, pose, self.map_voxel_size)
            N = self.pc_xyz.shape[1]
            if "labels" in data:
                lab = data["labels"]
                if not isinstance(lab, list) or len(lab) != N or any(isinstance(v, bool) or not isinstance(v, int) or not -2 ** 31 <= v < 2 ** 31 for v in lab):
                    raise ValueError(f"labels must be a list of {N} 32-bit integers, one per point of the loaded cloud")
                labels = np.asarray(lab, dtype=np.int32)
            else:
                masks = list(self.masks) + ([self.segment_mask.cpu().numpy()] if self.segment_mask is not None else [])
                if any(m.shape != (N,) for m in masks):
                    raise ValueError("/map/add: a kept mask does not belong to the loaded cloud")
                labels = np.full(N, -1, dtype=np.int32)
                for k in reversed(range(len(masks))):
                    labels[np.asarray(masks[k], dtype=bool)] = k
            with torch.no_grad():
                crop, self.crop = self.crop, None          # the whole loaded cloud is the scan, whatever crop is active
                try:
                    self._set_cloud()
                    if self.scan_map is None:
                        self.scan_map = self.predictor.new_map(self.map_voxel_size, self.map_max_voxels)
                    found = None
                    if track_cfg is not None and self.scan_map.num_voxels > 0:      # an empty map has nothing to track against: the pose as given
                        if search_cfg is None:
                            found = self._map_error(lambda: self.predictor.map_align(self.scan_map, track_cfg, pose))
                        else:
                            found = self._map_error(lambda: self.predictor.map_relocalize(self.scan_map, track_cfg, search_cfg))
                        pose = found.pose.tolist()
                        if origin is not None:
                            ops.carve_origin(origin, pose, self.map_voxel_size)
                    res = self._map_error(lambda: self.predictor.map_add(self.scan_map, torch.from_numpy(labels).to(self.device), pose))
                    cut = None if origin is None else self._map_error(lambda: self.predictor.map_carve(self.scan_map, origin, pose, margin))
                finally:
                    self.crop = crop
            out = {"new_voxels": int(res.new_voxels), "accepted": int(res.accepted), "rejected": int(res.rejected),
                   "num_voxels": int(self.scan_map.num_voxels), "num_adds": int(self.scan_map.num_adds)}
            if cut is not None:
                out.update(rays=int(cut.rays), hit_voxels=int(cut.hit_voxels), missed_voxels=int(cut.missed_voxels), crossed=int(cut.crossed),
                           num_carves=int(self.scan_map.num_carves))
            if track_cfg is not None:
                if found is None:
                    out.update(pose=np.eye(4)[:3].tolist() if pose is None else np.asarray(pose, dtype=np.float64)[:3].tolist(), pairs=0, coverage=0.0,
                               rms=None, converged=False, reason="the map was empty: nothing to track against")
                else:
                    out.update(pose=pose, pairs=int(found.pairs), coverage=float(found.coverage), rms=found.rms if np.isfinite(found.rms) else None,
                               converged=bool(found.converged), reason=found.reason)
                    if search_cfg is not None:
                        rec = found.search
                        out["search"] = dict(poses=rec.poses, sample=rec.sample, chosen=rec.chosen, candidates=[
                            dict(c, rms=c["rms"] if np.isfinite(c["rms"]) else None) for c in rec.candidates])
            return out

    def map_get(self, data: dict) -> dict:
        """The map as a cloud: {"min_votes": n (optional, default 1)} -> {"xyz", "rgb" (flattened, as /pointcloud/), "labels": [V ints, -1 = none],
        "votes": [V ints]}.  With "min_misses": n (>= 0) also "occupied": [V booleans], ScanMap.occupied(n) -- false where carving voted the voxel
        free.  Before any /map/add: a 400."""
        with self.lock:
            if not isinstance(data, dict) or set(data) - {"min_votes", "min_misses"}:
                raise ValueError('/map takes {"min_votes": n, "min_misses": n} (or nothing)')
            min_misses = data.get("min_misses")
            if min_misses is not None and (isinstance(min_misses, bool) or not isinstance(min_misses, int) or not 0 <= min_misses < 2 ** 31):
                raise ValueError("min_misses must be an integer >= 0")
            min_votes = data.get("min_votes", 1)
            if isinstance(min_votes, bool) or not isinstance(min_votes, int) or not 1 <= min_votes < 2 ** 31:
                raise ValueError("min_votes must be an integer >= 1")
            if self.scan_map is None or self.scan_map.num_voxels == 0:
                raise ValueError("/map before any /map/add: the map is empty")
            with torch.no_grad():
                xyz, rgb = self._map_error(self.scan_map.cloud)
                label, votes = self._map_error(lambda: self.scan_map.labels(min_votes))
                occupied = None if min_misses is None else self._map_error(lambda: self.scan_map.occupied(min_misses))
            out = {"xyz": xyz.cpu().numpy().astype(np.float64).flatten().tolist(), "rgb": rgb.cpu().numpy().astype(np.float64).flatten().tolist(),
                   "labels": label.cpu().numpy().astype(int).tolist(), "votes": votes.cpu().numpy().astype(int).tolist()}
            if occupied is not None:
                out["occupied"] = occupied.cpu().numpy().astype(bool).tolist()
            return out

    def map_view(self, data: dict) -> dict:
        """The session's scan map as a camera inside it sees it (predictor.map_view): {"camera": {...} as /view takes it, in the map's frame,
        "min_misses": n (optional; voxels that ScanMap.occupied(n) votes free are seen through; without it nothing is), "min_votes": n (optional,
        default 1)} -> {"width", "height", "rgb": height * width * 3 bytes as /view's (the voxels' mean colours, an empty pixel black), "index":
        height * width little-endian int32 words, the voxel id per pixel, -1 = empty, "depth": height * width little-endian float32 words, +inf =
        empty, "labels": height * width little-endian int32 words, the voxel's voted label, -1 = none; all base64}.  Before any /map/add, and for
        a camera whose centre lies outside [-1, 1]^3: a 400."""
        import base64
        from . import ops
        with self.lock:
            if not isinstance(data, dict) or "camera" not in data or set(data) - {"camera", "min_misses", "min_votes"} or not isinstance(data["camera"], dict):
                raise ValueError('/map/view takes {"camera": {...}, "min_misses": n (optional), "min_votes": n (optional)}')
            min_misses, min_votes = data.get("min_misses"), data.get("min_votes", 1)
            if min_misses is not None and (isinstance(min_misses, bool) or not isinstance(min_misses, int) or not 0 <= min_misses < 2 ** 31):
                raise ValueError("min_misses must be an integer >= 0")
            if isinstance(min_votes, bool) or not isinstance(min_votes, int) or not 1 <= min_votes < 2 ** 31:
                raise ValueError("min_votes must be an integer >= 1")
            camera = self._camera(data["camera"])
            ops.map_view_eye(camera, self.map_voxel_size)          # a camera outside the map: a 400 before anything runs
            if self.scan_map is None or self.scan_map.num_voxels == 0:
                raise ValueError("/map/view before any /map/add: the map is empty")
            m = self.scan_map
            with torch.no_grad():
                occupied = None if min_misses is None else self._map_error(lambda: m.occupied(min_misses))
                view = self._map_error(lambda: self.predictor.map_view(m, camera, occupied))
                labels = self._map_error(lambda: m.label_image(view, min_votes))
                img = (view.colour(self._map_error(m.cloud)[1], 0.0).clamp(0, 1) * 255).round().to(torch.uint8)
                index, depth = view.index.contiguous(), view.depth.contiguous()
            b64 = lambda t: base64.b64encode(t.cpu().numpy().tobytes()).decode("ascii")
            return {"width": camera.width, "height": camera.height, "rgb": b64(img), "index": b64(index), "depth": b64(depth), "labels": b64(labels)}

    def map_clear(self) -> dict:
        """Empties the session's scan map (a map that hit a capacity lives again)."""
        with self.lock:
            if self.scan_map is not None:
                self.scan_map.clear()
            return {"status": "cleared"}

    def crop_selection(self, data: dict) -> dict:
        """Zoom into the object just segmented: {"margin": m} (optional, default 0.1) -> the ball around the current /segment mask, its centre the
        mask's centroid and its radius the distance to the farthest point of the mask times 1 + m (predictor.set_crop_to_mask); from then on as
        after /crop with that centre and radius.  Without a cloud, without a /segment mask, with an empty mask or a bad margin: a 400 that leaves
        the previous state."""
        with self.lock:
            if self.pc_xyz is None:
                raise ValueError("/crop/selection before a point cloud was set")
            if self.segment_mask is None:
                raise ValueError("/crop/selection before any /segment: there is no mask to zoom into")
            if not isinstance(data, dict) or set(data) - {"margin"}:
                raise ValueError('/crop/selection takes {"margin": m} (or nothing)')
            margin = data.get("margin", 0.1)
            if isinstance(margin, bool) or not isinstance(margin, (int, float)) or not 0 <= margin < float("inf"):
                raise ValueError("margin must be a finite number >= 0")
            smooth = {"smooth": True} if self.smooth_edges else {}
            with torch.no_grad():
                # the mask is one of the loaded cloud: it is measured on the whole scene, whatever crop was active (self._set_cloud() brings that one
                # back on the next request if this call fails: it is cached)
                self.predictor.set_scene(self.pc_xyz, self.pc_rgb, max_points=self.working_points or self.pc_xyz.shape[1], **smooth)
                center, radius = self.predictor.set_crop_to_mask(pack_mask(self.segment_mask), margin=float(margin), max_points=self.crop_points, **smooth)
            self.crop = (tuple(float(v) for v in center), float(radius))
            self._reset_prompts()
            self.segment_mask = None
            crop = getattr(self.predictor, "crop", None)
            return {"status": "cropped", "center": list(self.crop[0]), "radius": self.crop[1], "members": int(getattr(crop, "num_members", 0)),
                    "working_points": int(getattr(crop, "num_working", 0))}


def pack_mask(mask: torch.Tensor) -> torch.Tensor:
    """bool [N] -> [ceil(N / 64)] int64 words of ops.mask_pack's layout (bit n % 64 of word n / 64 is point n), on the mask's device.  Plain torch
    on purpose: ops.mask_pack thresholds fp32 logits and runs on the GPU only, while /segment keeps a boolean mask (the cleaned one has no logits)
    and the session also runs against a predictor on the CPU; one row per request is not a hot path."""
    n = mask.numel()
    w = (n + 63) // 64
    pad = torch.zeros(w * 64, dtype=torch.int64, device=mask.device)
    pad[:n] = mask.reshape(-1).to(torch.int64)
    return (pad.reshape(w, 64) << torch.arange(64, dtype=torch.int64, device=mask.device)).sum(1)      # distinct bits: the sum is their OR, bit 63 wraps to the sign


MAX_BODY_BYTES = 64 << 20      # a sampled 10^5-point cloud as JSON is a few MB


def make_handler(session: DemoSession, allow_origin: str = "*"):
    class Handler(BaseHTTPRequestHandler):
        def _send(self, code, obj):
            body = json.dumps(obj).encode()
            self.send_response(code)
            self.send_header("Content-Type", "application/json")
            self.send_header("Content-Length", str(len(body)))
            self.send_header("Access-Control-Allow-Origin", allow_origin)      # what flask_cors provides in the reference
            self.send_header("Access-Control-Allow-Headers", "Content-Type, Access-Control-Allow-Origin")
            self.end_headers()
            self.wfile.write(body)

        def _run(self, fn, *a):
            try:
                self._send(200, fn(*a))
            except (ValueError, KeyError, AssertionError, FileNotFoundError) as e:
                self._send(400, {"error": f"{type(e).__name__}: {e}"})

        def do_OPTIONS(self):
            self._send(200, {})

        def _send_file(self, rel):
            try:
                body, mime = session.static_file(rel)
            except ValueError as e:
                return self._send(400, {"error": f"ValueError: {e}"})
            except FileNotFoundError as e:
                return self._send(404, {"error": f"not found: {e}"})
            self.send_response(200)
            self.send_header("Content-Type", mime)
            self.send_header("Content-Length", str(len(body)))
            self.send_header("Access-Control-Allow-Origin", allow_origin)
            self.end_headers()
            self.wfile.write(body)

        def do_GET(self):
            path = self.path.split("?", 1)[0]
            if path.startswith("/pointcloud/"):
                self._run(session.load_pointcloud, path[len("/pointcloud/"):])
            elif path == "/":
                self._send_file("index.html")                                   # app.py:71-73
            elif path.startswith("/static/"):
                self._send_file(path[len("/static/"):])                         # app.py:76-78
            elif path.startswith("/mesh/"):
                self._send_file("models/" + path[len("/mesh/"):])               # app.py:81-89
            else:
                self._send(404, {"error": f"no route {path}"})

        def do_POST(self):
            try:
                n = int(self.headers.get("Content-Length") or 0)
            except ValueError:
                return self._send(400, {"error": "bad Content-Length"})
            if n < 0 or n > MAX_BODY_BYTES:
                return self._send(413, {"error": f"request body over {MAX_BODY_BYTES} bytes"})
            try:
                data = json.loads(self.rfile.read(n) or b"{}")
            except json.JSONDecodeError as e:
                return self._send(400, {"error": f"bad JSON: {e}"})
            routes = {"/sampled_pointcloud": lambda: session.sampled_pointcloud(data), "/segment": lambda: session.segment(data),
                      "/segment_all": lambda: session.segment_all(data), "/propagate": lambda: session.propagate(data),
                      "/view": lambda: session.render_view(data), "/click_pixel": lambda: session.click_pixel(data),
                      "/frames": lambda: session.set_frames(data), "/fuse_labels": lambda: session.fuse_labels(data),
                      "/crop": lambda: session.set_crop(data), "/crop/clear": session.clear_crop,
                      "/instances": lambda: session.instances(data), "/superpoints": lambda: session.superpoints(data), "/crop/selection": lambda: session.crop_selection(data),
                      "/map/add": lambda: session.map_add(data), "/map": lambda: session.map_get(data), "/map/clear": session.map_clear,
                      "/map/view": lambda: session.map_view(data),
                      "/clear": session.clear, "/next": session.next, "/save": session.save}
            fn = routes.get(self.path)
            if fn is None:
                return self._send(404, {"error": f"no route {self.path}"})
            self._run(fn)

        def log_message(self, fmt, *args):  # quiet
            pass

    return Handler


def serve(session: DemoSession, host="localhost", port=5000) -> ThreadingHTTPServer:
    return ThreadingHTTPServer((host, port), make_handler(session))


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", default="localhost")
    ap.add_argument("--port", type=int, default=5000)
    ap.add_argument("--config", default="large")
    ap.add_argument("--ckpt", "--ckpt_path", dest="ckpt", default=None, help="safetensors checkpoint (random weights if omitted)")
    ap.add_argument("--pointcloud", default=None)
    ap.add_argument("--models-dir", default="demo/static/models")
    ap.add_argument("--static-dir", default="demo/static", help="the reference front end's files (index.html, *.js, models/)")
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--working-points", type=int, default=None,
                    help="run the model on a voxel working cloud of at most this many points and answer per loaded point (large scans); default: every point")
    ap.add_argument("--clean-min-points", type=int, default=None,
                    help="answer /segment with the cleaned mask: holes and islands below this many points filled / removed, only the clicked part kept")
    ap.add_argument("--crop-points", type=int, default=None,
                    help="POST /crop: the zoomed ball gets a working cloud of at most this many points; default: every point of the ball")
    ap.add_argument("--smooth-edges", action="store_true",
                    help="with --working-points or under /crop: blend each loaded point's mask value from the three nearest working points (smooth mask edges) "
                         "instead of copying its voxel's")
    ap.add_argument("--snap-superpoints", action="store_true",
                    help="/segment_all and /instances: snap every proposal to whole superpoints (planar patches grown from the surface normals)")
    ap.add_argument("--map-voxel-size", type=float, default=2.0 ** -6, help="POST /map/add: the voxel size of the session's scan map (normalised units)")
    ap.add_argument("--map-max-voxels", type=int, default=1 << 20, help="POST /map/add: the scan map's capacity in voxels; an add past it is a 400")
    return ap


def main():
    args = build_parser().parse_args()
    from .predictor import PointSAMPredictor
    pred = PointSAMPredictor.from_config(args.config, args.ckpt, precision=args.precision)
    srv = serve(DemoSession(pred, args.models_dir, args.pointcloud, static_dir=args.static_dir, working_points=args.working_points,
                            clean_min_points=args.clean_min_points, crop_points=args.crop_points, smooth_edges=args.smooth_edges,
                            snap_superpoints=args.snap_superpoints, map_voxel_size=args.map_voxel_size, map_max_voxels=args.map_max_voxels),
                args.host, args.port)
    print(f"Point-SAM demo back end on http://{args.host}:{args.port}")
    srv.serve_forever()


if __name__ == "__main__":
    main()
