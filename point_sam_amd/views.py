"""Camera views of a cloud: what a user sees and clicks is a 2-D picture of the scan, while prompts are scan coordinates and answers are per-point
masks.  A ``Camera`` is a pinhole (pose + intrinsics), a ``View`` is the z-buffer of point splats that ``ops.view_splat`` drew with it; the predictor
(``render_view`` / ``pick`` / ``click_pixels`` / ``mask_images`` / ``lift_masks`` / ``visible_bits``) goes from pixels to points and back through it.
The definition -- projection, key, footprint, pick, paint, lift -- is in include/pointsam_hip.h ("camera views"); the kernels are csrc/views.hip.
The other direction, from pictures to a scan, is a ``FrameSet``: RGB-D frames unprojected into one scan (csrc/frames.hip, "RGB-D frames" in the header),
every frame a ``View`` of it whose pixels show their own points (``predictor.set_frames``).

Conventions: the camera looks along +z of its own frame, x to the right and y DOWN, so pixel (x, y) = (floor(u), floor(v)) has its origin in the
image's top-left corner; ``pose`` maps the cloud's frame to the camera's, like the pose of ``ops.transfer_plan``.
"""
import math

import numpy as np
import torch

from . import ops


def _f32(value, what: str, positive: bool):
    if isinstance(value, bool) or not isinstance(value, (int, float, np.floating, np.integer)):
        raise ValueError(f"Camera: {what} must be a number, got {value!r}")
    with np.errstate(over="ignore"):
        v = np.float32(value)
    if not np.isfinite(v) or (positive and not v > 0):
        raise ValueError(f"Camera: {what} must be finite{' and positive' if positive else ''} in fp32, got {value!r}")
    return float(v)


class Camera:
    """A pinhole camera: pose 3 x 4 (or 4 x 4 with the last row (0, 0, 0, 1)) from the cloud's frame to the camera's, validated as ops.transfer_pose
    does; fx, fy > 0, cx, cy in pixels; width, height in 1 .. 8192; near > 0.  All values are rounded to fp32 once, here: ``pose_words`` (twelve fp32
    words, row-major) and the attributes are exactly what the kernels receive."""
    __slots__ = ("pose_words", "fx", "fy", "cx", "cy", "width", "height", "near")

    def __init__(self, pose, fx, fy, cx, cy, width, height, near=1e-3):
        if pose is None:
            raise ValueError("Camera: pose must be a 3 x 4 or 4 x 4 array, got None")
        self.pose_words = ops.transfer_pose(pose)
        self.fx, self.fy = _f32(fx, "fx", True), _f32(fy, "fy", True)
        self.cx, self.cy = _f32(cx, "cx", False), _f32(cy, "cy", False)
        for name, side in (("width", width), ("height", height)):
            if isinstance(side, bool) or not isinstance(side, (int, np.integer)) or not 1 <= side <= ops.VIEW_MAX_SIDE:
                raise ValueError(f"Camera: {name} must be an integer in 1 .. {ops.VIEW_MAX_SIDE}, got {side!r}")
        self.width, self.height = int(width), int(height)
        self.near = _f32(near, "near", True)

    @classmethod
    def from_fp32(cls, pose_words: np.ndarray, fx: float, fy: float, cx: float, cy: float, width: int, height: int, near: float) -> "Camera":
        """A camera from values that already ARE what the constructor would store (twelve finite fp32 pose words, fp32-representable floats, checked
        sides): no validation, for code that derives many cameras from validated ones (ops.frames_finish)."""
        cam = cls.__new__(cls)
        cam.pose_words, cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height, cam.near = pose_words, fx, fy, cx, cy, width, height, near
        return cam

    @property
    def pose(self) -> np.ndarray:
        return self.pose_words.reshape(3, 4)

    @classmethod
    def look_at(cls, eye, target, up, fov_y_degrees, width, height, near=1e-3) -> "Camera":
        """The camera at `eye` looking at `target` with `up` towards the top of the image, vertical field of view `fov_y_degrees`, square pixels, the
        principal point in the image's centre.  Computed in fp64 on the host, rounded to fp32 once: z = normalised (target - eye), x = normalised
        z x up, y = z x x (down), rotation rows (x, y, z), translation -R eye; fy = fx = (height / 2) / tan(fov / 2)."""
        try:
            e, t, u = (np.asarray(v, dtype=np.float64).reshape(3) for v in (eye, target, up))
        except (TypeError, ValueError):
            raise ValueError("Camera.look_at: eye, target and up must be three numbers each") from None
        if not (np.isfinite(e).all() and np.isfinite(t).all() and np.isfinite(u).all()):
            raise ValueError("Camera.look_at: eye, target and up must be finite")
        if isinstance(fov_y_degrees, bool) or not isinstance(fov_y_degrees, (int, float)) or not 0 < fov_y_degrees < 180:
            raise ValueError(f"Camera.look_at: fov_y_degrees must lie in (0, 180), got {fov_y_degrees!r}")
        z = t - e
        nz = np.linalg.norm(z)
        if not nz > 0:
            raise ValueError("Camera.look_at: eye and target coincide")
        z = z / nz
        x = np.cross(z, u)
        nx = np.linalg.norm(x)
        if not nx > 1e-12 * max(np.linalg.norm(u), 1e-300):
            raise ValueError("Camera.look_at: up is parallel to the viewing direction")
        x = x / nx
        y = np.cross(z, x)
        R = np.stack([x, y, z])
        pose = np.concatenate([R, (-R @ e)[:, None]], axis=1)
        if isinstance(height, bool) or not isinstance(height, (int, np.integer)) or isinstance(width, bool) or not isinstance(width, (int, np.integer)):
            raise ValueError(f"Camera.look_at: width and height must be integers, got {width!r} and {height!r}")
        f = (height / 2.0) / math.tan(math.radians(fov_y_degrees) / 2.0)
        return cls(pose, f, f, width / 2.0, height / 2.0, width, height, near)


class View:
    """A rendered view: ``keys`` [height, width] int64 words of ops.view_splat, the ``camera`` and footprint ``splat`` that drew them, ``num_points`` of
    the cloud they index (and which ``cloud`` of a set_pointcloud batch).  ``index`` and ``depth`` are read from the keys; nothing is copied to the host."""
    __slots__ = ("keys", "camera", "num_points", "splat", "cloud")

    def __init__(self, keys: torch.Tensor, camera: Camera, num_points: int, splat: int = 1, cloud: int = 0):
        self.keys, self.camera, self.num_points, self.splat, self.cloud = keys, camera, int(num_points), splat, cloud

    @property
    def index(self) -> torch.Tensor:
        """[height, width] int32, a VIEW of the keys' low words: the winning point per pixel, -1 where the pixel is empty."""
        H, W = self.keys.shape
        return self.keys.view(torch.int32).view(H, W, 2)[..., 0]

    @property
    def depth(self) -> torch.Tensor:
        """[height, width] float32: the winner's depth (its camera-frame z), +inf where the pixel is empty."""
        H, W = self.keys.shape
        d = self.keys.view(torch.float32).view(H, W, 2)[..., 1]
        return torch.where(self.keys == -1, torch.full_like(d, float("inf")), d)

    def colour(self, rgb: torch.Tensor, background=0.0) -> torch.Tensor:
        """rgb [num_points, 3] (any dtype, on the keys' device) -> [height, width, 3]: every pixel's winner's colour, `background` (a number or three)
        where the pixel is empty."""
        if rgb.dim() == 3 and rgb.shape[0] == 1:
            rgb = rgb[0]
        if rgb.dim() != 2 or tuple(rgb.shape) != (self.num_points, 3):
            raise ValueError(f"View.colour: rgb must be [{self.num_points}, 3] for this view, got {tuple(rgb.shape)}")
        idx = self.index
        out = rgb.index_select(0, idx.reshape(-1).clamp_min(0).long()).reshape(idx.shape + (3,))
        bg = torch.as_tensor(background, dtype=rgb.dtype, device=rgb.device).expand(3)
        return torch.where((idx < 0)[..., None], bg, out)


ORTHONORMAL_TOLERANCE = 1e-4


def check_frame_cameras(cameras, what: str) -> list:
    """The cameras of RGB-D frames: a non-empty list of Camera whose rotations are orthonormal, max|R R^T - I| <= 1e-4 in fp64 -- unprojection inverts
    a pose with the transpose.  ValueError names the frame."""
    if not isinstance(cameras, (list, tuple)) or len(cameras) < 1:
        raise ValueError(f"{what}: cameras must be a non-empty list of views.Camera, one per frame, got {type(cameras).__name__}")
    for f, cam in enumerate(cameras):
        if not isinstance(cam, Camera):
            raise TypeError(f"{what}: cameras[{f}] must be a views.Camera, got {type(cam).__name__}")
        R = cam.pose.astype(np.float64)[:, :3]
        err = float(np.abs(R @ R.T - np.eye(3)).max())
        if not err <= ORTHONORMAL_TOLERANCE:
            raise ValueError(f"{what}: the rotation of cameras[{f}] (frame {f}) is not orthonormal: max|R R^T - I| = {err:.3g} > {ORTHONORMAL_TOLERANCE}")
    return list(cameras)


class FrameSet:
    """RGB-D frames fused into one scan (predictor.set_frames): ``views``, one View per frame with splat = 0 whose keys -- a slice of ``keys``
    [F, height, width] -- hold every kept pixel's OWN point, with the frame's camera in the normalised frame; ``index`` [F, height, width] int32, a
    kept pixel's point or -1; ``xyz`` / ``rgb`` [num_points, 3], the scan as set_scene received it; ``center`` (three floats) and ``scale``, the
    normalisation xyz = (world - center) / scale: pass them to the next set_frames to normalise another batch of frames identically."""
    __slots__ = ("views", "keys", "index", "xyz", "rgb", "center", "scale", "num_points")

    def __init__(self, keys: torch.Tensor, cameras, index: torch.Tensor, xyz: torch.Tensor, rgb: torch.Tensor, center, scale: float):
        self.keys, self.index, self.xyz, self.rgb = keys, index, xyz, rgb
        self.center, self.scale, self.num_points = tuple(float(v) for v in center), float(scale), int(xyz.shape[0])
        self.views = [View(keys[f], cam, self.num_points, 0) for f, cam in enumerate(cameras)]


def build_frames(depth, rgb, cameras, far, edge=0.05, depth_scale=None, center=None, scale=None) -> FrameSet:
    """Unproject (ops.frames_unproject), normalise and key (ops.frames_finish) -> FrameSet.  center / scale None (both or neither): the rule of
    evaluation.normalize_points -- the mean, then the largest distance from it -- computed in fp64 on the device and rounded to fp32 once."""
    cameras = check_frame_cameras(cameras, "set_frames")
    if (center is None) != (scale is None):
        raise ValueError("set_frames: pass both center and scale, or neither")
    if isinstance(center, torch.Tensor):
        center = center.detach().cpu().numpy()
    world, col, index, _ = ops.frames_unproject(depth, rgb, cameras, far, edge, depth_scale)
    if center is None:
        w64 = world.double()
        mean = w64.mean(0)
        stats = torch.cat([mean, ((w64 - mean) ** 2).sum(1).max().sqrt()[None]]).float().cpu().numpy()          # rounded to fp32 once; one host read
        center, scale = stats[:3], float(stats[3])
        if not scale > 0:
            raise ValueError("set_frames: the kept points coincide (scale 0): pass center and scale")
    xyz, keys, normalised = ops.frames_finish(world, index, cameras, center, scale)
    return FrameSet(keys, normalised, index, xyz, col, np.asarray(center, dtype=np.float32).reshape(3), float(np.float32(scale)))


def check_view(view, num_points: int, what: str) -> View:
    if not isinstance(view, View):
        raise TypeError(f"{what}: view must be a views.View (render_view), got {type(view).__name__}")
    if view.num_points != num_points:
        raise ValueError(f"{what}: the view was rendered from a cloud of {view.num_points} points, the current one has {num_points}")
    return view


def check_pixels(pixels, device, what: str) -> torch.Tensor:
    """-> [P, 2] int32 on `device`.  Accepts a tensor or nested lists of integers."""
    t = pixels if isinstance(pixels, torch.Tensor) else torch.as_tensor(np.asarray(pixels))
    if t.dtype not in (torch.int32, torch.int64, torch.int16, torch.uint8):
        raise TypeError(f"{what}: pixels must be integers (x, y), got {t.dtype}")
    if t.dim() != 2 or t.shape[1] != 2 or t.shape[0] < 1:
        raise ValueError(f"{what}: pixels must be [P, 2] with P >= 1, got {tuple(t.shape)}")
    return t.to(device=device, dtype=torch.int32).contiguous()
