"""The pose between two scans: point-to-point ICP on the transfer index (csrc/align.hip, ops.align_step, predictor.align).

transfer.py carries masks from one scan to the next given the rigid motion that remains between them once both are normalised with the same centre
and scale.  Two re-scans of a room rarely come with that motion, and odometry is a few centimetres off; a wrong pose does not fail loudly, the masks
land beside their objects.  `icp` estimates it: every step pairs each query with its nearest source within a radius and sums what the closed-form
solution needs in ONE launch (ops.align_step: 20 fp64 words, bit-reproducible), the host reads those 160 bytes and solves a 3 x 3 SVD (`solve_rigid`).
The sums are over the queries AS GIVEN, so each step solves for the whole pose: nothing is composed, nothing drifts.

ICP is a local method: it refines an initial pose (the identity, or odometry) whose error is small against the search radius and the scene's
structure; it does not search globally.  `Alignment.coverage` and `rms` say how far to trust the answer.

Rooms are floors, walls and table tops, the surfaces ALONG which point-to-point ICP crawls: a query slides over a plane at no cost to the true
motion but is held by its nearest sample.  With a normal per source (`icp(..., normals=...)`: predictor.snapshot(normals=True) keeps the voxel
normals of normals.hip) every step minimises the distance to the pair's tangent PLANE instead: one ops.align_plane_step (32 fp64 words: the 6 x 6
normal equations of the linearised residual), one 256-byte host read and `solve_plane`.  That step is a small motion composed onto the pose, so
the run ends by tolerance on the update (`PlaneConfig`), typically in a handful of steps.

`search` is the global part, for callers without even a rough pose (a room re-scanned from another doorway, an object put down elsewhere): a grid of
candidate poses (`rotation_grid` x anchors x a translation lattice, `candidate_poses`) is scored on a sample of the queries by ONE launch
(ops.align_score: per pose the number of sampled queries that land within a radius of a source -- an exact integer), the `keep` best are refined by
`icp`, and the refinement with the most pairs wins.  The count alone does not decide: a false optimum of a partial overlap can cover as many
sampled queries as the truth, and only the refinement tells them apart.
"""
import dataclasses
import math

import numpy as np

from . import ops


def _number(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float)) and v == v and abs(v) != float("inf")


def _integer(v, lo, hi) -> bool:
    return not isinstance(v, bool) and isinstance(v, int) and lo <= v <= hi


class _Overrides:
    """from_overrides of the three configs; REQUIRED: the fields without a default."""
    REQUIRED = ()

    @classmethod
    def from_overrides(cls, data: dict):
        """A config from a dict of fields (a request's body; arrays as nested lists): an unknown field is a ValueError, like a bad value."""
        names = {f.name for f in dataclasses.fields(cls)}
        if not isinstance(data, dict) or set(data) - names or set(cls.REQUIRED) - set(data):
            raise ValueError(f"{cls.__name__} takes {''.join(r + ' and ' for r in cls.REQUIRED)}optionally {sorted(names - set(cls.REQUIRED))}, "
                             f"got {sorted(data) if isinstance(data, dict) else data!r}")
        return cls(**data)


@dataclasses.dataclass(frozen=True)
class AlignConfig(_Overrides):
    """radius: the search radius of step 0, and the cell size of the index (normalised coordinates); final_radius (None: radius): where the shrinking
    stops; shrink in (0, 1]: the radius of step k is max(final_radius, radius * shrink**k); iterations >= 1: the most steps; min_pairs >= 3: fewer
    pairs end the run; tol_rotation (radians) / tol_translation: when BOTH are positive, a step that changes the pose by less than both, at the final
    radius, ends the run as converged -- with either at 0 only the exact fixed point does.
    NONE of the defaults has been tuned on real data."""
    radius: float
    final_radius: float = None
    shrink: float = 1.0
    iterations: int = 30
    min_pairs: int = 16
    tol_rotation: float = 0.0
    tol_translation: float = 0.0
    REQUIRED = ("radius",)

    def __post_init__(self):
        if not _number(self.radius):
            raise ValueError(f"AlignConfig: radius must be a finite positive number, got {self.radius!r}")
        ops.transfer_radius(self.radius)
        if self.final_radius is not None:
            if not _number(self.final_radius) or not 0 < self.final_radius <= self.radius:
                raise ValueError(f"AlignConfig: final_radius must be None or lie in (0, radius], got {self.final_radius!r}")
            ops.transfer_radius(self.final_radius)
        if not _number(self.shrink) or not 0 < self.shrink <= 1:
            raise ValueError(f"AlignConfig: shrink must lie in (0, 1], got {self.shrink!r}")
        if not _integer(self.iterations, 1, 10000):
            raise ValueError(f"AlignConfig: iterations must be an integer in 1 .. 10000, got {self.iterations!r}")
        if not _integer(self.min_pairs, 3, 1 << 28):
            raise ValueError(f"AlignConfig: min_pairs must be an integer in 3 .. 2^28, got {self.min_pairs!r}")
        for name in ("tol_rotation", "tol_translation"):
            v = getattr(self, name)
            if not _number(v) or v < 0:
                raise ValueError(f"AlignConfig: {name} must be a finite number >= 0, got {v!r}")

    def step_radius(self, k: int) -> float:
        """The search radius of step k."""
        last = self.radius if self.final_radius is None else self.final_radius
        return max(float(last), float(self.radius) * float(self.shrink) ** k)


@dataclasses.dataclass
class Alignment:
    """icp's answer.  pose: 3 x 4 fp64, query frame -> source frame: what transfer_masks / propagate take.  pairs, rms: of the last step whose solve
    succeeded -- its pairs were found under the pose BEFORE that solve, rms is their root mean square distance AFTER it; coverage = pairs / the
    participating queries that have a cell.  history: (pairs, rms, radius) per step taken.  search: None from icp; from `search` its SearchRecord."""
    pose: np.ndarray
    pairs: int
    coverage: float
    rms: float
    iterations: int
    converged: bool
    reason: str
    history: list
    search: object = None


def solve_rigid(sums):
    """The 20 sums of ops.align_step -> (pose 3 x 4 fp64, rms): the rotation R and translation t that minimise sum |R x + t - s|^2 over the pairs (Kabsch /
    Umeyama without scale), in fp64 on the host: H = sum x s^T - (sum x)(sum s)^T / n = U S V^T, R = V diag(1, 1, det(V U^T)) U^T, t = mean s - R mean x;
    rms = sqrt(residual / n) with residual = sum |s - mean s|^2 + sum |x - mean x|^2 - 2 tr(R H), clamped at 0.  ValueError("degenerate") for n < 3 or
    a second singular value <= 1e-12 of the first (collinear pairs: the rotation about their line is free)."""
    m = np.asarray(sums, dtype=np.float64).reshape(-1)
    if m.shape != (ops.ALIGN_SUMS,) or not np.isfinite(m).all():
        raise ValueError(f"solve_rigid: sums must be {ops.ALIGN_SUMS} finite numbers (ops.align_step)")
    n = m[0]
    if n < 3:
        raise ValueError("degenerate: fewer than 3 pairs")
    sx, ss = m[2:5], m[5:8]
    H = m[8:17].reshape(3, 3) - np.outer(sx, ss) / n
    U, S, Vt = np.linalg.svd(H)
    if not S[1] > 1e-12 * S[0]:
        raise ValueError("degenerate: the pairs are collinear")
    V = Vt.T
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(V @ U.T) > 0 else -1.0])
    R = V @ D @ U.T
    t = ss / n - R @ (sx / n)
    residual = (m[18] - ss @ ss / n) + (m[17] - sx @ sx / n) - 2.0 * np.trace(R @ H)
    return np.concatenate([R, t[:, None]], 1), float(np.sqrt(max(residual, 0.0) / n))


@dataclasses.dataclass(frozen=True)
class PlaneConfig(_Overrides):
    """Point-to-plane ICP (icp / search with `normals`).  tol_rotation (radians) / tol_translation, both > 0: a step at the final radius whose update
    (omega, v) has |omega| <= tol_rotation and |v| <= tol_translation ends the run as converged.  A point-to-plane step is composed onto the fp64
    pose while the kernel linearises at its fp32 rounding, so the pose does not settle on a bit-exact fixed point the way point-to-point does: it
    jitters at the level of an fp32 ulp of a pose word near 1 (6e-8; about 2e-8 was seen on the fixture of the tests), and the tolerances must sit
    above that; they sit at 1e-6, well below the last update that still moved the pose there (4.6e-5).  condition in (0, 1): the solve is refused as
    degenerate when the smallest eigenvalue of the 6 x 6 system is <= condition x the largest (a single plane leaves three motions free).
    NONE of the defaults has been tuned on real data."""
    tol_rotation: float = 1e-6
    tol_translation: float = 1e-6
    condition: float = 1e-10

    def __post_init__(self):
        for name in ("tol_rotation", "tol_translation", "condition"):
            v = getattr(self, name)
            if not _number(v) or not v > 0:
                raise ValueError(f"PlaneConfig: {name} must be a finite positive number, got {v!r}")
        if not self.condition < 1:
            raise ValueError(f"PlaneConfig: condition must lie in (0, 1), got {self.condition!r}")


def _rodrigues(w) -> np.ndarray:
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:                                         # sin(th) / th and (1 - cos th) / th^2 at their limits: the next terms are th^2 / 6 and / 24
        return np.eye(3) + K + 0.5 * (K @ K)
    return np.eye(3) + (math.sin(th) / th) * K + ((1.0 - math.cos(th)) / (th * th)) * (K @ K)


def solve_plane(sums, pose, condition: float = PlaneConfig.condition):
    """The 32 sums of ops.align_plane_step, taken under `pose` (3 x 4 fp64) -> (new pose 3 x 4 fp64, rms, |omega|, |v|).  A = the symmetric 6 x 6 of
    [9..29], g = [3..8]; z = (omega, v) solves A z = -g (by the eigen-decomposition of A: np.linalg.eigh), the minimiser of sum (r + J . z)^2, the
    point-to-plane residual linearised in a small rotation omega and translation v of the POSED queries.  The update is composed onto the fp64 pose:
    R' = the rotation nearest (SVD) to Rodrigues(omega) R, t' = Rodrigues(omega) t + v.  rms = sqrt(max([2] + z . g, 0) / [0]): the linearised
    residual after the step.  ValueError("degenerate: ...") for fewer than 6 used pairs or a smallest eigenvalue <= condition x the largest."""
    m = np.asarray(sums, dtype=np.float64).reshape(-1)
    if m.shape != (ops.PLANE_SUMS,) or not np.isfinite(m).all():
        raise ValueError(f"solve_plane: sums must be {ops.PLANE_SUMS} finite numbers (ops.align_plane_step)")
    P = np.asarray(pose, dtype=np.float64)
    if P.shape != (3, 4) or not np.isfinite(P).all():
        raise ValueError("solve_plane: pose must be a finite 3 x 4 array")
    n = m[0]
    if n < 6:
        raise ValueError("degenerate: fewer than 6 used pairs")
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = m[9:30]
    A = A + np.triu(A, 1).T
    g = m[3:9]
    lam, V = np.linalg.eigh(A)
    if not lam[0] > condition * lam[-1]:
        raise ValueError("degenerate: the used pairs' planes leave a motion free")
    z = -(V @ ((V.T @ g) / lam))
    W = _rodrigues(z[:3])
    U, _, Vt = np.linalg.svd(W @ P[:, :3])
    R = U @ np.diag([1.0, 1.0, 1.0 if np.linalg.det(U @ Vt) > 0 else -1.0]) @ Vt
    t = W @ P[:, 3] + z[3:]
    rms = float(np.sqrt(max(m[2] + z @ g, 0.0) / n))
    return np.concatenate([R, t[:, None]], 1), rms, float(np.linalg.norm(z[:3])), float(np.linalg.norm(z[3:]))


def _initial(init) -> np.ndarray:
    if init is None:
        return np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    ops.transfer_pose(init)
    P = np.asarray(init.detach().cpu().numpy() if hasattr(init, "detach") else init, dtype=np.float64)[:3]
    return P.copy()


def _rotation_angle(A, B) -> float:
    c = (np.trace(A[:, :3].T @ B[:, :3]) - 1.0) / 2.0
    return float(np.arccos(min(1.0, max(-1.0, c))))


def icp(index, xyz, cfg: AlignConfig, init=None, bits=None, step=None, normals=None, plane=None) -> Alignment:
    """index: ops.transfer_index of the sources at cfg.radius; xyz [M, 3] the queries; init: the pose to start from (None: the identity); bits: an
    optional packed row, the queries that take part -> Alignment.  Each step is one ops.align_step under the current pose, one 160-byte host read
    and one solve_rigid.  Stops converged when the twelve fp32 words of the new pose equal the previous step's at the final radius (the next step
    would be bit-identical: a fixed point), or when both tolerances are positive and met there; stops unconverged, with the last good pose, when a
    step has fewer than cfg.min_pairs pairs or a degenerate solve, or when the iterations run out.  `step`: a stand-in for ops.align_step with its
    signature (a reference, a test).
    normals [N, 3] f32, one per source: point-to-plane.  Each step is one ops.align_plane_step, one 256-byte host read and one solve_plane; cfg's
    radius schedule, iterations and min_pairs (against word [0], the USED pairs) hold, its tolerances do not: the run is converged when, at the
    final radius, the update is within plane.tol_rotation and plane.tol_translation ("tolerance"), or the fp32 words repeat ("fixed point").
    coverage = used pairs / participating queries that have a cell; `step` then stands in for ops.align_plane_step (index, xyz, normals, pose,
    radius, bits).  plane: a PlaneConfig (None: the defaults); without normals it is a ValueError.
    Both kinds run ONE loop; they differ in the step, in the solve (-> new pose, rms, whether the update is small), in the word that counts the
    queries with a cell (19 / 31), and in the reason given when the words repeat AND the update is small: point-to-point says "fixed point",
    point-to-plane "tolerance"."""
    if not isinstance(cfg, AlignConfig):
        raise TypeError(f"icp: cfg must be an AlignConfig, got {type(cfg).__name__}")
    if normals is None:
        if plane is not None:
            raise ValueError("icp: plane configures point-to-plane ICP and needs normals")
        step = ops.align_step if step is None else step
        cell_word, both = ops.ALIGN_SUMS - 1, "fixed point"

        def take(pose, radius):
            return step(index, xyz, pose, radius, bits)

        def solve(sums, pose):
            new, rms = solve_rigid(sums)
            return new, rms, (cfg.tol_rotation > 0 and cfg.tol_translation > 0 and _rotation_angle(pose, new) <= cfg.tol_rotation and
                              float(np.linalg.norm(new[:, 3] - pose[:, 3])) <= cfg.tol_translation)
    else:
        plane = PlaneConfig() if plane is None else plane
        if not isinstance(plane, PlaneConfig):
            raise TypeError(f"icp: plane must be a PlaneConfig or None, got {type(plane).__name__}")
        step = ops.align_plane_step if step is None else step
        cell_word, both = ops.PLANE_SUMS - 1, "tolerance"

        def take(pose, radius):
            return step(index, xyz, normals, pose, radius, bits)

        def solve(sums, pose):
            new, rms, rot, tr = solve_plane(sums, pose, plane.condition)
            return new, rms, rot <= plane.tol_rotation and tr <= plane.tol_translation
    pose = _initial(init)
    last = cfg.step_radius(10 ** 9)
    out = Alignment(pose, 0, 0.0, float("nan"), 0, False, "iterations", [])
    for k in range(cfg.iterations):
        radius = cfg.step_radius(k)
        sums = take(pose, radius)
        sums = np.asarray(sums.cpu().numpy() if hasattr(sums, "cpu") else sums, dtype=np.float64)      # the one host read of the step
        out.iterations = k + 1
        pairs = int(sums[0])
        if pairs < cfg.min_pairs:
            out.history.append((pairs, float("nan"), radius))
            out.reason = f"pairs: {pairs} < min_pairs {cfg.min_pairs}"
            return out
        try:
            new, rms, small = solve(sums, pose)
        except ValueError as e:
            out.history.append((pairs, float("nan"), radius))
            out.reason = str(e)
            return out
        out.history.append((pairs, rms, radius))
        fixed = np.array_equal(new.astype(np.float32), pose.astype(np.float32))
        pose = new
        out.pose, out.pairs, out.rms, out.coverage = pose, pairs, rms, pairs / max(sums[cell_word], 1.0)
        if radius == last and (fixed or small):
            out.converged, out.reason = True, both if fixed and small else "fixed point" if fixed else "tolerance"
            return out
    return out


# ------------------------------------------------------------------------------------------------ the global search
MAX_POSES = ops.ALIGN_SCORE_MAX_POSES
GOLDEN_ANGLE = math.pi * (3.0 - math.sqrt(5.0))


@dataclasses.dataclass(frozen=True, eq=False)
class SearchConfig(_Overrides):
    """The grid `search` scores.  rotations: "yaw" (yaw_steps >= 1 turns by 2 pi k / yaw_steps about `up`, three numbers, not all zero), "so3" (`axes`
    >= 1 directions on the Fibonacci sphere, each with `rolls` >= 1 rolls about it: rotation_grid), or an explicit [R, 3, 3] array of rotation
    matrices.  anchors: None (the source centroid) or [A, 3] positions in the source frame where the query centroid may land -- e.g. the instance
    centroids of mask_geometry when an object is looked for.  offsets: g >= 0, the (2 g + 1)^3 translations offset_step * (i, j, k), -g <= i, j, k <=
    g, tried around each centre match (a partial overlap moves the centroid).  sample >= 1: the most queries scored.  radius: the scoring radius,
    None: the AlignConfig's; it may not exceed the index's.  keep >= 1: how many of the best-scoring candidates icp refines.
    rotations x anchors x offsets may not exceed 2^20 poses.  NONE of the defaults has been tuned on real data."""
    rotations: object = "yaw"
    yaw_steps: int = 72
    up: tuple = (0.0, 0.0, 1.0)
    axes: int = 96
    rolls: int = 24
    offsets: int = 0
    offset_step: float = 0.1
    anchors: object = None
    sample: int = 1024
    radius: float = None
    keep: int = 8

    def __post_init__(self):
        def array(v, tail, what):
            try:
                a = np.array(v, dtype=np.float64)
            except (TypeError, ValueError):
                a = None
            if a is None or a.ndim != len(tail) + 1 or a.shape[1:] != tail or not 1 <= len(a) <= MAX_POSES or not np.isfinite(a).all():
                raise ValueError(f"SearchConfig: {what} must be a finite [n, {', '.join(map(str, tail))}] array with 1 <= n <= 2^20, got {v!r}")
            a.setflags(write=False)
            return a
        if isinstance(self.rotations, str):
            if self.rotations not in ("yaw", "so3"):
                raise ValueError(f'SearchConfig: rotations must be "yaw", "so3" or an [R, 3, 3] array, got {self.rotations!r}')
        else:
            Rs = array(self.rotations, (3, 3), "rotations")
            if np.abs(Rs @ Rs.transpose(0, 2, 1) - np.eye(3)).max() > 1e-6 or np.abs(np.linalg.det(Rs) - 1.0).max() > 1e-6:
                raise ValueError("SearchConfig: every matrix of rotations must be orthonormal with determinant +1 (to 1e-6)")
            object.__setattr__(self, "rotations", Rs)
        for name, hi in (("yaw_steps", MAX_POSES), ("axes", MAX_POSES), ("rolls", MAX_POSES), ("sample", 1 << 28), ("keep", 1024)):
            if not _integer(getattr(self, name), 1, hi):
                raise ValueError(f"SearchConfig: {name} must be an integer in 1 .. {hi}, got {getattr(self, name)!r}")
        if not _integer(self.offsets, 0, 16):
            raise ValueError(f"SearchConfig: offsets must be an integer in 0 .. 16, got {self.offsets!r}")
        if not _number(self.offset_step) or not self.offset_step > 0:
            raise ValueError(f"SearchConfig: offset_step must be a finite positive number, got {self.offset_step!r}")
        up = self.up
        if not isinstance(up, (tuple, list)) or len(up) != 3 or not all(_number(v) for v in up) or not any(v != 0 for v in up):
            raise ValueError(f"SearchConfig: up must be three finite numbers, not all zero, got {up!r}")
        object.__setattr__(self, "up", tuple(float(v) for v in up))
        if self.anchors is not None:
            object.__setattr__(self, "anchors", array(self.anchors, (3,), "anchors"))
        if self.radius is not None:
            if not _number(self.radius):
                raise ValueError(f"SearchConfig: radius must be None or a finite positive number, got {self.radius!r}")
            ops.transfer_radius(self.radius)
        if self.num_rotations * (1 if self.anchors is None else len(self.anchors)) * (2 * self.offsets + 1) ** 3 > MAX_POSES:
            raise ValueError(f"SearchConfig: {self.num_rotations} rotations x {1 if self.anchors is None else len(self.anchors)} anchors x "
                             f"{(2 * self.offsets + 1) ** 3} offsets exceed 2^20 poses")

    @property
    def num_rotations(self) -> int:
        if isinstance(self.rotations, str):
            return self.yaw_steps if self.rotations == "yaw" else self.axes * self.rolls
        return len(self.rotations)


@dataclasses.dataclass
class SearchRecord:
    """What `search` did.  poses: the candidates scored; sample: the queries they were scored on; candidates: per refined candidate, in the order
    refined (best count first), dict(pose_index, count, pairs, rms, converged); chosen: the position in `candidates` of the one returned."""
    poses: int
    sample: int
    candidates: list
    chosen: int


def _axis_rotation(axis, angle: float) -> np.ndarray:
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def rotation_to(d) -> np.ndarray:
    """The shortest-arc rotation [3, 3] fp64 that takes +z to the direction d (normalised here): about z x d by the angle between them; for d = -z,
    where every axis in the xy plane is as short, the half turn about x."""
    d = np.asarray(d, dtype=np.float64).reshape(3)
    d = d / np.linalg.norm(d)
    s2 = d[0] * d[0] + d[1] * d[1]                                                # sin^2 of the angle, |z x d|^2
    if d[2] < 0 and s2 < 1e-200:
        return np.diag([1.0, -1.0, -1.0])
    K = np.array([[0.0, 0.0, d[0]], [0.0, 0.0, d[1]], [-d[0], -d[1], 0.0]])       # the cross-product matrix of v = z x d = (-d_y, d_x, 0)
    # I + K + K^2 (1 - cos) / sin^2; (1 - cos) / sin^2 = 1 / (1 + cos), each form used where it does not cancel
    return np.eye(3) + K + (K @ K) * (1.0 / (1.0 + d[2]) if d[2] >= 0 else (1.0 - d[2]) / s2)


def rotation_grid(cfg: SearchConfig) -> np.ndarray:
    """-> [R, 3, 3] fp64.  "yaw": entry k turns by 2 pi k / yaw_steps about `up` (entry 0 is the identity).  "so3": direction k of the Fibonacci
    sphere is d_k = (s cos(k g), s sin(k g), z_k) with z_k = 1 - (2 k + 1) / axes, s = sqrt(1 - z_k^2), g the golden angle pi (3 - sqrt 5); entry
    k * rolls + j = rotation_to(d_k) composed with the roll by 2 pi j / rolls about +z (the roll first).  An explicit array: itself."""
    if not isinstance(cfg, SearchConfig):
        raise TypeError(f"rotation_grid: cfg must be a SearchConfig, got {type(cfg).__name__}")
    if not isinstance(cfg.rotations, str):
        return np.array(cfg.rotations)
    if cfg.rotations == "yaw":
        return np.stack([_axis_rotation(cfg.up, 2.0 * math.pi * k / cfg.yaw_steps) for k in range(cfg.yaw_steps)])
    rolls = [_axis_rotation((0.0, 0.0, 1.0), 2.0 * math.pi * j / cfg.rolls) for j in range(cfg.rolls)]
    out = np.empty((cfg.axes, cfg.rolls, 3, 3))
    for k in range(cfg.axes):
        z = 1.0 - (2 * k + 1) / cfg.axes
        s = math.sqrt(max(0.0, 1.0 - z * z))
        tilt = rotation_to((s * math.cos(k * GOLDEN_ANGLE), s * math.sin(k * GOLDEN_ANGLE), z))
        for j in range(cfg.rolls):
            out[k, j] = tilt @ rolls[j]
    return out.reshape(-1, 3, 3)


def candidate_poses(cfg: SearchConfig, source_centroid, query_centroid) -> np.ndarray:
    """-> [P, 3, 4] fp64, query frame -> source frame: for each rotation R of rotation_grid, each anchor c (cfg.anchors, or the source centroid) and
    each offset o of the lattice, [R | c - R q + o] with q the query centroid -- the pose that turns the queries by R about their centroid and puts
    it at c + o.  Index = (rotation * anchors + anchor) * offsets + offset; offset = ((k + g) (2 g + 1) + (j + g)) (2 g + 1) + (i + g) for
    o = offset_step * (i, j, k): x runs fastest."""
    Rs = rotation_grid(cfg)
    q = np.asarray(query_centroid, dtype=np.float64).reshape(3)
    anchors = np.asarray(source_centroid, dtype=np.float64).reshape(1, 3) if cfg.anchors is None else cfg.anchors
    if not (np.isfinite(q).all() and np.isfinite(anchors).all()):
        raise ValueError("candidate_poses: the centroids must be finite")
    g = cfg.offsets
    steps = np.arange(-g, g + 1, dtype=np.float64) * float(cfg.offset_step)
    oz, oy, ox = np.meshgrid(steps, steps, steps, indexing="ij")
    offs = np.stack([ox.reshape(-1), oy.reshape(-1), oz.reshape(-1)], 1)                 # x fastest
    t = (anchors[None, :, None, :] - (Rs @ q)[:, None, None, :]) + offs[None, None, :, :]  # [R, A, O, 3]
    out = np.empty(t.shape[:3] + (3, 4))
    out[..., :3] = Rs[:, None, None]
    out[..., 3] = t
    return out.reshape(-1, 3, 4)


def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def sample_positions(n: int, sample: int) -> np.ndarray:
    """Which of n participating queries (in index order) are scored: all of them for n <= sample, else the ones at positions (k n) // sample."""
    return np.arange(n, dtype=np.int64) if n <= sample else (np.arange(sample, dtype=np.int64) * n) // sample


def search(index, xyz, cfg: SearchConfig, icp_cfg: AlignConfig, bits=None, score=None, step=None, normals=None, plane=None) -> Alignment:
    """A pose without a starting pose.  index: ops.transfer_index of the sources at icp_cfg.radius (anything with `src_xyz` when `score` and `step`
    are stand-ins); xyz [M, 3] the queries; bits: an optional packed row, the queries that take part -> Alignment, its `search` a SearchRecord.
      1. the queries scored: sample_positions among the participating ones, in index order -- deterministic (with bits, one host read of the row)
      2. the centroids of the sources and of those queries, in fp64; candidate_poses
      3. ONE ops.align_score over all candidates at cfg.radius (None: icp_cfg.radius), and one host read of the P counts
      4. the candidates ordered by (-count, index); the first cfg.keep each refined by icp(index, xyz, icp_cfg, init=pose, bits=bits, step=step)
      5. the refinement with the most pairs; ties go to the lower rms, then to the earlier candidate.  Where none has a pair, the first one's
         Alignment (converged=False, its reason says why).
    score / step: stand-ins for ops.align_score / ops.align_step with their signatures (a reference, a test).
    normals / plane: passed to every refinement (icp: point-to-plane); the scoring is the same."""
    if not isinstance(cfg, SearchConfig):
        raise TypeError(f"search: cfg must be a SearchConfig, got {type(cfg).__name__}")
    if not isinstance(icp_cfg, AlignConfig):
        raise TypeError(f"search: icp_cfg must be an AlignConfig, got {type(icp_cfg).__name__}")
    if normals is None and plane is not None:
        raise ValueError("search: plane configures point-to-plane ICP and needs normals")
    radius = icp_cfg.radius if cfg.radius is None else cfg.radius
    if radius > icp_cfg.radius:
        raise ValueError(f"search: the scoring radius {radius} exceeds the AlignConfig's {icp_cfg.radius}, the cell size of the index")
    score = ops.align_score if score is None else score
    rows = xyz[0] if len(xyz.shape) == 3 and xyz.shape[0] == 1 else xyz
    M = rows.shape[0]
    if bits is None:
        part = None
        n = M
    else:
        words = _host(bits).reshape(-1).view(np.uint64)
        part = np.nonzero(((words[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(-1)[:M])[0]
        n = len(part)
    if n == 0:
        raise ValueError("search: no query takes part")
    pick = sample_positions(n, cfg.sample)
    if part is not None:
        pick = part[pick]
    if hasattr(rows, "detach"):
        import torch
        picked = rows if part is None and n <= cfg.sample else rows.index_select(0, torch.from_numpy(pick).to(rows.device))
        picked = picked.contiguous()
        qc = _host(picked.double().mean(0))
    else:
        picked = np.ascontiguousarray(np.asarray(rows)[pick])
        qc = picked.astype(np.float64).mean(0)
    src = index.src_xyz
    sc = _host(src.double().mean(0)) if hasattr(src, "detach") else np.asarray(src, dtype=np.float64).mean(0)
    if not (np.isfinite(qc).all() and np.isfinite(sc).all()):
        raise ValueError("search: the sources and the scored queries must be finite")
    poses = candidate_poses(cfg, sc, qc)
    counts = _host(score(index, picked, poses, radius)).astype(np.int64).reshape(-1)      # the one host read of the scoring
    if counts.shape != (len(poses),):
        raise ValueError(f"search: score must return one count per pose, got {counts.shape} for {len(poses)} poses")
    order = np.lexsort((np.arange(len(poses)), -counts))[:cfg.keep]
    runs, record = [], SearchRecord(len(poses), len(pick), [], 0)
    for p in order.tolist():
        out = icp(index, xyz, icp_cfg, init=poses[p], bits=bits, step=step, normals=normals, plane=plane)
        runs.append(out)
        record.candidates.append(dict(pose_index=p, count=int(counts[p]), pairs=out.pairs, rms=out.rms, converged=out.converged))
    best = 0
    for k in range(1, len(runs)):
        a, b = runs[k], runs[best]
        if a.pairs > b.pairs or (a.pairs == b.pairs and a.pairs > 0 and a.rms < b.rms):
            best = k
    record.chosen = best
    runs[best].search = record
    return runs[best]
