"""The pose between two scans: point-to-point ICP on the transfer index (csrc/align.hip, ops.align_step, predictor.align).

transfer.py carries masks from one scan to the next given the rigid motion that remains between them once both are normalised with the same centre
and scale.  Two re-scans of a room rarely come with that motion, and odometry is a few centimetres off; a wrong pose does not fail loudly, the masks
land beside their objects.  `icp` estimates it: every step pairs each query with its nearest source within a radius and sums what the closed-form
solution needs in ONE launch (ops.align_step: 20 fp64 words, bit-reproducible), the host reads those 160 bytes and solves a 3 x 3 SVD (`solve_rigid`).
The sums are over the queries AS GIVEN, so each step solves for the whole pose: nothing is composed, nothing drifts.

ICP is a local method: it refines an initial pose (the identity, or odometry) whose error is small against the search radius and the scene's
structure; it does not search globally.  `Alignment.coverage` and `rms` say how far to trust the answer.
"""
import dataclasses

import numpy as np

from . import ops


@dataclasses.dataclass(frozen=True)
class AlignConfig:
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

    def __post_init__(self):
        def number(v):
            return not isinstance(v, bool) and isinstance(v, (int, float)) and v == v and abs(v) != float("inf")

        def integer(v, lo, hi):
            return not isinstance(v, bool) and isinstance(v, int) and lo <= v <= hi
        if not number(self.radius):
            raise ValueError(f"AlignConfig: radius must be a finite positive number, got {self.radius!r}")
        ops.transfer_radius(self.radius)
        if self.final_radius is not None:
            if not number(self.final_radius) or not 0 < self.final_radius <= self.radius:
                raise ValueError(f"AlignConfig: final_radius must be None or lie in (0, radius], got {self.final_radius!r}")
            ops.transfer_radius(self.final_radius)
        if not number(self.shrink) or not 0 < self.shrink <= 1:
            raise ValueError(f"AlignConfig: shrink must lie in (0, 1], got {self.shrink!r}")
        if not integer(self.iterations, 1, 10000):
            raise ValueError(f"AlignConfig: iterations must be an integer in 1 .. 10000, got {self.iterations!r}")
        if not integer(self.min_pairs, 3, 1 << 28):
            raise ValueError(f"AlignConfig: min_pairs must be an integer in 3 .. 2^28, got {self.min_pairs!r}")
        for name in ("tol_rotation", "tol_translation"):
            v = getattr(self, name)
            if not number(v) or v < 0:
                raise ValueError(f"AlignConfig: {name} must be a finite number >= 0, got {v!r}")

    @classmethod
    def from_overrides(cls, data: dict) -> "AlignConfig":
        """A config from a dict of fields (a request's body): an unknown field is a ValueError, like a bad value."""
        names = {f.name for f in dataclasses.fields(cls)}
        if not isinstance(data, dict) or set(data) - names or "radius" not in data:
            raise ValueError(f"AlignConfig takes radius and optionally {sorted(names - {'radius'})}, got {sorted(data) if isinstance(data, dict) else data!r}")
        return cls(**data)

    def step_radius(self, k: int) -> float:
        """The search radius of step k."""
        last = self.radius if self.final_radius is None else self.final_radius
        return max(float(last), float(self.radius) * float(self.shrink) ** k)


@dataclasses.dataclass
class Alignment:
    """icp's answer.  pose: 3 x 4 fp64, query frame -> source frame: what transfer_masks / propagate take.  pairs, rms: of the last step whose solve
    succeeded -- its pairs were found under the pose BEFORE that solve, rms is their root mean square distance AFTER it; coverage = pairs / the
    participating queries that have a cell.  history: (pairs, rms, radius) per step taken."""
    pose: np.ndarray
    pairs: int
    coverage: float
    rms: float
    iterations: int
    converged: bool
    reason: str
    history: list


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


def _initial(init) -> np.ndarray:
    if init is None:
        return np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    ops.transfer_pose(init)
    P = np.asarray(init.detach().cpu().numpy() if hasattr(init, "detach") else init, dtype=np.float64)[:3]
    return P.copy()


def _rotation_angle(A, B) -> float:
    c = (np.trace(A[:, :3].T @ B[:, :3]) - 1.0) / 2.0
    return float(np.arccos(min(1.0, max(-1.0, c))))


def icp(index, xyz, cfg: AlignConfig, init=None, bits=None, step=None) -> Alignment:
    """index: ops.transfer_index of the sources at cfg.radius; xyz [M, 3] the queries; init: the pose to start from (None: the identity); bits: an
    optional packed row, the queries that take part -> Alignment.  Each step is one ops.align_step under the current pose, one 160-byte host read
    and one solve_rigid.  Stops converged when the twelve fp32 words of the new pose equal the previous step's at the final radius (the next step
    would be bit-identical: a fixed point), or when both tolerances are positive and met there; stops unconverged, with the last good pose, when a
    step has fewer than cfg.min_pairs pairs or a degenerate solve, or when the iterations run out.  `step`: a stand-in for ops.align_step with its
    signature (a reference, a test)."""
    if not isinstance(cfg, AlignConfig):
        raise TypeError(f"icp: cfg must be an AlignConfig, got {type(cfg).__name__}")
    step = ops.align_step if step is None else step
    pose = _initial(init)
    last = cfg.step_radius(10 ** 9)
    out = Alignment(pose, 0, 0.0, float("nan"), 0, False, "iterations", [])
    for k in range(cfg.iterations):
        radius = cfg.step_radius(k)
        sums = step(index, xyz, pose, radius, bits)
        sums = np.asarray(sums.cpu().numpy() if hasattr(sums, "cpu") else sums, dtype=np.float64)      # the one host read of the step
        out.iterations = k + 1
        pairs = int(sums[0])
        if pairs < cfg.min_pairs:
            out.history.append((pairs, float("nan"), radius))
            out.reason = f"pairs: {pairs} < min_pairs {cfg.min_pairs}"
            return out
        try:
            new, rms = solve_rigid(sums)
        except ValueError as e:
            out.history.append((pairs, float("nan"), radius))
            out.reason = str(e)
            return out
        out.history.append((pairs, rms, radius))
        fixed = np.array_equal(new.astype(np.float32), pose.astype(np.float32))
        small = (cfg.tol_rotation > 0 and cfg.tol_translation > 0 and _rotation_angle(pose, new) <= cfg.tol_rotation and
                 float(np.linalg.norm(new[:, 3] - pose[:, 3])) <= cfg.tol_translation)
        pose = new
        out.pose, out.pairs, out.rms, out.coverage = pose, pairs, rms, pairs / max(sums[19], 1.0)
        if radius == last and (fixed or small):
            out.converged, out.reason = True, "fixed point" if fixed else "tolerance"
            return out
    return out
