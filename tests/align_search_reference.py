"""Plain numpy reference of the global pose search (point_sam_amd/align.py: search; ops.align_score), written from the definitions and independent of
the package.  Scoring is the existing definition of a pair (tests/align_reference.py: nearest), refinement is align_reference.icp.

    score              counts[p] = the number of scored queries with at least one candidate under pose p = the queries align_reference.nearest pairs
    rotations          "yaw": k -> the turn by 2 pi k / n about `up`.  "so3": direction k of the Fibonacci sphere, z_k = 1 - (2 k + 1) / axes, azimuth
                       k * pi (3 - sqrt 5); the shortest-arc rotation taking +z to it (for -z the half turn about x), applied after a roll by
                       2 pi j / rolls about +z; index k * rolls + j
    candidates         [R | c - R q + o] for each rotation R, each anchor c, each lattice offset o = step * (i, j, k), -g <= i, j, k <= g; row-major over
                       (rotation, anchor, offset), within the offsets x fastest
    sample             n participating queries, in index order: all of them for n <= sample, else the ones at positions (k n) // sample
    selection          candidates ordered by (-count, index); the first `keep` refined; the most pairs wins, then the lower rms, then the earlier
"""
import math

import numpy as np

import align_reference as A
import transfer_reference as T

f32 = np.float32
GOLDEN = math.pi * (3.0 - math.sqrt(5.0))


def score(src, r_index, sample, poses, radius, r2=None):
    """-> counts [P] int64.  One call of the vectorised nearest over the P posed copies of the sample (a posed copy is passed without a pose).  r2: the
    fp32 bound itself instead of fl32(radius * radius)."""
    src, sample = np.asarray(src, dtype=f32), np.asarray(sample, dtype=f32)
    P, m = len(poses), len(sample)
    r2 = A.r2_of(radius) if r2 is None else f32(r2)
    out = np.zeros(P, dtype=np.int64)
    block = max(1, (1 << 19) // m)                                  # bounded memory: 2^19 posed points at a time
    for lo in range(0, P, block):
        part = poses[lo:lo + block]
        posed = np.concatenate([T.posed(sample, np.asarray(p, dtype=np.float64)[:3].astype(f32)) for p in part], 0)
        near = A.nearest(src, r_index, posed, r2)[0]
        out[lo:lo + len(part)] = (near >= 0).reshape(len(part), m).sum(1)
    return out


def turn(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    c, s = math.cos(angle), math.sin(angle)
    return c * np.eye(3) + s * np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]) + (1 - c) * np.outer(a, a)


def from_z(d):
    """The shortest-arc rotation taking +z to the unit vector d, by the angle-axis form; the half turn about x for d = -z."""
    d = np.asarray(d, dtype=np.float64)
    d = d / np.linalg.norm(d)
    v = np.cross([0.0, 0.0, 1.0], d)
    s = np.linalg.norm(v)
    if s < 1e-12:
        return np.eye(3) if d[2] > 0 else np.diag([1.0, -1.0, -1.0])
    return turn(v / s, math.atan2(s, d[2]))


def yaw_grid(steps, up=(0.0, 0.0, 1.0)):
    return np.stack([turn(up, 2 * math.pi * k / steps) for k in range(steps)])


def fibonacci(axes):
    k = np.arange(axes)
    z = 1.0 - (2 * k + 1) / axes
    s = np.sqrt(1.0 - z * z)
    return np.stack([s * np.cos(k * GOLDEN), s * np.sin(k * GOLDEN), z], 1)


def so3_grid(axes, rolls):
    return np.stack([from_z(d) @ turn([0.0, 0.0, 1.0], 2 * math.pi * j / rolls) for d in fibonacci(axes) for j in range(rolls)])


def lattice(g, step):
    return np.array([[i * step, j * step, k * step] for k in range(-g, g + 1) for j in range(-g, g + 1) for i in range(-g, g + 1)], dtype=np.float64)


def candidates(rotations, anchors, query_centroid, g=0, step=0.1):
    q = np.asarray(query_centroid, dtype=np.float64)
    out = []
    for Rm in rotations:
        for c in np.asarray(anchors, dtype=np.float64).reshape(-1, 3):
            for o in lattice(g, step):
                out.append(np.concatenate([Rm, (c - Rm @ q + o)[:, None]], 1))
    return np.stack(out)


def sample_positions(n, sample):
    return list(range(n)) if n <= sample else [(k * n) // sample for k in range(sample)]


def ordered(counts, keep):
    return sorted(range(len(counts)), key=lambda p: (-int(counts[p]), p))[:keep]


def choose(runs):
    """runs: dicts with pairs and rms, in the order refined -> the position of the winner."""
    return min(range(len(runs)), key=lambda k: (-runs[k]["pairs"], runs[k]["rms"] if runs[k]["pairs"] > 0 else math.inf, k))


def search(src, qry, rotations, icp, g=0, step=0.1, sample=1024, radius=None, keep=8, anchors=None, take=None):
    """icp: dict(radius, final_radius, shrink, iterations) -> dict(counts, order, runs, chosen, poses, picked)."""
    src, qry = np.asarray(src, dtype=f32), np.asarray(qry, dtype=f32)
    part = np.arange(len(qry)) if take is None else np.nonzero(take)[0]
    picked = part[sample_positions(len(part), sample)]
    sc = src.astype(np.float64).mean(0)
    poses = candidates(rotations, sc if anchors is None else anchors, qry[picked].astype(np.float64).mean(0), g, step)
    counts = score(src, icp["radius"], qry[picked], poses, icp["radius"] if radius is None else radius)
    order = ordered(counts, keep)
    runs = [A.icp(src, qry, init=poses[p], take=take, **icp) for p in order]
    return dict(counts=counts, order=order, runs=runs, chosen=choose(runs), poses=poses, picked=picked)


# ------------------------------------------------------------------------------------------------ the fixtures
# Sources surfaces(6000, 21), queries surfaces(6100, 22) (tests/align_reference.py: no rotational symmetry), the queries given in a frame from which
# the TRUTH leads back to the sources'.  Far from the identity: plain ICP from the identity does not get there.
TRANSLATION = np.array([0.3, -0.2, 0.1])
YAW_TRUTH = np.concatenate([A.rotation([0, 0, 1], 132.0), TRANSLATION[:, None]], 1)             # (a)
SO3_TRUTH = np.concatenate([A.rotation([0.3, -0.5, 0.8], 130.0), TRANSLATION[:, None]], 1)      # (b)
ICP = dict(radius=0.1, final_radius=0.04, shrink=0.9, iterations=60)
SCORE_RADIUS, SAMPLE, KEEP = 0.06, 512, 8
YAW_STEPS, YAW_OFFSETS, YAW_OFFSET_STEP = 72, 1, 0.1               # 72 x 27 = 1944 poses
SO3_AXES, SO3_ROLLS, SO3_KEEP = 96, 24, 4                          # 2304 poses, the centroid match alone
# What the reference (search below with the settings above) was measured to do; tests/test_align_search_cpu.py recomputes and holds all of it.
# REF_*_ERROR: what plain reference ICP (align_reference.icp under ICP) reaches against the truth when STARTED AT the truth -- a good start.
#   (a) all 4405 queries paired from the truth (converged at step 16, rms 0.010688): rotation off by 2.1688e-3 rad, translation by 9.6339e-4.  The eight
#       best-scoring poses, their counts of 512 (the median over the 1944 is 143); seven refine to all 4405 pairs (errors 1.92e-3 .. 2.30e-3 rad,
#       6.9e-4 .. 1.12e-3), the eighth into a false optimum with 2985 pairs, 0.106 off in translation.  Chosen: the first, 2.1493e-3 rad and 9.6059e-4.
#   (b) all 6100 paired from the truth (step 30, rms 0.010680): 1.4619e-3 rad, 3.7303e-4.  The four best-scoring poses and their counts (median 145);
#       all four refine to 6100 pairs, the third has the lowest rms and is chosen: 1.9129e-3 rad and 5.3500e-4.
YAW_REF_ROTATION_ERROR, YAW_REF_TRANSLATION_ERROR = 2.1688e-3, 9.6339e-4
YAW_ORDER, YAW_COUNTS = [738, 765, 792, 711, 819, 684, 766, 712], [501, 485, 451, 432, 389, 380, 363, 361]
SO3_REF_ROTATION_ERROR, SO3_REF_TRANSLATION_ERROR = 1.4619e-3, 3.7303e-4
SO3_ORDER, SO3_COUNTS = [872, 561, 560, 679], [422, 398, 388, 371]


def _case(truth, cut):
    a, b_in_a = A.surfaces(6000, 21), A.surfaces(6100, 22)
    if cut:
        b_in_a = b_in_a[b_in_a[:, 0] < 0.1]                        # the second scan sees only part of the scene
    b = (b_in_a - truth[:, 3]) @ truth[:, :3]                      # q = R^T (p - t)
    return a.astype(f32), b.astype(f32)


def yaw_case():
    """(a): 132 degrees about z, and the queries are the part of the second sample with x < 0.1 in the sources' frame: a partial overlap."""
    return _case(YAW_TRUTH, True)


def so3_case():
    """(b): 130 degrees about a skew axis, full overlap."""
    return _case(SO3_TRUTH, False)
