"""Scan map relocalisation (include/pointsam_hip.h, "scan map relocalisation"; ScanMap.track_score, ScanMap.relocalize, ScanMap.anchors) in plain
numpy, from the definitions and independent of the package.

    score     counts[p] = the number of scored queries with at least one candidate under pose p = the queries tests/track_reference.py's nearest
              pairs: the posed copy of the sample (scanmap_reference.posed, the pose's fp32 words) is handed to nearest WITHOUT a pose, which does no
              arithmetic on it, so the posed coordinate, the cell and the candidates are track_reference.step's
    search    tests/align_search_reference.py's rules (candidates, sample, ordering, choice) with `score` above and track_reference.icp as the refinement
    anchors   the pairable voxels grouped by coarse cell (each cell coordinate // cells); per coarse cell with at least min_voxels of them the fp64
              sum of their fp32 means taken in id order, divided by their number; ordered by coarse (cz, cy, cx)
"""
import numpy as np

import align_reference as AR
import align_search_reference as ASR
import scanmap_reference as SM
import track_reference as TR

F = np.float32


def score(ref, sample, poses, radius, reach=None, r2=None, V=None, skip=None, min_count=1, definition=False):
    """-> counts [P] int64.  Blocked over the poses (bounded memory: 2^19 posed points at a time); definition=True: on nearest_definition, query by
    query.  reach None: track_reference.reach_of(radius, the map's voxel size); r2: the fp32 bound itself instead of fl32(radius * radius)."""
    find = TR.nearest_definition if definition else TR.nearest
    sample = np.ascontiguousarray(sample, dtype=F)
    P, m = len(poses), len(sample)
    reach = max(1, int(np.ceil(float(F(radius)) * float(ref.inv_h)))) if reach is None else reach
    r2 = TR.r2_of(radius) if r2 is None else F(r2)
    out = np.zeros(P, dtype=np.int64)
    block = max(1, (1 << 19) // m)
    for lo in range(0, P, block):
        part = poses[lo:lo + block]
        with np.errstate(all="ignore"):
            posed = np.concatenate([SM.posed(sample, SM.pose_words(p)) for p in part], 0)
        near = find(ref, posed, r2, reach, None, None, V, skip, min_count)[0]
        out[lo:lo + len(part)] = (near >= 0).reshape(len(part), m).sum(1)
    return out


def seven_poses():
    """The poses every step case is scored under: the identity, align_reference.TRUE_POSE, a half turn, a translation of 3e6 (every query leaves the
    map) and three seeded random rigid poses with small translations."""
    g = np.random.default_rng(5)
    out = [np.eye(4)[:3], AR.TRUE_POSE, np.concatenate([AR.rotation([0, 0, 1], 180.0), np.zeros((3, 1))], 1),
           np.concatenate([np.eye(3), np.full((3, 1), 3e6)], 1)]
    for _ in range(3):
        out.append(np.concatenate([AR.rotation(g.normal(size=3), float(g.uniform(0, 360))), g.uniform(-0.1, 0.1, size=(3, 1))], 1))
    return np.stack(out)


def pairable(ref, occupied=None, min_count=1):
    ok = np.asarray(ref.count, dtype=np.int64).reshape(ref.V) >= min_count
    return ok if occupied is None else ok & np.asarray(occupied, dtype=bool)


def anchors(keys, means, ok, cells=8, min_voxels=8):
    """keys [V] int64 (cx | cy << 21 | cz << 42), means [V, 3] float32, ok [V] bool -> [A, 3] float64."""
    groups = {}
    for v in range(len(keys)):
        if ok[v]:
            k = int(keys[v])
            c = tuple(((k >> (21 * a)) & ((1 << 21) - 1)) // cells for a in range(3))
            groups.setdefault((c[2], c[1], c[0]), []).append(v)
    out = []
    for c in sorted(groups):
        if len(groups[c]) >= min_voxels:
            s = np.zeros(3)
            for v in groups[c]:                                    # id order
                s = s + np.asarray(means[v], dtype=np.float64)
            out.append(s / len(groups[c]))
    return np.array(out, dtype=np.float64).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------ the search fixture
# Sources: a RefMap of align_search_reference.yaw_case()'s cloud a, added once under the identity at SEARCH_H with max_voxels 8192: 2134 voxels.
# Queries: yaw_case()'s b, 4405 of them.  ICP: align_search_reference.ICP (radius 0.1 = reach 4).  The grid: 72 yaw steps x offsets 1 at step 0.1 =
# 1944 poses, scored on 512 sampled queries at radius 0.06 (reach 2); the best 8 refined.  The source centroid is the fp64 numpy mean of the 2134
# voxel means.
SEARCH_H, SEARCH_MAX_VOXELS, SEARCH_VOXELS, SEARCH_QUERIES, SEARCH_POSES = 2.0 ** -5, 8192, 2134, 4405, 1944
# What search_fixture() below was measured to do on the CPU; tests/test_track_score_cpu.py recomputes and holds all of it.
#   The eight best-scoring poses and their counts of 512 (the median over the 1944 poses is 139).  The first six refine to all 4405 pairs; the last
#   two end in a false optimum with 2982 and 2918 pairs, about 0.10 off in translation.  Chosen: position 1 (pose 738), by the lower rms among the
#   ties at 4405 pairs: 1.5769e-3 rad and 6.8429e-4 off the truth.  Reference ICP STARTED AT the truth converges at step 24 with rms 0.0145862 and is
#   1.5631e-3 rad and 6.6583e-4 off -- the map is a cloud of voxel means, not the surface.  From the identity: 410 pairs, not converged, 2.16 rad off.
SEARCH_ORDER, SEARCH_COUNTS, SEARCH_MEDIAN = [765, 738, 792, 711, 819, 684, 766, 739], [488, 487, 455, 408, 395, 389, 366, 362], 139
SEARCH_PAIRS = [4405, 4405, 4405, 4405, 4405, 4405, 2982, 2918]
SEARCH_CHOSEN, SEARCH_ROTATION_ERROR, SEARCH_TRANSLATION_ERROR = 1, 1.5769e-3, 6.8429e-4
REF_ITERATIONS, REF_RMS, REF_ROTATION_ERROR, REF_TRANSLATION_ERROR = 24, 0.0145862, 1.5631e-3, 6.6583e-4
IDENTITY_PAIRS, IDENTITY_ROTATION_ERROR = 410, 2.16


def search_case():
    """-> (RefMap, a, b)."""
    a, b = ASR.yaw_case()
    ref = SM.RefMap(SEARCH_H, SEARCH_MAX_VOXELS)
    ref.add(a, np.zeros_like(a))
    return ref, a, b


def search_centroid(ref):
    return TR.means(ref).astype(np.float64).mean(0)


def search_poses(ref, b):
    """-> (poses [1944, 3, 4] float64, picked: the positions of the scored queries)."""
    picked = np.asarray(ASR.sample_positions(len(b), ASR.SAMPLE))
    poses = ASR.candidates(ASR.yaw_grid(ASR.YAW_STEPS), search_centroid(ref), b[picked].astype(np.float64).mean(0), ASR.YAW_OFFSETS, ASR.YAW_OFFSET_STEP)
    return poses, picked


def refine(ref, b, init=None):
    c = ASR.ICP
    return TR.icp(ref, b, c["radius"], c["final_radius"], c["shrink"], c["iterations"], init=init)


def search_fixture():
    """The whole search in numpy -> dict(counts, order, runs, chosen, poses, picked)."""
    ref, _, b = search_case()
    poses, picked = search_poses(ref, b)
    counts = score(ref, b[picked], poses, ASR.SCORE_RADIUS)
    order = ASR.ordered(counts, ASR.KEEP)
    runs = [refine(ref, b, poses[p]) for p in order]
    return dict(ref=ref, b=b, counts=counts, order=order, runs=runs, chosen=ASR.choose(runs), poses=poses, picked=picked)
