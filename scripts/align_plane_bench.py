"""Times one point-to-plane ICP step (csrc/align_plane.hip) next to the point-to-point step (csrc/align.hip) on the same index and queries, and runs
both alignments on a synthetic room to count their steps and measure what they reach.

    python scripts/align_plane_bench.py [--points 4194304] [--working 131072] [--repeats 20] [--out FILE.json] [--point-only]

One process, one GPU.  The clouds, the pose and the radius are scripts/align_bench.py's: scan A and scan B of scripts/scene_bench.py (a sphere shell, a
floor and two walls) with seeds 5 and 6, B given in a frame from which a small rigid pose leads back to A's; sources: A's working cloud (at most
`--working` points), queries: B's working cloud; radius: twice the working voxel size.  Normals: what predictor.snapshot(normals=True) keeps -- the
voxel normals of scan A (regions.build_graph, superpoints.estimate_normals with the default SuperpointConfig) at the working cloud's points.

  step        ops.align_plane_step (32 fp64 words) against ops.align_step (20) under the true pose: device-event times, median of `--repeats` after two
              warm-up rounds, with min and max, the two ALTERNATING.  The pairs are the same by construction; the script checks it on `nearest`.
  icp         align.icp from the identity with and without normals under one AlignConfig(radius, final_radius=radius / 2, shrink=0.8, iterations=60)
              and a default PlaneConfig: steps taken, why it stopped, the rotation and translation error against the true pose, wall time (every step
              ends in a host read of 256 or 160 bytes).

--point-only measures ops.align_step alone and touches nothing of the plane step: with PSAM_LIB_PATH naming another build of the library, the same
step on that build (the comparison against the commit before the plane step existed).  Every record says which it was: `point_only`, and
`library` = "in-tree" or "PSAM_LIB_PATH" (that another build was named, not its path).
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scene_bench import alternate, event, make_scan, stat, wall  # noqa: E402
from transfer_bench import rigid_pose  # noqa: E402

from point_sam_amd import align, ops, regions, scene, superpoints  # noqa: E402


def pose_error(pose, truth):
    """-> (the angle between the two rotations in radians, |translation difference|)."""
    c = (np.trace(pose[:, :3].T @ truth[:, :3]) - 1.0) / 2.0
    return math.acos(min(1.0, max(-1.0, c))), float(np.linalg.norm(pose[:, 3] - truth[:, 3]))


def clouds(M, working):
    pose = rigid_pose()
    axyz, _ = make_scan(M, 5)
    bxyz, _ = make_scan(M, 6)
    bxyz = ((bxyz.double() - pose[:, 3].cuda()) @ pose[:, :3].cuda()).float().clamp_(-1, 1).contiguous()      # q = R^T (p - t)
    h = scene.choose_voxel_size(axyz, working)
    keep = ops.voxel_downsample(axyz, h)[0]
    src = axyz.index_select(0, keep).contiguous()
    bwork = bxyz.index_select(0, ops.voxel_downsample(bxyz, scene.choose_voxel_size(bxyz, working))[0]).contiguous()
    return pose, axyz, keep, src, bwork, h


def run(M, working, repeats, point_only):
    pose, axyz, keep, src, bwork, h = clouds(M, working)
    radius = 2 * h
    index = ops.transfer_index(src, radius)
    res = dict(points=M, max_points=working, voxel_size=h, sources=src.shape[0], queries=bwork.shape[0], radius=radius, repeats=repeats,
               point_only=point_only, library="PSAM_LIB_PATH" if os.environ.get("PSAM_LIB_PATH") else "in-tree")
    if point_only:
        times = [event(lambda: ops.align_step(index, bwork, pose))[1] for _ in range(repeats + 2)][2:]
        res["step"] = dict(point_ms=stat(times), pairs=int(ops.align_step(index, bwork, pose)[0]))
        return res
    graph = regions.build_graph(axyz)
    normals = superpoints.estimate_normals(graph, axyz).per_point()[0].index_select(0, keep).contiguous()
    res.update(normals_voxel_size=graph.voxel_size, sources_without_a_normal=int((normals == 0).all(1).sum()))
    (plane, near_a), (point, near_b) = ops.align_plane_step(index, bwork, normals, pose, return_nearest=True), ops.align_step(index, bwork, pose, return_nearest=True)
    assert torch.equal(near_a, near_b) and plane[0] + plane[30] == point[0] and plane[31] == point[19], (plane.tolist(), point.tolist())
    a, b = alternate(lambda: ops.align_plane_step(index, bwork, normals, pose), lambda: ops.align_step(index, bwork, pose), event, repeats)
    res["step"] = dict(plane_ms=stat(a), point_ms=stat(b), plane_over_point=round(float(np.median(a) / np.median(b)), 3), pairs=int(point[0]),
                       used_pairs=int(plane[0]), unused_pairs=int(plane[30]))
    cfg = align.AlignConfig(radius, final_radius=radius / 2, shrink=0.8, iterations=60)
    truth = pose.numpy()
    for name, kw in (("plane", dict(normals=normals)), ("point", dict())):
        out = align.icp(index, bwork, cfg, **kw)
        times = [wall(lambda: align.icp(index, bwork, cfg, **kw))[1] for _ in range(min(repeats, 5) + 1)][1:]
        rot, tr = pose_error(out.pose, truth)
        res[f"icp_{name}"] = dict(iterations=out.iterations, converged=out.converged, reason=out.reason, pairs=out.pairs, coverage=round(out.coverage, 4),
                                  rms=out.rms, rotation_error_rad=rot, translation_error=tr, wall_ms=stat(times))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4194304")
    ap.add_argument("--working", type=int, default=131072)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--point-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = []
    for M in (int(m) for m in args.points.split(",")):
        res = run(M, args.working, args.repeats, args.point_only)
        print(json.dumps(res), flush=True)
        out.append(res)
        torch.cuda.empty_cache()
        if args.out:                                       # after every configuration: a run that is cut short keeps what it measured
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
