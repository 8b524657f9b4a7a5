"""Times one ICP step and a full alignment (csrc/align.hip, point_sam_amd/align.py) next to a form composed from torch and the public transfer ops.

    python scripts/align_bench.py [--points 4194304] [--working 131072] [--repeats 20] [--out FILE.json]

One process, one GPU.  Sources: the working cloud (at most `--working` points) of one synthetic scan of scripts/scene_bench.py.  Queries: a second scan
(another seed) given in a frame from which a small rigid pose leads back to the first -- once its working cloud (what predictor.align searches), once
all `--points` points.  Radius: twice the working voxel size.  Each figure is the median of `--repeats` device-event times after two warm-up rounds, with
min and max; the two forms ALTERNATE.

  step        ops.align_step (one pair launch, one combine launch, 160 bytes out) against the composed step: ops.transfer_plan -> idx3[:, 0] -> gathers
              of the pairs -> fp64 products and torch.sum reductions.  The composed step keeps [M, 3] plans and [pairs, 3] fp64 gathers in memory and its
              sums are not reproducible bit for bit (torch.sum's order is its own); the pair count must agree and the sums over coordinates to 1e-9 of it.
  walk        the same step on indexes of cell size 1, 2 and 4 times the search radius, the search radius unchanged: the 27 hash probes per query stay,
              the chains grow about 4-fold per doubling on surfaces.  Time that follows the chain length is the chain walk's; time that does not is the
              probes' (and the launch's).
  icp         align.icp end to end (wall time: every step ends in a 160-byte host read) with either step, from the identity
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scene_bench import alternate, event, make_scan, pair, stat, wall  # noqa: E402
from transfer_bench import rigid_pose  # noqa: E402

from point_sam_amd import align, ops, scene  # noqa: E402


def composed_step(index, xyz, pose=None, radius=None, bits=None):
    """ops.align_step's sums from the public ops of before it and torch; sums[19] is the query count (a plan does not say which query has a cell)."""
    idx3, _ = ops.transfer_plan(index, xyz, pose)
    j = idx3[:, 0].long()
    words = ops.transfer_pose(pose)
    p = xyz
    if words is not None:
        P = torch.from_numpy(words.reshape(3, 4)).to(xyz.device)
        p = xyz @ P[:, :3].T + P[:, 3]
    d = p - index.src_xyz[j.clamp_min(0)]
    q = (d * d).sum(1)
    ok = j >= 0
    if radius is not None:                                 # the nearest source within a smaller radius is the nearest one, if it is that close
        ok &= q <= ops.transfer_radius(radius)[2].item()
    if bits is not None:
        ok &= ops.mask_unpack(bits.reshape(1, -1), xyz.shape[0])[0]
    x, s = xyz[ok].double(), index.src_xyz[j[ok]].double()
    return torch.cat([ok.sum()[None].double(), q[ok].double().sum()[None], x.sum(0), s.sum(0), (x[:, :, None] * s[:, None, :]).sum(0).reshape(-1),
                      (x * x).sum()[None], (s * s).sum()[None], torch.full((1,), float(xyz.shape[0]), dtype=torch.float64, device=xyz.device)])


def measure(index, qry, pose, repeats):
    native, composed = ops.align_step(index, qry, pose), composed_step(index, qry, pose)
    # the same pairs, so the same exact terms in another order: the sums over coordinates (|term| <= 1) agree to 1e-9 of the pair count; sum q is
    # left out, the composed form computes its q in another fp32 arithmetic
    diff = float((native - composed)[2:19].abs().max())
    assert native[0] == composed[0] and diff <= 1e-9 * float(native[0]), (native.tolist(), composed.tolist())
    res = dict(queries=qry.shape[0], pairs=int(native[0]), with_cell=int(native[19]), max_abs_difference=diff)
    res["step"] = pair(*alternate(lambda: ops.align_step(index, qry, pose), lambda: composed_step(index, qry, pose), event, repeats))
    res["step_queries_per_us"] = round(qry.shape[0] / (res["step"]["native_ms"]["median"] * 1e3), 2)
    return res


def run(M, working, repeats):
    pose = rigid_pose()
    axyz, _ = make_scan(M, 5)
    bxyz, _ = make_scan(M, 6)
    bxyz = ((bxyz.double() - pose[:, 3].cuda()) @ pose[:, :3].cuda()).float().clamp_(-1, 1).contiguous()      # q = R^T (p - t)
    h = scene.choose_voxel_size(axyz, working)
    src = axyz.index_select(0, ops.voxel_downsample(axyz, h)[0]).contiguous()
    bwork = bxyz.index_select(0, ops.voxel_downsample(bxyz, scene.choose_voxel_size(bxyz, working))[0]).contiguous()
    radius = 2 * h
    index = ops.transfer_index(src, radius)
    res = dict(points=M, max_points=working, voxel_size=h, sources=src.shape[0], radius=radius, repeats=repeats,
               sources_per_occupied_cell=round(src.shape[0] / ops.voxel_count(src, radius, index.origin), 2))
    res["working"] = measure(index, bwork, pose, repeats)
    res["scan"] = measure(index, bxyz, pose, min(repeats, 10))
    res["walk"] = []
    for k in (1, 2, 4):
        coarse = ops.transfer_index(src, k * radius)
        times = [event(lambda: ops.align_step(coarse, bwork, pose, radius))[1] for _ in range(repeats + 2)][2:]
        res["walk"].append(dict(cell_over_radius=k, sources_per_occupied_cell=round(src.shape[0] / ops.voxel_count(src, k * radius, coarse.origin), 2),
                                step_ms=stat(times), pairs=int(ops.align_step(coarse, bwork, pose, radius)[0])))
    cfg = align.AlignConfig(radius, final_radius=radius / 2, shrink=0.8, iterations=30)
    for name, qry, n in (("working", bwork, min(repeats, 5)), ("scan", bxyz, 2)):
        out = align.icp(index, qry, cfg)
        c = align.icp(index, qry, cfg, step=composed_step)
        a, b = alternate(lambda: align.icp(index, qry, cfg), lambda: align.icp(index, qry, cfg, step=composed_step), wall, n)
        err = np.abs(out.pose - pose.numpy()).max()
        res[f"icp_{name}"] = dict(pair(a, b), iterations=out.iterations, converged=out.converged, reason=out.reason, pairs=out.pairs, rms=round(out.rms, 6),
                                  coverage=round(out.coverage, 4), max_abs_pose_error=float(err), composed_iterations=c.iterations,
                                  max_abs_pose_difference_to_composed=float(np.abs(out.pose - c.pose).max()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4194304")
    ap.add_argument("--working", type=int, default=131072)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = []
    for M in (int(m) for m in args.points.split(",")):
        res = run(M, args.working, args.repeats)
        print(json.dumps(res), flush=True)
        out.append(res)
        torch.cuda.empty_cache()
        if args.out:                                       # after every configuration: a run that is cut short keeps what it measured
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
