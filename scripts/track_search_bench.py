"""Times the relocalisation of a scan in a scan map (ScanMap.track_score, ScanMap.relocalize) against the forms a caller had before it.

    python scripts/track_search_bench.py [--voxel-size 0.0078125] [--points 3000000] [--repeats 7] [--json out.json]

Everything is generated from a seed; nothing outside the repository is read.  The map is a synthetic room (the six walls of a box, three boxes of
furniture and a sphere) sampled with --points points and added once; the scan is the part of another sampling of the same room inside a ball, given
in a frame a quarter turn and a shift away.  Timed, per reach (the scoring radius is reach x the voxel size) and per number of poses, on the 1024
sampled queries align.search would score:

    score       one ScanMap.track_score over the whole grid (the clear, the means table and the score kernel)
    steps       the form the code had before: one ScanMap.track_step per pose on the same sample.  Timed on the first --step-poses poses only and
                scaled to the grid; the scaling is stated in the output
    readout     the read-out form: ScanMap.cloud(), ops.transfer_index on it at the scoring radius, ops.align_score -- the index build counted
    table       track_score with ONE pose and ONE query: the clear, the means table and a one-wave score launch -- what every call pays before it
                scores anything
    search      the whole ScanMap.relocalize: host clock, it ends in host reads

Device events around each form, every form warmed up first, the forms alternated inside each repeat, median and range over the repeats.  The counts
of `score` are compared with `steps` (on the poses both ran) before anything is timed; `readout` answers another question (it ignores min_count and
occupied, and its candidates are the 27 cells of an index at the radius) and is not compared.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from point_sam_amd import ops                                      # noqa: E402
from point_sam_amd.align import AlignConfig, SearchConfig, candidate_poses, sample_positions      # noqa: E402
from point_sam_amd.scanmap import ScanMap                          # noqa: E402


def room(n: int, seed: int) -> torch.Tensor:
    """n points on the walls of [-0.9, 0.9]^3, on three boxes and on a sphere, on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = torch.rand(n, 3, generator=g, device="cuda")
    which = torch.randint(0, 10, (n,), generator=g, device="cuda")
    pts = torch.empty(n, 3, device="cuda")
    boxes = [((-0.9, -0.9, -0.9), (0.9, 0.9, 0.9))] * 6 + [((-0.7, -0.6, -0.9), (-0.2, 0.1, -0.3)), ((0.1, 0.3, -0.9), (0.8, 0.7, -0.5)),
                                                          ((0.3, -0.8, -0.9), (0.6, -0.3, 0.2))]
    for k, (lo, hi) in enumerate(boxes):
        lo, hi = torch.tensor(lo, device="cuda"), torch.tensor(hi, device="cuda")
        m = which == k
        p = lo + (hi - lo) * u[m]
        face = k % 6 if k < 6 else None
        if face is None:                                           # a random face of a furniture box
            f = torch.randint(0, 6, (int(m.sum()),), generator=g, device="cuda")
        else:
            f = torch.full((int(m.sum()),), face, device="cuda")
        for axis in range(3):
            p[:, axis] = torch.where(f == 2 * axis, lo[axis].expand_as(p[:, axis]), p[:, axis])
            p[:, axis] = torch.where(f == 2 * axis + 1, hi[axis].expand_as(p[:, axis]), p[:, axis])
        pts[m] = p
    m = which == 9
    d = torch.randn(int(m.sum()), 3, generator=g, device="cuda")
    pts[m] = torch.tensor([-0.3, 0.5, 0.1], device="cuda") + 0.25 * d / d.norm(dim=1, keepdim=True)
    return pts.contiguous()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    ms = sorted(ms)
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1], repeats=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel-size", type=float, default=2.0 ** -7)
    ap.add_argument("--points", type=int, default=3_000_000)
    ap.add_argument("--scan-points", type=int, default=400_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--step-poses", type=int, default=256)
    ap.add_argument("--reaches", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("track_search_bench needs a GPU: there is nothing to time without one")
    h = args.voxel_size
    m = ScanMap(h, 1 << 21)
    pts = room(args.points, 1)
    m.add(pts, torch.zeros_like(pts))
    V = m.num_voxels
    # the scan: another sampling, the part within 0.6 of a point of the room, in a frame 90 degrees about z and a shift away
    truth = np.array([[0.0, -1.0, 0.0, 0.12], [1.0, 0.0, 0.0, -0.07], [0.0, 0.0, 1.0, 0.03]])
    other = room(args.scan_points, 2)
    other = other[(other - torch.tensor([0.2, 0.1, -0.5], device="cuda")).norm(dim=1) < 0.6]
    Rm, t = torch.tensor(truth[:, :3], device="cuda", dtype=torch.float64), torch.tensor(truth[:, 3], device="cuda", dtype=torch.float64)
    scan = ((other.double() - t) @ Rm).float().contiguous()        # q = R^T (p - t)
    M = scan.shape[0]
    pick = torch.from_numpy(sample_positions(M, 1024)).cuda()
    sample = scan.index_select(0, pick).contiguous()
    qc = sample.double().mean(0).cpu().numpy()
    sc = m.cloud()[0].double().mean(0).cpu().numpy()
    anchors = m.anchors(cells=32, min_voxels=64)                   # coarse cells a quarter of a unit wide
    grids = {"72 yaw x 27 offsets": SearchConfig(yaw_steps=72, offsets=1, offset_step=4 * h),
             "72 yaw x 125 offsets": SearchConfig(yaw_steps=72, offsets=2, offset_step=4 * h),
             f"72 yaw x {min(len(anchors), 50)} anchors x 27 offsets": SearchConfig(yaw_steps=72, offsets=1, offset_step=4 * h, anchors=anchors[:50])}
    out = dict(device=torch.cuda.get_device_name(0), voxel_size=h, map_voxels=V, map_points=args.points, scan_points=M, sample=int(sample.shape[0]),
               anchors=int(len(anchors)), rows=[])
    print(json.dumps({k: v for k, v in out.items() if k != "rows"}), flush=True)
    for reach in args.reaches:
        radius = reach * h
        for name, cfg in grids.items():
            poses = candidate_poses(cfg, sc, qc)
            words = torch.from_numpy(ops.transfer_poses(poses)).cuda()
            P = words.shape[0]
            S = min(P, args.step_poses)
            forms = {
                "score": lambda: m.track_score(sample, words, radius),
                "steps": lambda: [m.track_step(sample, poses[p], radius) for p in range(S)],
                "readout": lambda: ops.align_score(ops.transfer_index(m.cloud()[0], radius), sample, words, radius),
                "table": lambda: m.track_score(sample[:1], words[:1], radius),
            }
            counts = forms["score"]()                              # warm-up, and the check
            pairs = [int(s[0]) for s in forms["steps"]()]
            assert counts[:S].tolist() == pairs, "track_score and track_step disagree"
            forms["readout"](), forms["table"]()
            torch.cuda.synchronize()
            ms = {k: [] for k in forms}
            for _ in range(args.repeats):
                for k, fn in forms.items():                        # alternated inside a repeat
                    ms[k].append(timed(fn))
            row = dict(reach=reach, grid=name, poses=P, best_count=int(counts.max()), median_count=int(counts.median()), step_poses=S,
                       **{k: stats(v) for k, v in ms.items()})
            row["steps_scaled_to_grid_ms"] = row["steps"]["median_ms"] * P / S
            out["rows"].append(row)
            print(json.dumps(row), flush=True)
    # the whole search: 10-degree yaw steps x every anchor of the map x a lattice that spans an anchor's coarse cell, scored and refined at 4 voxels
    icp = AlignConfig(radius=4 * h, final_radius=h, shrink=0.8, iterations=40)
    search = SearchConfig(yaw_steps=36, offsets=2, offset_step=8 * h, anchors=anchors[:(1 << 20) // (36 * 125)], sample=1024, radius=4 * h, keep=8)
    found = m.relocalize(scan, icp, search)                        # warm-up
    rot = math.acos(min(1.0, max(-1.0, (np.trace(found.pose[:, :3].T @ truth[:, :3]) - 1.0) / 2.0)))
    walls = []
    for _ in range(max(3, args.repeats // 2)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.relocalize(scan, icp, search)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    out["search"] = dict(poses=found.search.poses, sample=found.search.sample, keep=search.keep, pairs=found.pairs, scan_points=M,
                         rotation_error_rad=rot, translation_error=float(np.linalg.norm(found.pose[:, 3] - truth[:, 3])), converged=found.converged,
                         steps_of_the_winner=found.iterations, **stats(walls))
    print(json.dumps(out["search"]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
