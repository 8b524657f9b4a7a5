"""Times scan map tracking (ops.track_step, ScanMap.track) against the composed form it replaces: ops.align_step on a transfer index of the map's cloud.

    python scripts/track_bench.py [--voxel-size 0.0078125] [--points 2000000] [--queries 131072] [--reps 50] [--warmup 10] [--out FILE]

The map is a synthetic room (four walls' worth of planes and a sphere, about 2 * 10^5 voxels at the default size), the scan 131072 points of the same
surfaces under a small pose.  Per radius (h: reach 1, 2 h: reach 2) it reports the median and the quartiles over --reps repetitions, the variants
taken in turn inside every repetition so that drift hits them alike:

    track_step           one ScanMap.track_step                                             device events, and the host clock around a synchronise
    align_step           one ops.align_step on a PREBUILT transfer_index(cloud, radius)     the same two clocks
    composed             cloud() + transfer_index (one host read) + align_step: what a scan costs without tracking, since the map changed since the
                         last scan                                                          host clock
    track / icp          a whole ScanMap.track against align.icp on a prebuilt index, and against the index build + icp     host clock

It also checks that both steps pair the same number of queries to within the few that the two cell grids treat differently, and prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def room(n, seed):
    """n points on a floor, two walls, a table top and a sphere inside [-0.9, 0.9]^3."""
    g = np.random.default_rng(seed)
    which = g.integers(0, 5, size=n)
    u, v = g.uniform(-0.9, 0.9, size=n), g.uniform(-0.9, 0.9, size=n)
    pts = np.empty((n, 3))
    for k, (axis, at) in enumerate(((2, -0.85), (0, -0.88), (1, 0.87), (2, -0.2))):
        m = which == k
        pts[m] = np.insert(np.stack([u[m], v[m]], 1), axis, at, axis=1)
    m = which == 4
    d = g.normal(size=(int(m.sum()), 3))
    pts[m] = np.array([0.2, -0.1, 0.3]) + 0.45 * d / np.linalg.norm(d, axis=1, keepdims=True)
    return pts.astype(np.float32)


def quartiles(xs):
    q = statistics.quantiles(xs, n=4)
    return {"median_ms": round(statistics.median(xs), 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4)}


def host_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel-size", type=float, default=2.0 ** -7)
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--queries", type=int, default=131072)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("track_bench: needs a GPU; a CPU run measures nothing")
    from point_sam_amd import align, ops
    from point_sam_amd.scanmap import ScanMap
    h = args.voxel_size
    m = ScanMap(h, 1 << 19)
    pts = torch.from_numpy(room(args.points, 1)).cuda()
    m.add(pts, torch.zeros_like(pts))
    th = np.deg2rad(0.3)
    truth = np.array([[np.cos(th), -np.sin(th), 0, h / 3], [np.sin(th), np.cos(th), 0, -h / 4], [0, 0, 1, h / 5]])
    q = room(args.queries, 2).astype(np.float64)
    qry = torch.from_numpy(((q - truth[:, 3]) @ truth[:, :3]).astype(np.float32)).cuda()      # truth leads the scan back onto the map
    result = {"voxel_size": h, "voxels": m.num_voxels, "queries": args.queries, "reps": args.reps, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "steps": {}}
    for name, radius in (("reach 1", h), ("reach 2", 2 * h)):
        index = ops.transfer_index(m.cloud()[0].contiguous(), radius)
        variants = {"track_step": lambda: m.track_step(qry, truth, radius), "align_step": lambda: ops.align_step(index, qry, truth, radius),
                    "composed": lambda: ops.align_step(ops.transfer_index(m.cloud()[0].contiguous(), radius), qry, truth, radius)}
        for _ in range(args.warmup):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        times = {k: {"event": [], "host": []} for k in variants}
        for _ in range(args.reps):
            for k, fn in variants.items():
                if k != "composed":                                # its host read sits inside: events would measure the same span as the host clock
                    times[k]["event"].append(event_ms(fn))
                times[k]["host"].append(host_ms(fn)[0])
        sums = {k: fn().cpu().numpy() for k, fn in variants.items()}
        result["steps"][name] = {"radius": radius, "pairs": {k: int(s[0]) for k, s in sums.items()},
                                 **{k: {clock: quartiles(v) for clock, v in t.items() if v} for k, t in times.items()}}
    cfg = align.AlignConfig(radius=2 * h, final_radius=h, shrink=0.8, iterations=30)
    init = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    index = ops.transfer_index(m.cloud()[0].contiguous(), cfg.radius)
    loops = {"track": lambda: m.track(qry, cfg, init), "icp_prebuilt_index": lambda: align.icp(index, qry, cfg, init),
             "icp_with_index_build": lambda: align.icp(ops.transfer_index(m.cloud()[0].contiguous(), cfg.radius), qry, cfg, init)}
    for fn in loops.values():
        fn()
    times = {k: [] for k in loops}
    outs = {}
    for _ in range(max(5, args.reps // 5)):
        for k, fn in loops.items():
            t, outs[k] = host_ms(fn)
            times[k].append(t)
    result["loop"] = {k: dict(quartiles(v), iterations=outs[k].iterations, pairs=outs[k].pairs, converged=bool(outs[k].converged), rms=outs[k].rms,
                              translation_error=float(np.linalg.norm(outs[k].pose[:, 3] - truth[:, 3]))) for k, v in times.items()}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
