"""Times scan map normals and point-to-plane tracking (ops.map_normals, ops.track_plane_step, ScanMap.track(normals=True)) against what the map offered
before them: the composed normals (cloud() + voxel_downsample + region_neighbors + voxel_normals) and point-to-point tracking (track_step, track()).

    python scripts/track_plane_bench.py [--voxel-size 0.0078125] [--points 2000000] [--queries 131072] [--reps 50] [--warmup 10] [--out FILE]

The map and the scan are scripts/track_bench.py's: a synthetic room (about 2 * 10^5 voxels at the default size) and 131072 points of the same surfaces
under a small pose.  Medians and quartiles over --reps repetitions, the variants taken in turn inside every repetition so that drift hits them alike:

    normals        map_normals at reach 1 and 2 (device events and the host clock around a synchronise) against the composed form (host clock: it
                   reads the voxel count back)
    steps          per radius (h: reach 1, 2 h: reach 2) one track_plane_step on normals computed once, against one track_step
    loop           a whole track(normals=True), the normals included, against track() on the same scan, schedule and start

It checks that both steps pair the same queries (used + unused = the point-to-point pairs), and prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from track_bench import event_ms, host_ms, quartiles, room      # noqa: E402


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
        raise SystemExit("track_plane_bench: needs a GPU; a CPU run measures nothing")
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
              "device": torch.cuda.get_device_name(0), "normals": {}, "steps": {}}

    def composed():
        """What the parent offers: read the cloud out, voxelise it again, list the neighbours, solve."""
        cloud = m.cloud()[0].contiguous()
        keep, inv = ops.voxel_downsample(cloud, h)
        nbr = ops.region_neighbors(cloud, keep.contiguous(), h)
        return ops.voxel_normals(cloud, inv, nbr)

    variants = {"map_normals reach 1": lambda: m.normals(1), "map_normals reach 2": lambda: m.normals(2), "composed": composed}
    for _ in range(args.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {k: {"event": [], "host": []} for k in variants}
    for _ in range(args.reps):
        for k, fn in variants.items():
            if k != "composed":                                    # its host read sits inside: events would measure the same span as the host clock
                times[k]["event"].append(event_ms(fn))
            times[k]["host"].append(host_ms(fn)[0])
    result["normals"] = {k: {clock: quartiles(v) for clock, v in t.items() if v} for k, t in times.items()}
    mine, theirs = m.normals(1), composed()
    result["normals"]["with a normal"] = {"map_normals reach 1": int((mine.count >= 5).sum()), "map_normals reach 2": int((m.normals(2).count >= 5).sum()),
                                          "composed": int((theirs[0] >= 5).sum())}

    normal = mine.normal
    for name, radius in (("reach 1", h), ("reach 2", 2 * h)):
        variants = {"track_plane_step": lambda: m.track_plane_step(qry, normal, truth, radius), "track_step": lambda: m.track_step(qry, truth, radius)}
        for _ in range(args.warmup):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        times = {k: {"event": [], "host": []} for k in variants}
        for _ in range(args.reps):
            for k, fn in variants.items():
                times[k]["event"].append(event_ms(fn))
                times[k]["host"].append(host_ms(fn)[0])
        sums = {k: fn().cpu().numpy() for k, fn in variants.items()}
        assert sums["track_plane_step"][0] + sums["track_plane_step"][30] == sums["track_step"][0], "the two steps pair the same queries"
        result["steps"][name] = {"radius": radius, "used": int(sums["track_plane_step"][0]), "unused": int(sums["track_plane_step"][30]),
                                 "pairs": int(sums["track_step"][0]), **{k: {clock: quartiles(v) for clock, v in t.items()} for k, t in times.items()}}

    cfg = align.AlignConfig(radius=2 * h, final_radius=h, shrink=0.8, iterations=30)
    init = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    loops = {"track_plane": lambda: m.track(qry, cfg, init, normals=True), "track": lambda: m.track(qry, cfg, init)}
    for fn in loops.values():
        fn()
    times = {k: [] for k in loops}
    outs = {}
    for _ in range(max(5, args.reps // 5)):
        for k, fn in loops.items():
            t, outs[k] = host_ms(fn)
            times[k].append(t)
    result["loop"] = {k: dict(quartiles(v), iterations=outs[k].iterations, pairs=outs[k].pairs, converged=bool(outs[k].converged), reason=outs[k].reason,
                              rms=outs[k].rms, translation_error=float(np.linalg.norm(outs[k].pose[:, 3] - truth[:, 3])),
                              rotation_error=align._rotation_angle(outs[k].pose, truth)) for k, v in times.items()}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
