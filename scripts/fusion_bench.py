"""Times the label fusion (csrc/fusion.hip through point_sam_amd/fusion.py) next to the torch-composed form of the same definition.

    python scripts/fusion_bench.py [--frames 64] [--width 640] [--height 480] [--working 131072] [--world-points 8000000] [--repeats 10] [--torch-repeats 3] [--out FILE.json]
                                   [--readme FILE.md]

One process, one GPU.  The world is synthetic and the same for every frame: twelve sphere shells on a ring over a floor, --world-points points in all.
Every frame is a camera on a ring around it looking inwards; its depth image is the z-buffer of the world (ops.view_splat, footprint 1, holes are
depth 0), and its 2-D labels are the objects of its pixels' winning points, numbered 0 .. count - 1 in an order of the frame's own: the frames overlap
and see the objects from different sides.  The frames are fused into one scan by ops.frames_unproject / frames_finish.  The region rows and the links
are made on a voxel working cloud of at most --working points, the vote runs over the whole scan: predictor.fuse_labels' pipeline, called through
fusion.fuse.

The torch-composed form on the same inputs: per view a projection of every point (elementwise fp32 operators, the division IEEE), a gather of the
pixel's key and label, the visibility compare, one comparison per region for the rows, and for the vote a `scatter_add` histogram over the instances
(thirteen objects here; the two agree wherever the 8-slot table dropped nothing, and the script refuses to time anything if it dropped something).
Its rows, seen / labelled counts, labels and votes are compared with ours first and must be equal; the two are then timed ALTERNATING on the same
inputs, device-event times, median with min and max after two warm-up rounds.  The linking (one [R + V]^2 intersection matrix, a handful of torch operators, the edge list read by the host) is common to both.
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

from scene_bench import alternate, event, pair, stat  # noqa: E402

from point_sam_amd import fusion, ops, scene  # noqa: E402
from point_sam_amd.views import Camera, View  # noqa: E402

SPHERES = 12


def make_world(points, seed):
    """-> (world [P, 3] f32, obj [P] int64 in 0 .. SPHERES) on the device: SPHERES shells of radius 0.12 on a ring of radius 0.6, and a floor."""
    g = torch.Generator().manual_seed(seed)
    per = points // (2 * SPHERES)
    parts, obj = [], []
    for o in range(SPHERES):
        a = 2 * math.pi * o / SPHERES
        d = torch.randn(per, 3, generator=g)
        parts.append(0.12 * d / d.norm(dim=1, keepdim=True) + torch.tensor([0.6 * math.sin(a), 0.15, 0.6 * math.cos(a)]))
        obj.append(torch.full((per,), o))
    n = points - per * SPHERES
    fl = torch.rand(n, 2, generator=g) * 2 - 1
    parts.append(torch.stack([fl[:, 0], torch.full((n,), 0.3), fl[:, 1]], 1))
    obj.append(torch.full((n,), SPHERES))
    return torch.cat(parts).float().cuda().contiguous(), torch.cat(obj).cuda()


def make_frames(world, obj, F, H, W):
    """-> (depth [F, H, W] f32 with 0 where nothing is seen, the object per pixel [F, H, W] int64 or -1, cameras, far)."""
    cams, depth, pix = [], [], []
    for f in range(F):
        a = 2 * math.pi * f / F
        cam = Camera.look_at((2.6 * math.sin(a), -1.2, 2.6 * math.cos(a)), (0, 0, 0), (0, -1, 0), 40.0, W, H, near=0.05)
        view = View(ops.view_splat(world, cam, 1), cam, world.shape[0], 1)
        empty = view.keys == -1
        depth.append(torch.where(empty, torch.zeros_like(view.depth), view.depth))
        pix.append(torch.where(empty, torch.full_like(view.keys, -1), obj[view.index.clamp_min(0).long()]))
        cams.append(cam)
    return torch.stack(depth).contiguous(), torch.stack(pix), cams, 10.0


def make_labels(pix, seed):
    """pix [F, H, W] int64, the object of every pixel or -1 -> (labels [F, H, W] int32, row_base [F + 1] numpy): frame f numbers the objects it sees
    0 .. count - 1 in the order of a seeded permutation."""
    g = torch.Generator().manual_seed(seed)
    labels = torch.full(pix.shape, -1, dtype=torch.int32, device=pix.device)
    counts = []
    for f in range(pix.shape[0]):
        present = torch.unique(pix[f][pix[f] >= 0]).cpu()
        order = present[torch.randperm(present.numel(), generator=g)]
        table = torch.full((SPHERES + 1,), -1, dtype=torch.int32)
        table[order] = torch.arange(order.numel(), dtype=torch.int32)
        labels[f] = torch.where(pix[f] >= 0, table.to(pix.device)[pix[f].clamp_min(0)], torch.full_like(labels[f], -1))
        counts.append(int(order.numel()))
    return labels.contiguous(), np.concatenate([[0], np.cumsum(counts)])


def observe(xyz, cam, keys, labels, tau):
    """One view in torch operators -> (visible [N] bool, label [N] int32).  cam: the 17 camera words as 0-dim device tensors."""
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    a, b, c = (((cam[4 * r] * x + cam[4 * r + 1] * y) + cam[4 * r + 2] * z) + cam[4 * r + 3] for r in range(3))
    u = cam[12] * (a / c) + cam[14]
    v = cam[13] * (b / c) + cam[15]
    H, W = keys.shape
    ok = (c >= cam[16]) & torch.isfinite(c) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    p = torch.where(ok, v.floor().long() * W + u.floor().long(), torch.zeros_like(ok, dtype=torch.int64))
    k = keys.reshape(-1)[p]
    front = (k >> 32).to(torch.int32).view(torch.float32)
    vis = ok & (k != -1) & (c <= front + tau)
    return vis, labels.reshape(-1)[p]


def torch_rows(xyz, table, keys, labels, rb, tau):
    """-> rows [R + V, N] bool."""
    V, R = keys.shape[0], int(rb[-1])
    rows = torch.zeros(R + V, xyz.shape[0], dtype=torch.bool, device=xyz.device)
    for v in range(V):
        vis, lab = observe(xyz, table[v], keys[v], labels[v], tau)
        for l in range(int(rb[v + 1] - rb[v])):
            rows[int(rb[v]) + l] = vis & (lab == l)
        rows[R + v] = vis
    return rows


def torch_vote(xyz, table, keys, labels, rb, remap, G, tau):
    """-> (label, votes, seen, labelled) by a scatter_add histogram over the G instances."""
    N, dev = xyz.shape[0], xyz.device
    hist = torch.zeros(N, G, dtype=torch.int32, device=dev)
    seen = torch.zeros(N, dtype=torch.int32, device=dev)
    labelled = torch.zeros(N, dtype=torch.int32, device=dev)
    for v in range(keys.shape[0]):
        vis, lab = observe(xyz, table[v], keys[v], labels[v], tau)
        count = int(rb[v + 1] - rb[v])
        valid = vis & (lab >= 0) & (lab < count)
        g = remap[(int(rb[v]) + lab.clamp(0, max(count - 1, 0))).long()] if count else torch.full_like(lab, -1)
        valid = valid & (g >= 0)
        hist.scatter_add_(1, g.clamp_min(0).long()[:, None], valid.to(torch.int32)[:, None])
        seen += vis
        labelled += valid
    score = hist.long() * (G + 1) + (G - 1 - torch.arange(G, device=dev))          # the highest count, ties to the lower label
    best = score.argmax(1)
    votes = hist.gather(1, best[:, None])[:, 0]
    return torch.where(votes > 0, best.to(torch.int32), torch.full_like(votes, -1)), votes, seen, labelled


def run(args):
    points, obj = make_world(args.world_points, 11)
    depth, pix, cams, far = make_frames(points, obj, args.frames, args.height, args.width)
    rgb = torch.zeros(depth.shape + (3,), dtype=torch.uint8, device="cuda")
    world, col, index, M = ops.frames_unproject(depth, rgb, cams, far, 0.05)
    center = world.double().mean(0).float()
    scale = ((world.double() - center.double()) ** 2).sum(1).max().sqrt().float()
    xyz, keys, ncams = ops.frames_finish(world, index, cams, center.cpu().numpy(), float(scale))
    del depth, rgb, col, world, points, obj
    labels, rb = make_labels(pix, 5)
    del pix
    h = scene.choose_voxel_size(xyz, args.working)
    keep_idx, _ = ops.voxel_downsample(xyz, h)
    link_xyz = xyz.index_select(0, keep_idx).contiguous()
    cfg = fusion.FusionConfig(tau=0.01)
    V, R, Nw = keys.shape[0], int(rb[-1]), link_xyz.shape[0]

    fused = fusion.fuse(xyz, link_xyz, ncams, keys, labels, cfg)
    G = fused.num_instances
    table = torch.tensor([[float(w) for w in c.pose_words] + [c.fx, c.fy, c.cx, c.cy, c.near] for c in ncams], dtype=torch.float32).cuda()
    bits, _ = ops.fuse_region_bits(link_xyz, ncams, keys, labels, rb, cfg.tau)
    rows = torch_rows(link_xyz, table, keys, labels, rb, cfg.tau)
    t_label, t_votes, t_seen, t_labelled = torch_vote(xyz, table, keys, labels, rb, fused.remap, G, cfg.tau)
    equal = dict(rows=bool(torch.equal(ops.mask_unpack(bits, Nw), rows)), label=bool(torch.equal(t_label, fused.labels)),
                 votes=bool(torch.equal(t_votes, fused.votes)), seen=bool(torch.equal(t_seen, fused.seen)),
                 labelled=bool(torch.equal(t_labelled, fused.labelled)), dropped_none=int(fused.dropped.max()) == 0)
    print(json.dumps(dict(scan_points=M, working_points=Nw, regions=R, instances=G, equal=equal)), flush=True)
    assert all(equal.values()), f"native and torch-composed fusion disagree: {equal}"
    del rows, t_label, t_votes, t_seen, t_labelled
    torch.cuda.empty_cache()

    res = dict(frames=V, height=args.height, width=args.width, scan_points=M, working_points=Nw, voxel_size=h, regions=R, instances=G, tau=cfg.tau, equal=equal,
               max_seen=int(fused.seen.max()), mean_seen=round(float(fused.seen.float().mean()), 2))
    timed = lambda fn: stat([event(fn)[1] for _ in range(args.repeats + 2)][2:])
    res["region_bits_ms"] = timed(lambda: ops.fuse_region_bits(link_xyz, ncams, keys, labels, rb, cfg.tau))
    res["link_ms"] = timed(lambda: fusion.link_regions(ops.mask_intersections(bits, bits), rb, cfg))
    res["vote_ms"] = timed(lambda: ops.fuse_vote(xyz, ncams, keys, labels, cfg.tau, rb, fused.remap, cfg.min_votes))
    res["label_bits_ms"] = timed(lambda: ops.label_bits(fused.labels, G))
    res["fuse_ms"] = timed(lambda: fusion.fuse(xyz, link_xyz, ncams, keys, labels, cfg))
    # what the vote must touch at least: a point's coordinates in, five words out, and per observation a key and a label at pixel granularity
    res["vote_bytes"] = M * (12 + 20) + M * V * 12
    res["vote_gathers_per_s"] = round(M * V / (res["vote_ms"]["median"] * 1e-3), 0)
    res["rows_alternating"] = pair(*alternate(lambda: ops.fuse_region_bits(link_xyz, ncams, keys, labels, rb, cfg.tau),
                                              lambda: torch_rows(link_xyz, table, keys, labels, rb, cfg.tau), event, args.torch_repeats))
    res["vote_alternating"] = pair(*alternate(lambda: ops.fuse_vote(xyz, ncams, keys, labels, cfg.tau, rb, fused.remap, cfg.min_votes),
                                              lambda: torch_vote(xyz, table, keys, labels, rb, fused.remap, G, cfg.tau), event, args.torch_repeats))
    return res


def readme(r, args):
    ms = lambda s: f"{s['median']:.3f} [{s['min']:.3f} … {s['max']:.3f}]"
    alt = lambda a: f"{a['native_ms']['median']:.3f} / {a['torch_ms']['median']:.3f} ({a['torch_over_native']:.1f} ×)"
    lines = ["# profiles/fusion — multi-view label fusion", "",
             f"`python scripts/fusion_bench.py --frames {args.frames} --width {args.width} --height {args.height} --working {args.working} --repeats {args.repeats} "
             f"--torch-repeats {args.torch_repeats}`: one MI355X (gfx950), one process, torch {torch.__version__}.  Device-event times in ms, "
             "`median [min … max]` after two warm-up rounds; the alternating rows time the two forms in turn on the same inputs, the order swapped every "
             "round.  Every number in the table is measured by this one run of the script.  The torch-composed form (scripts/fusion_bench.py: per view a "
             "projection, a gather, a compare per region, a `scatter_add` histogram) gave **the same** rows, labels, votes, seen and labelled counts before "
             "anything was timed.  These are records, not gates.", "",
             "| | |", "|---|---|",
             f"| frames × height × width | {r['frames']} × {r['height']} × {r['width']} |",
             f"| scan points / working-cloud points (voxel {r['voxel_size']:.4g}) | {r['scan_points']} / {r['working_points']} |",
             f"| (view, region) rows R / instances | {r['regions']} / {r['instances']} |",
             f"| views that see a point: mean / max | {r['mean_seen']} / {r['max_seen']} |",
             f"| `ops.fuse_region_bits` on the working cloud (clear, rows, areas: three launches) | {ms(r['region_bits_ms'])} |",
             f"| `ops.mask_intersections` + `fusion.link_regions` (one host read) | {ms(r['link_ms'])} |",
             f"| `ops.fuse_vote` on the scan (one launch) | {ms(r['vote_ms'])} |",
             f"| `ops.label_bits` of the result | {ms(r['label_bits_ms'])} |",
             f"| `fusion.fuse`, everything with its host work | {ms(r['fuse_ms'])} |",
             f"| point × view projections per second in the vote | {r['vote_gathers_per_s'] / 1e9:.1f} G/s |",
             f"| rows, alternating: native / torch-composed | {alt(r['rows_alternating'])} |",
             f"| vote, alternating: native / torch-composed | {alt(r['vote_alternating'])} |", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--working", type=int, default=131072)
    ap.add_argument("--world-points", type=int, default=8000000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--torch-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--readme", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fusion_bench: needs a GPU (a timing taken elsewhere says nothing)")
    res = run(args)
    print(json.dumps(res), flush=True)
    for path, text in ((args.out, json.dumps(res, indent=1)), (args.readme, readme(res, args))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
