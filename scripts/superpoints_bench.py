"""Times point normals, superpoints and mask snapping (point_sam_amd/superpoints.py, csrc/normals.hip, csrc/superpoints.hip) stage by stage.

    python scripts/superpoints_bench.py [--points 1000000] [--rows 64] [--repeats 5] [--out FILE.json]

One process, one GPU, no model: a synthetic room -- a floor, two walls, a box and a ball on the floor, sampled with a little noise.  By device
events: the graph build (it synchronises with the host, so wall time is given too); the normals (moments + eigen), and the same call with
min_points above every count, which accumulates and sums the moments but solves nothing -- the difference is the eigen-solve; union, absorb and
compaction; the snap of `--rows` ball masks.  Next to them a torch composition of the same steps: fp64 moments by index_add_ and a gather over the
26 neighbours, torch.linalg.eigh, and a union-find on the host over the edges the join rule passes (copies to the host included).  Before anything
is timed the device's scatter matrices must be the composition's to fp64 accumulation error and its labels must be the host reference's partition.
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
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

from point_sam_amd import ops, regions, superpoints  # noqa: E402


def timed(fn, repeats):
    """-> (result, [ms per repeat]) by device events, after one warm-up call."""
    out = fn()
    ms = []
    for _ in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    return out, ms


def stat(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def room(N, seed):
    """Floor z = -0.8, walls x = -0.8 and y = -0.8, a box and a ball standing on the floor; sigma = 0.001."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = torch.rand(N, 3, generator=g, device="cuda")
    part = torch.randint(0, 10, (N,), generator=g, device="cuda")
    p = u * 1.6 - 0.8
    for axis, ids in ((2, (0, 1, 2)), (0, (3, 4)), (1, (5, 6))):
        m = (part.unsqueeze(1) == torch.tensor(ids, device="cuda")).any(1)
        p[m, axis] = -0.8
    box = part == 7                                               # the faces of a cube of side 0.5: one coordinate pinned to a face
    face = torch.randint(0, 3, (N,), generator=g, device="cuda")
    side = torch.randint(0, 2, (N,), generator=g, device="cuda").float()
    q = u * 0.5 + torch.tensor([0.0, 0.0, -0.8], device="cuda")
    q[torch.arange(N, device="cuda"), face] = (side * 0.5 + torch.tensor([0.0, 0.0, -0.8], device="cuda")[face])
    p[box] = q[box]
    ball = part >= 8
    d = torch.randn(N, 3, generator=g, device="cuda")
    p[ball] = (0.3 * d / d.norm(dim=1, keepdim=True) + torch.tensor([-0.4, -0.3, -0.5], device="cuda"))[ball]
    p = p + torch.randn(N, 3, generator=g, device="cuda") * 0.001
    return p.clamp_(-1, 1).contiguous()


def torch_moments(xyz, graph):
    """The composition: fp64 sums per voxel by index_add_, the neighbourhood by a gather, S = n P - s s^T in fp64 (about the voxel's own anchor, or
    fp64 would cancel), eigh."""
    V = graph.keep_idx.numel()
    q = torch.floor(xyz.double() * 2.0 ** 20) + 2.0 ** 20
    q = q - q[graph.keep_idx].mean(0)                             # one anchor for all: S is invariant, fp64 keeps more of it
    feats = torch.cat([torch.ones_like(q[:, :1]), q, q[:, [0, 0, 0, 1, 1, 2]] * q[:, [0, 1, 2, 1, 2, 2]]], 1)
    own = torch.zeros(V, 10, dtype=torch.float64, device=xyz.device).index_add_(0, graph.inv, feats)
    nb = graph.nbr.long()
    tot = own + (own[nb.clamp(min=0)] * (nb >= 0).unsqueeze(-1)).sum(1)
    n, s, P = tot[:, :1], tot[:, 1:4], tot[:, 4:]
    return n[:, 0], n * P - s[:, [0, 0, 0, 1, 1, 2]] * s[:, [0, 1, 2, 1, 2, 2]]


def torch_eigen(S):
    M = S[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)
    w, e = torch.linalg.eigh(M)
    return e[:, :, 0].float(), (w[:, 0].clamp(min=0) / w.sum(1).clamp(min=1e-300)).float()


def main():
    import superpoint_reference as SP
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, K, cfg = args.points, args.rows, superpoints.SuperpointConfig()
    xyz = room(N, 3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    graph, build_ms = timed(lambda: regions.build_graph(xyz, cfg.voxel_size, cfg.points_per_voxel), args.repeats)
    build_wall = (time.perf_counter() - t0) * 1e3 / (args.repeats + 1)
    V = graph.keep_idx.numel()

    (count, normal, curv, S), normals_ms = timed(lambda: ops.voxel_normals(xyz, graph.inv, graph.nbr, cfg.min_points, scatter=True), args.repeats)
    _, moments_ms = timed(lambda: ops.voxel_normals(xyz, graph.inv, graph.nbr, 2 ** 31 - 1), args.repeats)
    labels_fn = lambda: ops.superpoint_labels(graph.inv, graph.nbr, count, normal, curv, cfg.cos_angle, cfg.max_curvature, cfg.min_points, cfg.min_size,
                                              cfg.absorb_rounds)
    (vl, pl, size, num), labels_ms = timed(labels_fn, args.repeats)
    _, union_ms = timed(lambda: ops.superpoint_labels(graph.inv, graph.nbr, count, normal, curv, cfg.cos_angle, cfg.max_curvature, cfg.min_points,
                                                      cfg.min_size, 0), args.repeats)
    num_sp = int(num.item())
    sp = superpoints.Superpoints(pl, vl, size[:num_sp].contiguous(), num_sp, None)
    g = torch.Generator(device="cuda").manual_seed(5)
    centres = xyz[torch.randint(0, N, (K,), generator=g, device="cuda")]
    r = torch.rand(K, 1, generator=g, device="cuda") * 0.3 + 0.1
    bits, _, _, _ = ops.mask_pack((r - torch.cdist(centres, xyz)).contiguous(), 0.0, 0.0)
    (sb, sa, sc), snap_ms = timed(lambda: superpoints.snap_bits(sp, bits), args.repeats)

    # ---- the torch composition, checked against the device first
    (tn, tS), tmom_ms = timed(lambda: torch_moments(xyz, graph), args.repeats)
    assert torch.equal(tn.int(), count)
    scale = S.abs().amax(1, keepdim=True).clamp(min=1)
    moment_gap = float(((tS - S).abs() / scale).max())
    assert moment_gap < 1e-6, moment_gap                          # the composition accumulates in fp64; the device's S is exact
    (tnorm, tcurv), teig_ms = timed(lambda: torch_eigen(S), args.repeats)
    valid = count >= cfg.min_points
    curv_gap = float((tcurv[valid] - curv[valid]).abs().max())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = SP.superpoints(graph.inv.cpu().numpy(), graph.nbr.cpu().numpy(), count.cpu().numpy(), normal.cpu().numpy(), curv.cpu().numpy(), cfg.cos_angle,
                          cfg.max_curvature, cfg.min_points, cfg.min_size, cfg.absorb_rounds)
    host_ms = (time.perf_counter() - t0) * 1e3
    assert want[3] == num_sp and np.array_equal(want[1], pl.cpu().numpy()), "device and host superpoints differ"

    res = dict(points=N, voxels=V, voxel_size=graph.voxel_size, superpoints=num_sp, largest=int(size[:num_sp].max()), rows=K,
               rows_changed=int(sc.sum()), checks=dict(torch_moments_relative_gap=moment_gap, torch_curvature_gap=curv_gap),
               device_ms=dict(graph_build=stat(build_ms), graph_build_wall=round(build_wall, 3), normals=stat(normals_ms),
                              normals_without_eigen_solve=stat(moments_ms), union_absorb_compact=stat(labels_ms), union_compact_only=stat(union_ms),
                              snap=stat(snap_ms)),
               torch_ms=dict(moments_index_add=stat(tmom_ms), eigh=stat(teig_ms), host_union_find_absorb=round(host_ms, 1)))
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
