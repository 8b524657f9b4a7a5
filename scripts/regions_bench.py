"""Times the connected-component clean-up of masks (point_sam_amd/regions.py, csrc/regions.hip) stage by stage.

    python scripts/regions_bench.py [--cases proposals,scene] [--repeats 5] [--host-rows 16] [--out FILE.json]

One process, one GPU, no model: the masks are noisy balls on a uniform cloud (logit = 8 (r - distance to a centre) + noise, thresholded at 0), which
have a ragged rim of islands and pin-holes like thresholded decoder logits.  `proposals` = K 3072 candidates on N 32768 points (the small case of
scripts/proposals_bench.py); `scene` = K 768 on a working cloud of 131072 points (what set_scene(max_points=131072) leaves of a larger scan).
Per case, by device events: the graph build (voxel-size bisection, downsample, neighbour table; it synchronises with the host, so wall time is
given too), the labels of all rows, the clean-up of all rows (holes + islands at `--min-points`), and for scale the rest of the proposal
post-processing on the same rows (intersections, sort + validity + suppression, paint) and the host composition of the same clean-up with
scipy.sparse.csgraph on `--host-rows` rows (copy to the host included), scaled to K rows.  Before anything is timed the device clean-up of those rows
must equal the host's.
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

from point_sam_amd import ops, regions  # noqa: E402

CASES = {"proposals": dict(points=32768, rows=3072), "scene": dict(points=131072, rows=768)}


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


def blobs(N, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    xyz = (torch.rand(N, 3, generator=g, device="cuda") * 2 - 1).contiguous()
    centres = xyz[torch.randint(0, N, (K,), generator=g, device="cuda")]
    r = torch.rand(K, 1, generator=g, device="cuda") * 0.45 + 0.15
    bits = torch.empty(K, ops.mask_words(N), dtype=torch.int64, device="cuda")
    areas = tuple(torch.empty(K, dtype=torch.int32, device="cuda") for _ in range(3))
    for k0 in range(0, K, 256):                           # the logits of 256 rows at a time: never K * N floats
        k1 = min(K, k0 + 256)
        logits = (r[k0:k1] - torch.cdist(centres[k0:k1], xyz)) * 8 + torch.randn(k1 - k0, N, generator=g, device="cuda") * 0.6
        ops.mask_pack(logits.contiguous(), 0.0, 1.0, out=(bits,) + areas, row=k0)
    score = torch.rand(K, generator=g, device="cuda")
    return xyz, bits, areas, score


def run_case(name, repeats, host_rows, min_points):
    import region_reference as R
    import scene_reference as SR
    c = CASES[name]
    N, K = c["points"], c["rows"]
    xyz, bits, (area, area_hi, area_lo), score = blobs(N, K, 7)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    graph, build_ms = timed(lambda: regions.build_graph(xyz), repeats)
    build_wall = (time.perf_counter() - t0) * 1e3 / (repeats + 1)
    _, nbr_ms = timed(lambda: ops.region_neighbors(xyz, graph.keep_idx, graph.voxel_size), repeats)
    V = graph.keep_idx.numel()
    cfg = regions.RegionConfig(min_island=min_points, min_hole=min_points)
    # agreement with the host composition on the first rows, which is also the host's timing
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host_masks = SR.unwords(bits[:host_rows].cpu().numpy().view(np.uint64), N)
    ref = R.Graph(xyz.cpu().numpy(), graph.voxel_size)
    t1 = time.perf_counter()
    want, want_area, want_changed, _ = R.clean(ref, host_masks, min_points, min_points)
    t2 = time.perf_counter()
    got, got_area, got_changed = regions.clean_bits(graph, bits[:host_rows].contiguous(), cfg=cfg)
    assert np.array_equal(got.cpu().numpy().view(np.uint64), SR.words(want)), "device and host clean-up differ"
    assert np.array_equal(got_area.cpu().numpy(), want_area) and np.array_equal(got_changed.cpu().numpy(), want_changed)
    _, label_ms = timed(lambda: regions.components(graph, bits), repeats)
    (cb, ca, cc), clean_ms = timed(lambda: regions.clean_bits(graph, bits, cfg=cfg), repeats)

    def rest():
        order = torch.sort(score, descending=True, stable=True).indices.to(torch.int32)
        valid = ops.mask_valid(ca, area_hi, area_lo, score, N, 1, 1.0001, float("-inf"), float("-inf"))
        keep = ops.mask_nms(order, valid, ca, ops.mask_intersections(cb), 0.7)
        return ops.mask_paint(cb, order, keep, N)

    _, rest_ms = timed(rest, repeats)
    return dict(case=name, points=N, rows=K, voxels=V, voxel_size=graph.voxel_size, min_points=min_points, rows_per_call=regions.rows_per_call(graph),
                rows_changed=int(cc.sum()), points_removed_or_added=int((ca.long() - area.long()).abs().sum()),
                device_ms=dict(graph_build=stat(build_ms), graph_build_wall=round(build_wall, 3), neighbors_only=stat(nbr_ms), labels=stat(label_ms),
                               clean=stat(clean_ms), rest_of_post_processing=stat(rest_ms)),
                host_scipy_ms=dict(rows=host_rows, graph_build=round((t1 - t0) * 1e3, 2), clean=round((t2 - t1) * 1e3, 2),
                                   clean_scaled_to_all_rows=round((t2 - t1) * 1e3 * K / host_rows, 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="proposals,scene")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-rows", type=int, default=16)
    ap.add_argument("--min-points", type=int, default=25)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = []
    for name in args.cases.split(","):
        res = run_case(name, args.repeats, args.host_rows, args.min_points)
        print(json.dumps(res), flush=True)
        out.append(res)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
