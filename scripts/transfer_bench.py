"""Times the radius 3-NN transfer between two scans (csrc/transfer.hip, point_sam_amd/transfer.py) next to a torch-composed search.

    python scripts/transfer_bench.py [--points 4194304,10000000] [--working 131072] [--repeats 20] [--torch-queries 262144] [--no-model] [--out FILE.json]

One process, one GPU.  Sources: the working cloud (at most `--working` points) of one synthetic scan of scripts/scene_bench.py.  Queries: a second scan
(another seed) of `--points` points, given in a frame from which a small rigid pose leads back to the first.  Radius: twice the working voxel size.
Each figure is the median of `--repeats` device-event times after two warm-up rounds, with min and max.

  index       ops.transfer_index (clear, insert; includes its one host read of the bounds, so it is wall time)
  plan        ops.transfer_plan over all queries; against it a torch-composed plan: `cdist` to every source, `topk(3, largest=False)`, a radius cut,
              weights, 4096 queries at a time (a [4096, Nw] distance block is 2 GiB at Nw = 131072).  The composed plan costs M * Nw distances, so it is
              timed on the first `--torch-queries` queries only, ALTERNATING with the native plan on the same prefix; both are reported for that prefix.
              cdist runs in its default matrix-product form, |p|^2 + |s|^2 - 2 p.s, whose cancellation error (about 1e-7 absolute on a squared distance
              of 1e-4) reorders near neighbours, and topk breaks ties differently: the two are compared by the share of equal index rows, not required
              to be identical.  (The direct form, compute_mode="donot_use_mm_for_euclid_dist", returned wrong distances for a [4096, 95244] block on the
              MI355X it was tried on -- 1 % of its nearest neighbours agreed with an fp64 cdist, the native plan equalled the numpy reference -- so it is
              not used.)
  apply       ops.scene_interp_bits through transfer.transfer_bits per click, [3, Nw] logits
  propagate   predictor.propagate end to end (wall time) with ViT-L, random weights, the tokenizer of scripts/scene_bench.py (skipped with --no-model)
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scene_bench import TOKENIZER, alternate, event, make_scan, pair, stat, wall  # noqa: E402

from point_sam_amd import get_config, ops, scene, transfer  # noqa: E402

CHUNK = 4096
POSE = torch.tensor([[0.9998, -0.02, 0.0, 0.004], [0.02, 0.9998, 0.0, -0.003], [0.0, 0.0, 1.0, 0.002]], dtype=torch.float64)      # ~1.15 degrees about z


def rigid_pose():
    """A proper rotation (the rows above re-orthonormalised) and a small translation, 3 x 4 float64."""
    u, _, vt = torch.linalg.svd(POSE[:, :3])
    return torch.cat([u @ vt, POSE[:, 3:]], 1)


def torch_plan(src, r2, xyz, pose, eps=1e-8):
    """The plan composed from torch operators, chunked.  -> (idx3 [M, 3] int32, w3 [M, 3] f32)."""
    M, dev = xyz.shape[0], xyz.device
    idx3 = torch.empty(M, 3, dtype=torch.int32, device=dev)
    w3 = torch.empty(M, 3, dtype=torch.float32, device=dev)
    R, t = pose[:, :3].to(dev, torch.float32), pose[:, 3].to(dev, torch.float32)
    for lo in range(0, M, CHUNK):
        p = xyz[lo:lo + CHUNK] @ R.T + t
        q = torch.cdist(p, src).square_()              # the matrix-product form (|p|^2 + |s|^2 - 2 p.s): see the module docstring
        q3, j3 = torch.topk(q, 3, dim=1, largest=False)
        used = q3 <= r2
        a = torch.where(used, 1.0 / q3.clamp_min(eps), torch.zeros((), device=dev))
        w = a / a.sum(1, keepdim=True)
        hit = used[:, 0] & ((q3[:, 0] == 0) | ~used[:, 1])
        used = used & ~(hit[:, None] & (torch.arange(3, device=dev)[None] > 0))
        idx3[lo:lo + CHUNK] = torch.where(used, j3, torch.full((), -1, device=dev, dtype=torch.int64)).to(torch.int32)
        w3[lo:lo + CHUNK] = torch.where(hit[:, None], used.to(torch.float32), torch.where(used, w, torch.zeros((), device=dev)))
    return idx3, w3


def run(M, working, repeats, torch_queries, model):
    pose = rigid_pose()
    axyz, argb = make_scan(M, 5)
    bxyz, brgb = make_scan(M, 6)
    bxyz = ((bxyz.double() - pose[:, 3].cuda()) @ pose[:, :3].cuda()).float().clamp_(-1, 1).contiguous()      # q = R^T (p - t)
    h = scene.choose_voxel_size(axyz, working)
    keep_idx, _ = ops.voxel_downsample(axyz, h)
    src = axyz.index_select(0, keep_idx).contiguous()
    Nw, radius = src.shape[0], 2 * h
    res = dict(points=M, max_points=working, voxel_size=h, sources=Nw, radius=radius, repeats=repeats, plan_bytes=24 * M)

    res["index_wall_ms"] = stat([wall(lambda: ops.transfer_index(src, radius))[1] for _ in range(repeats + 2)][2:])
    index = ops.transfer_index(src, radius)
    res["index_workspace_bytes"] = index.ws.numel() * 8
    times = [event(lambda: ops.transfer_plan(index, bxyz, pose))[1] for _ in range(repeats + 2)][2:]
    res["plan_ms"] = stat(times)
    res["plan_queries_per_us"] = round(M / (res["plan_ms"]["median"] * 1e3), 2)
    idx3, w3 = ops.transfer_plan(index, bxyz, pose)
    res["plan_shape"] = dict(none=round(float((idx3[:, 0] < 0).float().mean()), 4), copy=round(float(((idx3[:, 0] >= 0) & (idx3[:, 1] < 0)).float().mean()), 4),
                             two=round(float(((idx3[:, 1] >= 0) & (idx3[:, 2] < 0)).float().mean()), 4), three=round(float((idx3[:, 2] >= 0).float().mean()), 4))

    T = min(torch_queries, M)
    head = bxyz[:T].contiguous()
    ti, _ = torch_plan(src, float(index.r2), head, pose)
    res["torch_prefix_queries"] = T
    res["prefix_rows_equal_to_torch_composed"] = round(float((ti == idx3[:T]).all(1).float().mean()), 6)
    res["prefix_first_index_equal"] = round(float((ti[:, 0] == idx3[:T, 0]).float().mean()), 6)
    del ti
    res["plan_prefix"] = pair(*alternate(lambda: ops.transfer_plan(index, head, pose), lambda: torch_plan(src, float(index.r2), head, pose), event, min(repeats, 5)))

    centres = torch.tensor([[0.0, 0.0, 0.0], [0.3, -0.2, 0.1], [-0.4, 0.4, -0.5]], device="cuda")
    logits = (torch.tensor([[0.6], [0.35], [0.5]], device="cuda") - torch.cdist(centres, src)).contiguous()      # [3, Nw]
    plan = transfer.TransferPlan(idx3, w3, Nw)
    res["transfer_bits_3_ms"] = stat([event(lambda: transfer.transfer_bits(plan, logits, 0.0))[1] for _ in range(repeats + 2)][2:])
    res["transfer_bits_area"] = transfer.transfer_bits(plan, logits, 0.0)[1].tolist()

    if model is not None:
        from point_sam_amd.predictor import PointSAMPredictor
        pred = PointSAMPredictor(model)
        pred.set_scene(axyz, argb, max_points=working)
        snap = pred.snapshot(logits)
        pred.set_scene(bxyz, brgb, max_points=working)
        for clicks in (1, 2):
            out = pred.propagate(snap, radius, pose, clicks=clicks)
            res[f"propagate_{clicks}_click_wall_ms"] = stat([wall(lambda: pred.propagate(snap, radius, pose, clicks=clicks))[1] for _ in range(min(repeats, 5) + 1)][1:])
        res["propagate"] = dict(lost=out.lost.tolist(), prior_area=out.prior_area.tolist(), covered=round(out.covered, 4),
                                area=(out.logits > 0).sum(1).tolist(), working_points=pred.scene.num_working)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4194304,10000000")
    ap.add_argument("--working", type=int, default=131072)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--torch-queries", type=int, default=1 << 18)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    model = None
    if not args.no_model:
        from point_sam_amd.model import PointCloudSAM
        from point_sam_amd.weights import random_state_dict
        cfg = get_config("large", *TOKENIZER[args.working])
        model = PointCloudSAM(cfg, random_state_dict(cfg, 1), "cuda", precision="f16x3")
    out = []
    for M in (int(m) for m in args.points.split(",")):
        res = run(M, args.working, args.repeats, args.torch_queries, model)
        print(json.dumps(res), flush=True)
        out.append(res)
        torch.cuda.empty_cache()
        if args.out:                                       # after every configuration: a run that is cut short keeps what it measured
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
