"""Times the interpolated scene masks (csrc/scene_interp.hip) next to the exact voxel transfer they replace and to a torch-composed plan.

    python scripts/scene_interp_bench.py [--points 4194304,10000000] [--working 131072] [--repeats 20] [--out FILE.json]

One process, one GPU, no model: the logits are a synthetic [3, Nw] field on the working cloud (the kernels do not care where they come from).  The scan
is scripts/scene_bench.py's.  Per scan size, each figure the median of `--repeats` device-event times after two warm-up rounds, with min and max:

  plan        ops.region_neighbors + ops.scene_interp_plan (once per scene) against a torch-composed plan: `nbr[inv]` gather, coordinate gather,
              distances, `topk(3, largest=False)`, weights; chunked over the scan (2^20 points at a time) to fit memory.  torch's topk breaks distance
              ties differently, so the two are compared by the share of equal rows, not required to be identical.
  apply       per click, [3, Nw] logits: ops.scene_interp_rows against ops.scene_expand_rows, and ops.scene_interp_bits against
              ops.mask_pack + ops.scene_expand_bits -- alternating in the same run on the same data.
  agreement   on a 2^16-point sample: the share of scan points whose first plan index is the true nearest working point (ops.knn, K = 1).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scene_bench import alternate, event, make_scan, pair, stat  # noqa: E402

from point_sam_amd import ops, scene  # noqa: E402

CHUNK = 1 << 20


def torch_plan(xyz, inv, wxyz, nbr, eps=1e-8):
    """The plan composed from torch operators, chunked.  -> (idx3 [M, 3] int32, w3 [M, 3] f32)."""
    M = xyz.shape[0]
    idx3 = torch.empty(M, 3, dtype=torch.int32, device=xyz.device)
    w3 = torch.empty(M, 3, dtype=torch.float32, device=xyz.device)
    nbr64 = nbr.to(torch.int64)
    for lo in range(0, M, CHUNK):
        p, v = xyz[lo:lo + CHUNK], inv[lo:lo + CHUNK]
        cand = torch.cat([v[:, None], nbr64.index_select(0, v)], 1)                  # [n, 27]
        ok = cand >= 0
        d = p[:, None, :] - wxyz[cand.clamp_min(0)]
        q = torch.where(ok, (d * d).sum(-1), torch.full((), float("inf"), device=xyz.device))
        q3, pos = torch.topk(q, 3, dim=1, largest=False)
        r3 = torch.gather(cand, 1, pos)
        used = torch.isfinite(q3)
        a = torch.where(used, 1.0 / q3.clamp_min(eps), torch.zeros((), device=xyz.device))
        w = a / a.sum(1, keepdim=True)
        hit = (q3[:, 0] == 0) | ~used[:, 1]
        used = used & ~(hit[:, None] & (torch.arange(3, device=xyz.device)[None] > 0))
        idx3[lo:lo + CHUNK] = torch.where(used, r3, torch.full((), -1, device=xyz.device, dtype=torch.int64)).to(torch.int32)
        w3[lo:lo + CHUNK] = torch.where(hit[:, None], used.to(torch.float32), torch.where(used, w, torch.zeros((), device=xyz.device)))
    return idx3, w3


def run(M, working, repeats):
    xyz, _ = make_scan(M, 5)
    h = scene.choose_voxel_size(xyz, working)
    keep_idx, inv = ops.voxel_downsample(xyz, h)
    Nw = keep_idx.numel()
    wxyz = xyz.index_select(0, keep_idx)
    res = dict(points=M, max_points=working, voxel_size=h, working_points=Nw, repeats=repeats, plan_bytes=24 * M)

    nbr = ops.region_neighbors(xyz, keep_idx, h)
    res["neighbors_ms"] = stat([event(lambda: ops.region_neighbors(xyz, keep_idx, h))[1] for _ in range(repeats + 2)][2:])
    idx3, w3 = ops.scene_interp_plan(xyz, inv, wxyz, nbr)
    ti, tw = torch_plan(xyz, inv, wxyz, nbr)
    res["plan_rows_equal_to_torch_composed"] = round(float((ti == idx3).all(1).float().mean()), 6)
    res["plan_weights_max_abs_diff_where_rows_equal"] = float(((tw - w3).abs().amax(1))[(ti == idx3).all(1)].max())
    del ti, tw
    res["plan"] = pair(*alternate(lambda: ops.scene_interp_plan(xyz, inv, wxyz, nbr), lambda: torch_plan(xyz, inv, wxyz, nbr), event, repeats))
    res["plan_shape"] = dict(three=round(float((idx3[:, 2] >= 0).float().mean()), 4), two=round(float(((idx3[:, 1] >= 0) & (idx3[:, 2] < 0)).float().mean()), 4),
                             copy=round(float((idx3[:, 1] < 0).float().mean()), 4))

    # per click: three rows of logits, signed distances to three spheres
    centres = torch.tensor([[0.0, 0.0, 0.0], [0.3, -0.2, 0.1], [-0.4, 0.4, -0.5]], device="cuda")
    logits = (torch.tensor([[0.6], [0.35], [0.5]], device="cuda") - torch.cdist(centres, wxyz)).contiguous()      # [3, Nw]
    smooth = ops.scene_interp_rows(logits, idx3, w3)
    assert torch.equal(smooth.index_select(1, keep_idx), logits), "the representatives must keep their logits"
    a, b = alternate(lambda: ops.scene_interp_rows(logits, idx3, w3), lambda: ops.scene_expand_rows(logits, inv), event, repeats)
    res["apply_rows_3"] = dict(interp_ms=stat(a), expand_ms=stat(b), interp_over_expand=round(stat(a)["median"] / stat(b)["median"], 3),
                               bytes=dict(interp=M * (24 + 12), expand=M * (8 + 12)))

    def hard_bits():
        return ops.scene_expand_bits(ops.mask_pack(logits, 0.0, 0.0)[0], inv, Nw)

    bits, area = ops.scene_interp_bits(logits, idx3, w3, 0.0)
    want = ops.mask_pack(smooth, 0.0, 0.0) if M <= (1 << 24) else None
    assert want is None or (torch.equal(bits, want[0]) and torch.equal(area, want[1])), "bits and mask_pack of the rows disagree"
    a, b = alternate(lambda: ops.scene_interp_bits(logits, idx3, w3, 0.0), hard_bits, event, repeats)
    res["apply_bits_3"] = dict(interp_ms=stat(a), pack_expand_ms=stat(b), interp_over_expand=round(stat(a)["median"] / stat(b)["median"], 3),
                               changed_bits=[int(v) for v in ((bits ^ hard_bits()[0]) != 0).sum(1).tolist()], area=area.tolist())

    sample = torch.randperm(M, device="cuda")[:1 << 16]
    near = ops.knn(xyz.index_select(0, sample)[None].contiguous(), wxyz[None].contiguous(), 1)[0, :, 0]
    res["first_index_is_true_nearest"] = round(float((idx3.index_select(0, sample)[:, 0].to(torch.int64) == near).float().mean()), 6)
    res["own_representative_is_true_nearest"] = round(float((inv.index_select(0, sample) == near).float().mean()), 6)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4194304,10000000")
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
