"""Times a scene crop (point_sam_amd/scene.py: build_crop, predictor.set_crop) stage by stage, next to a torch-composed version of the crop build, and
the multi-crop proposal merge.

    python scripts/crops_bench.py [--points 2000000,10000000] [--crop-points 32768] [--repeats 10] [--out FILE.json]

One process, one GPU, ViT-L with random weights (512 groups of 64: crop clouds of up to 32768 points).  Per scan size, on the scan of
scripts/scene_bench.py and a ball around a point of its sphere shell that holds about a tenth of the points:

  crop_build        ops.crop_downsample at the crop's voxel size (one call: select, normalise, voxel-reduce, compact, gather) against the composition
                    in torch -- compare, nonzero, index_select of xyz and rgb, subtract / scale / clamp, ops.voxel_downsample of the normalised
                    members, the gathers and the scatter of inv -- ALTERNATING in the same run on the same data; the two must agree exactly first
  crop_count        one count-only pass (the voxel-size bisection runs about eight)
  build_crop        scene.build_crop with max_points: the member count, the bisection and the build
  encode            the encoder on the crop cloud
  set_crop          the predictor's call, uncached (build_crop + encode)
  click             predict_masks under the crop (decode + paste-back of 3 rows), and the paste-back of 3 rows / of `--masks` packed masks alone
  multi_crop        generate_masks(cfg, crops=CropLayerConfig(num_crops=2)) end to end, and proposals.merge_proposals alone on its layers

build figures are wall time around a synchronised region (both sides read counts on the host); the others are device-event times.  Every figure is
the median of `--repeats` repetitions after two warm-up rounds, with min and max.
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

from point_sam_amd import get_config, ops, scene  # noqa: E402
from point_sam_amd.model import PointCloudSAM  # noqa: E402
from point_sam_amd.predictor import PointSAMPredictor  # noqa: E402
from point_sam_amd.proposals import CropLayerConfig, ProposalConfig, generate_proposals, merge_proposals  # noqa: E402
from point_sam_amd.weights import random_state_dict  # noqa: E402


def torch_crop(xyz, rgb, center, radius, h):
    """The crop build without csrc/crops.hip: the same fp32 arithmetic, six passes over the scan and a hash table sized for the members."""
    r = np.float32(radius)
    r2, inv_r = float(r * r), float(np.float32(1) / r)
    c = torch.tensor(center, dtype=torch.float32, device=xyz.device)
    d = xyz - c
    q = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    idx = torch.nonzero(q <= r2)[:, 0]
    mx, mr = xyz.index_select(0, idx), rgb.index_select(0, idx)
    u = torch.clamp((mx - c) * inv_r, -1.0, 1.0)
    keep_local, inv_local = ops.voxel_downsample(u, h)
    inv = torch.full((xyz.shape[0],), -1, dtype=torch.int64, device=xyz.device)
    inv[idx] = inv_local
    return idx[keep_local], inv, u.index_select(0, keep_local), mr.index_select(0, keep_local)


def run(M, model, crop_points, repeats, n_masks):
    xyz, rgb = make_scan(M, 5)
    pred = PointSAMPredictor(model)
    one = torch.ones(1, 1, dtype=torch.int64, device="cuda")
    # the ball: around the scan point nearest to (0.6, 0, 0) (the sphere shell), as wide as the nearest tenth of the points
    center_idx = int(torch.argmin((xyz - torch.tensor([0.6, 0.0, 0.0], device="cuda")).norm(dim=1)))
    center = tuple(xyz[center_idx].tolist())
    radius = float(torch.quantile((xyz[::max(1, M // 1000000)] - xyz[center_idx]).norm(dim=1), 0.1))
    res = dict(points=M, crop_points=crop_points, center=center, radius=radius, repeats=repeats)

    (crop, wxyz, wrgb), _ = wall(lambda: scene.build_crop(xyz, rgb, center, radius, max_points=crop_points))
    h = crop.voxel_size
    res.update(members=crop.num_members, member_fraction=round(crop.num_members / M, 4), voxel_size=h, working_points=crop.num_working)
    assert h is not None, "the ball fits into --crop-points: nothing would be reduced"
    native = ops.crop_downsample(xyz, rgb, center, radius, h)
    composed = torch_crop(xyz, rgb, center, radius, h)
    assert all(torch.equal(a, b) for a, b in zip(native[:4], composed)), "native and torch-composed crop build disagree"
    del native, composed
    res["crop_build"] = pair(*alternate(lambda: ops.crop_downsample(xyz, rgb, center, radius, h), lambda: torch_crop(xyz, rgb, center, radius, h), wall, repeats))
    res["crop_count_ms"] = stat([wall(lambda: ops.crop_count(xyz, center, radius, h))[1] for _ in range(repeats + 2)][2:])
    res["build_crop_ms"] = stat([wall(lambda: scene.build_crop(xyz, rgb, center, radius, max_points=crop_points))[1] for _ in range(repeats + 2)][2:])
    res["encode_ms"] = stat([event(lambda: model.encode(wxyz[None], wrgb[None]))[1] for _ in range(repeats + 2)][2:])

    pred.set_scene(xyz, rgb, max_points=crop_points)

    def set_crop():
        pred._crop_cache = None                            # uncached: build and encode every time
        pred.set_crop(center, radius, max_points=crop_points)

    res["set_crop_ms"] = stat([wall(set_crop)[1] for _ in range(repeats + 2)][2:])
    click = xyz[crop.keep_idx[crop.num_working // 2]].view(1, 1, 3)
    res["click_under_crop_ms"] = stat([event(lambda: pred.predict_masks(click, one, None, True))[1] for _ in range(repeats + 2)][2:])
    logits, _ = model.decode(pred._crop_state, scene.crop_prompts(crop, click), one, None, True)
    rows = logits.reshape(-1, crop.num_working)
    res["paste_logits_3_rows_ms"] = stat([event(lambda: ops.crop_expand_rows(rows, crop.inv, float("-inf")))[1] for _ in range(repeats + 2)][2:])
    bits_w = torch.randint(-2 ** 62, 2 ** 62, (n_masks, ops.mask_words(crop.num_working)), dtype=torch.int64, device="cuda")
    res["paste_masks_ms"] = dict(masks=n_masks, **stat([event(lambda: ops.crop_expand_bits(bits_w, crop.inv, crop.num_working))[1] for _ in range(repeats + 2)][2:]))
    pred.clear_crop()

    # multi-crop proposals: 64 prompts per layer, two crops
    pc = ProposalConfig(num_prompts=64, prompt_chunk=64, pred_iou_thresh=float("-inf"), stability_thresh=0.0, min_points=1, max_area_frac=1.0001)
    cl = CropLayerConfig(num_crops=2, radius=radius, max_points=crop_points)
    few = max(3, repeats // 3)
    res["multi_crop_ms"] = dict(num_crops=2, prompts_per_layer=64, **stat([wall(lambda: pred.generate_masks(pc, crops=cl))[1] for _ in range(few + 1)][1:]))
    base = scene.expand_proposals(pred.scene, generate_proposals(model, pred._state, pc)[0])
    under = pred.generate_masks(pc)                        # stands in for a crop layer: any scan-width rows do for the merge's cost
    layers = [(-1, base), (0, under[0]), (1, base)]
    res["merge_ms"] = dict(rows=sum(len(p) for _, p in layers), **stat([wall(lambda: merge_proposals(layers, M, cl.nms_thresh))[1] for _ in range(few + 1)][1:]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="2000000,10000000")
    ap.add_argument("--crop-points", type=int, default=32768)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--masks", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg = get_config("large", 512, 64)
    model = PointCloudSAM(cfg, random_state_dict(cfg, 1), "cuda", precision="f16x3")
    out = []
    for M in (int(m) for m in args.points.split(",")):
        res = run(M, model, args.crop_points, args.repeats, args.masks)
        print(json.dumps(res), flush=True)
        out.append(res)
        torch.cuda.empty_cache()
        if args.out:                                       # after every size: a run that is cut short keeps what it measured
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
