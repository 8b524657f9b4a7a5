"""Times a full-resolution scene (point_sam_amd/scene.py) stage by stage, next to a torch-composed version of the same reduction and transfer.

    python scripts/scene_bench.py [--points 1048576,4194304] [--working 32768,131072] [--repeats 20] [--masks 256] [--out FILE.json]

One process, one GPU, ViT-L with random weights (working clouds up to 32768 points: 512 x 64 groups; up to 131072: 2048 x 256).  Per (scan size,
working size): the voxel-size search (count-only passes), the downsample, the encode of the working cloud, one click (decode), and the expansion of
the click's logits (3 rows), of int32 labels (1 row) and of `--masks` packed masks -- native and torch-composed ALTERNATING in the same run on the same
data, each the median of `--repeats` timed repetitions after two warm-up rounds, with min and max.  The two must agree exactly before anything is timed.

The torch-composed version is what one writes without the kernels: cells by the same fp32 arithmetic, `torch.unique(keys, return_inverse=True)`,
`scatter_reduce(amin)` of the point indices for the representatives, an argsort to rank them by index; `index_select` for the rows; for the masks the
working rows unpacked to bool, `index_select`, and the areas by `sum` (the result stays one byte per point and mask: torch has no bit pack).

The downsample figures are wall time around a synchronised region for both sides (both read a count on the host: the native call once, `torch.unique`
inside); the other stages are device-event times.

The scan: points on a sphere shell, a floor and two walls inside [-1, 1]^3, each surface sample repeated 8 times in a row with a jitter of 1e-3 (a
sensor that oversamples: neighbouring indices usually share a voxel), random colours.
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

from point_sam_amd import get_config, ops, scene  # noqa: E402
from point_sam_amd.model import PointCloudSAM  # noqa: E402
from point_sam_amd.predictor import PointSAMPredictor  # noqa: E402
from point_sam_amd.weights import random_state_dict  # noqa: E402

TOKENIZER = {32768: (512, 64), 131072: (2048, 256)}


def make_scan(M, seed):
    g = torch.Generator().manual_seed(seed)
    S = (M + 7) // 8
    u = torch.rand(S, 3, generator=g)
    kind = torch.randint(0, 4, (S,), generator=g)
    d = torch.randn(S, 3, generator=g)
    sphere = 0.6 * d / d.norm(dim=1, keepdim=True)
    floor = torch.stack([u[:, 0] * 1.8 - 0.9, u[:, 1] * 1.8 - 0.9, torch.full((S,), -0.9)], 1)
    wall_a = torch.stack([torch.full((S,), -0.9), u[:, 1] * 1.8 - 0.9, u[:, 2] * 1.8 - 0.9], 1)
    wall_b = torch.stack([u[:, 0] * 1.8 - 0.9, torch.full((S,), 0.9), u[:, 2] * 1.8 - 0.9], 1)
    base = torch.where((kind == 0)[:, None], sphere, torch.where((kind == 1)[:, None], floor, torch.where((kind == 2)[:, None], wall_a, wall_b)))
    xyz = (base.repeat_interleave(8, 0)[:M] + 1e-3 * torch.randn(M, 3, generator=g)).clamp_(-1, 1)
    rgb = torch.rand(M, 3, generator=g) * 2 - 1
    return xyz.cuda().contiguous(), rgb.cuda().contiguous()


def torch_downsample(xyz, h):
    M = xyz.shape[0]
    inv_h = float(np.float32(1) / np.float32(h))
    c = torch.floor((xyz + 1.0) * inv_h).to(torch.int64)
    keys = c[:, 0] | (c[:, 1] << 21) | (c[:, 2] << 42)
    uniq, inverse = torch.unique(keys, return_inverse=True)
    first = torch.full((uniq.numel(),), M, dtype=torch.int64, device=xyz.device).scatter_reduce_(
        0, inverse, torch.arange(M, dtype=torch.int64, device=xyz.device), "amin", include_self=True)
    order = torch.argsort(first)
    rank = torch.empty_like(order)
    rank[order] = torch.arange(order.numel(), dtype=torch.int64, device=xyz.device)
    return first[order], rank[inverse]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def event(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return out, s.elapsed_time(e)


def alternate(native, composed, timer, repeats):
    """-> (native times, torch-composed times): two warm-up rounds, then `repeats` rounds, the order swapped every round."""
    for _ in range(2):
        native(); composed()
    torch.cuda.synchronize()
    a, b = [], []
    for r in range(repeats):
        for which in ((0, 1) if r % 2 == 0 else (1, 0)):
            (a if which == 0 else b).append(timer(native if which == 0 else composed)[1])
    return a, b


def stat(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), n=len(v))


def pair(a, b):
    return dict(native_ms=stat(a), torch_ms=stat(b), torch_over_native=round(statistics.median(b) / statistics.median(a), 3))


def run(M, working, models, repeats, n_masks):
    xyz, rgb = make_scan(M, 5)
    model = models[working]
    pred = PointSAMPredictor(model)
    one = torch.ones(1, 1, dtype=torch.int64, device="cuda")
    res = dict(points=M, max_points=working, groups=TOKENIZER[working][0], group_size=TOKENIZER[working][1], repeats=repeats)

    h = scene.choose_voxel_size(xyz, working)
    search = [wall(lambda: scene.choose_voxel_size(xyz, working))[1] for _ in range(repeats + 2)][2:]
    count1 = [wall(lambda: ops.voxel_count(xyz, h))[1] for _ in range(repeats + 2)][2:]
    keep_idx, inv = ops.voxel_downsample(xyz, h)
    tk, ti = torch_downsample(xyz, h)
    assert torch.equal(keep_idx, tk) and torch.equal(inv, ti), "native and torch-composed downsample disagree"
    Nw = keep_idx.numel()
    res.update(voxel_size=h, working_points=Nw, voxel_search_ms=stat(search), voxel_count_ms=stat(count1))
    res["downsample"] = pair(*alternate(lambda: ops.voxel_downsample(xyz, h), lambda: torch_downsample(xyz, h), wall, repeats))
    del tk, ti

    wx, wr = xyz.index_select(0, keep_idx)[None].contiguous(), rgb.index_select(0, keep_idx)[None].contiguous()
    gather = [event(lambda: (xyz.index_select(0, keep_idx), rgb.index_select(0, keep_idx)))[1] for _ in range(repeats + 2)][2:]
    enc = [event(lambda: model.encode(wx, wr))[1] for _ in range(repeats + 2)][2:]
    st = model.encode(wx, wr)
    click = xyz[keep_idx[Nw // 2]].view(1, 1, 3)
    dec = [event(lambda: model.decode(st, click, one, None, True))[1] for _ in range(repeats + 2)][2:]
    logits, _ = model.decode(st, click, one, None, True)
    model.check_coordinate_range()
    res.update(gather_working_cloud_ms=stat(gather), encode_ms=stat(enc), click_decode_ms=stat(dec))

    rows = logits.reshape(-1, Nw)
    assert torch.equal(ops.scene_expand_rows(rows, inv), rows.index_select(1, inv))
    res["expand_logits_3_rows"] = pair(*alternate(lambda: ops.scene_expand_rows(rows, inv), lambda: rows.index_select(1, inv), event, repeats))
    labels = torch.randint(-1, n_masks, (Nw,), dtype=torch.int32, device="cuda")
    assert torch.equal(ops.scene_expand_rows(labels, inv), labels.index_select(0, inv))
    res["expand_labels_1_row"] = pair(*alternate(lambda: ops.scene_expand_rows(labels, inv), lambda: labels.index_select(0, inv), event, repeats))

    # packed masks: balls around n_masks working points, thresholded at several radii
    centres = wx[0][torch.randperm(Nw, device="cuda")[:n_masks]]
    radius = torch.linspace(0.05, 0.6, n_masks, device="cuda")[:, None]
    bits_w, _, _, _ = ops.mask_pack((radius - torch.cdist(centres, wx[0])).contiguous(), 0.0, 0.0)

    def composed_bits():
        full = ops.mask_unpack(bits_w, Nw).index_select(1, inv)
        return full, full.sum(1, dtype=torch.int32)

    bits_f, area_f = ops.scene_expand_bits(bits_w, inv, Nw)
    full, area_t = composed_bits()
    assert torch.equal(area_f, area_t) and all(torch.equal(ops.mask_unpack(bits_f[k:k + 8], M), full[k:k + 8]) for k in range(0, n_masks, 64)), \
        "native and torch-composed mask expansion disagree"      # every area, and the bits of eight rows in every 64 (the unpack is 512 B per word)
    del full, area_t
    res["expand_masks"] = dict(masks=n_masks, **pair(*alternate(lambda: ops.scene_expand_bits(bits_w, inv, Nw), composed_bits, event, repeats)),
                               bytes=dict(native_bits=n_masks * ops.mask_words(M) * 8, torch_bool=n_masks * M, as_f32=n_masks * M * 4))
    pred.set_scene(xyz, rgb, max_points=working)
    assert pred.scene.num_working == Nw
    e2e = [event(lambda: pred.predict_masks(click, one, None, True))[1] for _ in range(repeats + 2)][2:]
    res["click_full_resolution_ms"] = stat(e2e)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1048576,4194304")
    ap.add_argument("--working", default="32768,131072")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--masks", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    working = [int(w) for w in args.working.split(",")]
    models = {}
    for w in working:
        cfg = get_config("large", *TOKENIZER[w])
        models[w] = PointCloudSAM(cfg, random_state_dict(cfg, 1), "cuda", precision="f16x3")
    out = []
    for M in (int(m) for m in args.points.split(",")):
        for w in working:
            res = run(M, w, models, args.repeats, args.masks)
            print(json.dumps(res), flush=True)
            out.append(res)
            torch.cuda.empty_cache()
            if args.out:                                   # after every configuration: a run that is cut short keeps what it measured
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
