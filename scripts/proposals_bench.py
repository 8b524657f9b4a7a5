"""Times the automatic mask proposals (point_sam_amd/proposals.py) stage by stage, next to a torch-composed baseline of the same post-processing.

    python scripts/proposals_bench.py [--sizes small,large] [--prompts 1024] [--repeats 5] [--out FILE.json]

One process, one GPU, ViT-L with random weights: `small` = N 32768, 512 x 64 groups, 64 prompts per decode; `large` = N 131072, 2048 x 256 groups,
16 prompts per decode.  Per size: the decode time per chunk and in total, and pack / intersections / nms (sort + validity + suppression) / paint
each, by device events, native and torch-composed ALTERNATING in the same run on the same logits.  The two must agree on `keep` and on the labels
before anything is timed.

The torch-composed baseline is what one writes without the kernels: `(logits > thr)` kept as fp32 rows, `m @ m.T` for the intersections (exact in
fp32: 0/1 products, sums below 2^24), the fp64 IoU test on the device, the over-threshold matrix copied to the host ONCE and the greedy loop in
numpy on it (kinder to the baseline than a loop with a synchronisation per kept mask), labels by a masked minimum over the kept rows.  Its nms
figure is wall time around a synchronised region, because part of it runs on the host.

Random weights give degenerate masks at threshold 0 (nearly every candidate covers all of the cloud or none of it), which would make suppression
and painting trivial; the threshold is therefore the median logit of the first chunk and only the area filter's lower bound (1 point) applies.
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

from point_sam_amd import get_config, ops  # noqa: E402
from point_sam_amd.model import PointCloudSAM  # noqa: E402
from point_sam_amd.weights import random_state_dict  # noqa: E402

SIZES = {"small": dict(points=32768, groups=512, group_size=64, chunk=64), "large": dict(points=131072, groups=2048, group_size=256, chunk=16)}
NMS_THR, OFF = 0.7, 1.0


class Timer:
    """Device events around a region on the current stream; .ms() after a synchronise."""

    def __init__(self):
        self.pairs = []

    def __enter__(self):
        self.s, self.e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.s.record()
        return self

    def __exit__(self, *exc):
        self.e.record()
        self.pairs.append((self.s, self.e))

    def ms(self):
        return [s.elapsed_time(e) for s, e in self.pairs]


def cloud(N, seed):
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(1, N, 3, generator=g) * 2 - 1
    xyz = xyz - xyz.mean(dim=1, keepdim=True)
    xyz = xyz / xyz.norm(dim=2).max(dim=1).values.view(1, 1, 1)
    return xyz.cuda().contiguous(), (torch.rand(1, N, 3, generator=g) * 2 - 1).cuda().contiguous()


def torch_post(mf, area, area_hi, area_lo, score, N, thr_nms):
    """The torch-composed post-processing after its 'pack' -> (keep [K] bool on the host, labels [N] on the device, (t_inter, t_nms, t_paint) ms)."""
    K = mf.shape[0]
    ti, tp = Timer(), Timer()
    with ti:
        inter = mf @ mf.T
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    order = torch.sort(score, descending=True, stable=True).indices
    valid = (area >= 1) & (area_lo > 0) & (score == score)
    io = inter[order][:, order].double()
    ao = area[order].double()
    over = (io > float(np.float32(thr_nms)) * (ao[:, None] + ao[None, :] - io)).cpu().numpy()      # the one copy to the host
    vo = valid[order].cpu().numpy()
    removed = ~vo
    keep_o = np.zeros(K, dtype=bool)
    for p in range(K):
        if not removed[p]:
            keep_o[p] = True
            removed[p + 1:] |= over[p, p + 1:]
    t_nms = (time.perf_counter() - t0) * 1e3
    kept = order[torch.from_numpy(keep_o).cuda()]
    with tp:
        k = kept.numel()
        lab = torch.full((N,), k, dtype=torch.int64, device=mf.device)
        for r0 in range(0, k, 256):      # blocks of 256 kept rows: the masked minimum needs an int64 [rows, N] temporary
            rows = mf[kept[r0:r0 + 256]] > 0
            idx = torch.arange(r0, r0 + rows.shape[0], device=mf.device)[:, None]
            lab = torch.minimum(lab, torch.where(rows, idx, k).min(0).values)
        lab = torch.where(lab == k, -1, lab).to(torch.int32)
    torch.cuda.synchronize()
    keep = np.zeros(K, dtype=bool)
    keep[order.cpu().numpy()[keep_o]] = True
    return keep, lab, (ti.ms()[0], t_nms, tp.ms()[0])


def native_post(bits, area, area_hi, area_lo, score, N, thr_nms):
    ti, tn, tp = Timer(), Timer(), Timer()
    with ti:
        inter = ops.mask_intersections(bits)
    with tn:
        order = torch.sort(score, descending=True, stable=True).indices.to(torch.int32)
        valid = ops.mask_valid(area, area_hi, area_lo, score, N, 1, 1.0001, float("-inf"), 0.0)
        keep = ops.mask_nms(order, valid, area, inter, thr_nms)
    with tp:
        labels = ops.mask_paint(bits, order, keep, N)
    torch.cuda.synchronize()
    return keep.cpu().numpy().astype(bool), labels, (ti.ms()[0], tn.ms()[0], tp.ms()[0])


def run_size(name, prompts, repeats):
    s = SIZES[name]
    N, chunk = s["points"], s["chunk"]
    cfg = get_config("large", s["groups"], s["group_size"])
    model = PointCloudSAM(cfg, random_state_dict(cfg, 1), "cuda", precision="f16x3")
    xyz, rgb = cloud(N, 11)
    st = model.encode(xyz, rgb)
    _, pts = ops.fps(st.coords, prompts)
    ones = torch.ones(chunk, 1, dtype=torch.int64, device="cuda")
    K, W = 3 * prompts, ops.mask_words(N)
    for _ in range(2):                                    # warm-up: decode, both packs
        logits, iou = model.decode(st, pts[:, :chunk].reshape(chunk, 1, 3), ones, None, True)
    thr = float(logits.median())
    bufs = (torch.empty(K, W, dtype=torch.int64, device="cuda"),) + tuple(torch.empty(K, dtype=torch.int32, device="cuda") for _ in range(3))
    mf = torch.empty(K, N, dtype=torch.float32, device="cuda")
    t_area = [torch.empty(K, dtype=torch.int32, device="cuda") for _ in range(3)]
    score = torch.empty(K, dtype=torch.float32, device="cuda")
    hi, lo = float(np.float32(thr) + np.float32(OFF)), float(np.float32(thr) - np.float32(OFF))
    for _ in range(2):                                    # warm-up of both packs on the warm-up chunk (first-use costs of the torch ops are not timed)
        ops.mask_pack(logits, thr, OFF, out=bufs, row=0)
        l2 = logits.view(-1, N)
        mf[:3 * chunk] = l2 > thr
        t_area[0][:3 * chunk] = (l2 > thr).sum(1); t_area[1][:3 * chunk] = (l2 > hi).sum(1); t_area[2][:3 * chunk] = (l2 > lo).sum(1)
    td, tpn, tpt = Timer(), Timer(), Timer()
    torch.cuda.synchronize()
    for m0 in range(0, prompts, chunk):
        c = min(chunk, prompts - m0)
        with td:
            logits, iou = model.decode(st, pts[:, m0:m0 + c].reshape(c, 1, 3), ones[:c], None, True)
        rows = slice(3 * m0, 3 * (m0 + c))
        order_ab = (0, 1) if (m0 // chunk) % 2 == 0 else (1, 0)
        for which in order_ab:
            if which == 0:
                with tpn:
                    ops.mask_pack(logits, thr, OFF, out=bufs, row=3 * m0)
            else:
                with tpt:
                    l2 = logits.view(-1, N)
                    m = l2 > thr
                    mf[rows] = m
                    t_area[0][rows] = m.sum(1); t_area[1][rows] = (l2 > hi).sum(1); t_area[2][rows] = (l2 > lo).sum(1)
        score[rows] = iou.reshape(-1)
    torch.cuda.synchronize()
    model.check_coordinate_range()
    for a, b in zip(bufs[1:], t_area):
        assert torch.equal(a, b), "areas of the two packs differ"
    assert torch.equal(ops.mask_unpack(bufs[0][:64], N), mf[:64] > 0)
    # agreement first, then the alternating repeats
    kn, ln, _ = native_post(*bufs, score, N, NMS_THR)
    kt, lt, _ = torch_post(mf, *t_area, score, N, NMS_THR)
    assert np.array_equal(kn, kt), "native and torch-composed NMS disagree on keep"
    assert torch.equal(ln, lt), "native and torch-composed labels differ"
    nat, tor = [], []
    for r in range(repeats):
        for which in ((0, 1) if r % 2 == 0 else (1, 0)):
            if which == 0:
                nat.append(native_post(*bufs, score, N, NMS_THR)[2])
            else:
                tor.append(torch_post(mf, *t_area, score, N, NMS_THR)[2])

    def stat(v):
        return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))

    pairs = K * K * W                                      # 64-bit and + popcount of the full matrix; the mirrored path computes ~half of them
    res = dict(size=name, points=N, groups=s["groups"], group_size=s["group_size"], prompts=prompts, prompt_chunk=chunk, candidates=K, kept=int(kn.sum()),
               mask_threshold=thr, decode_ms=dict(per_chunk=stat(td.ms()), total=round(sum(td.ms()), 3), chunks=len(td.ms())),
               native_ms=dict(pack_total=round(sum(tpn.ms()), 4), pack_per_chunk=stat(tpn.ms()), intersections=stat([t[0] for t in nat]),
                              nms=stat([t[1] for t in nat]), paint=stat([t[2] for t in nat])),
               torch_ms=dict(pack_total=round(sum(tpt.ms()), 4), pack_per_chunk=stat(tpt.ms()), intersections=stat([t[0] for t in tor]),
                             nms=stat([t[1] for t in tor]), paint=stat([t[2] for t in tor])),
               bytes=dict(chunk_logits=chunk * 3 * N * 4, native=dict(bits=K * W * 8, inter=K * K * 4, nms_workspace=(K + 1) * ((K + 63) // 64) * 8),
                          torch=dict(masks_f32=K * N * 4, inter_f32=K * K * 4, iou_test_f64=3 * K * K * 8)))
    it = res["native_ms"]["intersections"]["median"]
    res["intersections_and_popcount_per_s"] = dict(full_matrix_count=pairs, computed_count=(K // 64) * (K // 64 + 1) // 2 * 64 * 64 * W,
                                                   rate_full_matrix=round(pairs / (it * 1e-3)), rate_computed=round((K // 64) * (K // 64 + 1) // 2 * 4096 * W / (it * 1e-3)))
    post = sum(res["native_ms"][k]["median"] for k in ("intersections", "nms", "paint")) + res["native_ms"]["pack_total"]
    res["native_post_ms"] = round(post, 3)
    res["native_post_share_of_decode"] = round(post / res["decode_ms"]["total"], 5)
    res["torch_post_ms"] = round(sum(res["torch_ms"][k]["median"] for k in ("intersections", "nms", "paint")) + res["torch_ms"]["pack_total"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="small,large")
    ap.add_argument("--prompts", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = []
    for name in args.sizes.split(","):
        res = run_size(name, args.prompts, args.repeats)
        print(json.dumps(res), flush=True)
        out.append(res)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
