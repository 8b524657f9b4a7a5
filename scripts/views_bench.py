"""Times the camera-view kernels (csrc/views.hip, point_sam_amd/views.py) next to a torch-composed splat.

    python scripts/views_bench.py [--points 1000000,10000000] [--width 1280] [--height 960] [--repeats 20] [--torch-repeats 5] [--out FILE.json]

One process, one GPU.  The scan: `--points` points uniform in the unit ball (seeded), seen from (0, 0, -3) with a 45 degree vertical field of view, so the
ball fills most of the image's height.  Each figure is the median of `--repeats` device-event times after two warm-up rounds, with min and max.

  splat       ops.view_splat at s = 0, 1, 2 (the clear and the point pass together).  With it what the pass must move at least (12 N bytes of xyz; the
              keys, 8 bytes per pixel, are written by the clear) and the atomics it may issue at most (one per offer: the in-view points times their
              clipped footprints, counted by the composed form).
              Against it the torch-composed splat: the projection as elementwise fp32 operators, then per footprint offset a range filter, an int64
              key build and `scatter_reduce_(amin)`.  Its keys are compared with ours first (`torch_keys_equal`); the two are then timed ALTERNATING on
              the same inputs.
  pick        ops.view_pick, window 2, for 1 click and for 1024 clicks
  paint_ids   ops.view_paint_ids at K = 3 and K = 256 random rows
  lift_bits   ops.view_lift_bits at K = 1 (no image: the visible set) and K = 8 images, tau = 0.05
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scene_bench import alternate, event, pair, stat  # noqa: E402

from point_sam_amd import ops  # noqa: E402
from point_sam_amd.views import Camera  # noqa: E402

EMPTY = torch.iinfo(torch.int64).max


def make_ball(N, seed):
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(N, 3, generator=g)
    r = torch.rand(N, 1, generator=g) ** (1.0 / 3.0)
    return (r * d / d.norm(dim=1, keepdim=True)).float().cuda().contiguous()


def torch_splat(xyz, cam, s, count=False):
    """-> (keys [H, W] int64 in view_splat's format, offers: the number of (point, pixel) pairs reduced, counted only on request)."""
    P = [float(v) for v in cam.pose_words]
    x, y, z = xyz.unbind(1)
    c = [((P[4 * a] * x + P[4 * a + 1] * y) + P[4 * a + 2] * z) + P[4 * a + 3] for a in range(3)]
    u = cam.fx * (c[0] / c[2]) + cam.cx
    v = cam.fy * (c[1] / c[2]) + cam.cy
    W, H = cam.width, cam.height
    ok = (c[2] >= cam.near) & torch.isfinite(c[2]) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    px = torch.where(ok, torch.floor(u), torch.zeros_like(u)).to(torch.int64)
    py = torch.where(ok, torch.floor(v), torch.zeros_like(v)).to(torch.int64)
    key = (c[2].view(torch.int32).to(torch.int64) << 32) | torch.arange(xyz.shape[0], dtype=torch.int64, device=xyz.device)      # c_z > 0 where it counts
    keys = torch.full((H * W,), EMPTY, dtype=torch.int64, device=xyz.device)
    offers = 0
    for dy in range(-s, s + 1):
        for dx in range(-s, s + 1):
            qx, qy = px + dx, py + dy
            m = ok & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            keys.scatter_reduce_(0, (qy * W + qx)[m], key[m], "amin", include_self=True)
            if count:
                offers = offers + m.sum()
    return torch.where(keys == EMPTY, torch.full_like(keys, -1), keys).view(H, W), offers


def run(N, width, height, repeats, torch_repeats):
    xyz = make_ball(N, 7)
    cam = Camera.look_at((0, 0, -3), (0, 0, 0), (0, -1, 0), 45.0, width, height)
    res = dict(points=N, width=width, height=height, repeats=repeats, xyz_bytes=12 * N, keys_bytes=8 * width * height)
    timed = lambda fn, n=repeats: stat([event(fn)[1] for _ in range(n + 2)][2:])
    for s in (0, 1, 2):
        ours = ops.view_splat(xyz, cam, s)
        theirs, offers = torch_splat(xyz, cam, s, count=True)
        equal = bool(torch.equal(ours, theirs))
        r = dict(torch_keys_equal=equal, pixels_differing=int((ours != theirs).sum()), filled=round(float((ours != -1).float().mean()), 4),
                 offers_max_atomics=int(offers))
        del theirs
        r["native_ms"] = timed(lambda: ops.view_splat(xyz, cam, s))
        r["xyz_gb_per_s"] = round(12 * N / (r["native_ms"]["median"] * 1e6), 1)
        r["alternating"] = pair(*alternate(lambda: ops.view_splat(xyz, cam, s), lambda: torch_splat(xyz, cam, s), event, torch_repeats))
        res[f"splat_s{s}"] = r
    keys = ops.view_splat(xyz, cam, 1)
    g = torch.Generator().manual_seed(3)
    for P in (1, 1024):
        pix = torch.stack([torch.randint(0, width, (P,), generator=g), torch.randint(0, height, (P,), generator=g)], 1).to(torch.int32).cuda()
        res[f"pick_{P}_ms"] = timed(lambda: ops.view_pick(keys, pix, 2))
    Wd = ops.mask_words(N)
    for K in (3, 256):
        bits = torch.randint(-2 ** 62, 2 ** 62, (K, Wd), dtype=torch.int64, device="cuda")
        res[f"paint_ids_K{K}_ms"] = timed(lambda: ops.view_paint_ids(keys, bits, N))
        del bits
    res["lift_bits_K1_ms"] = timed(lambda: ops.view_lift_bits(xyz, cam, keys, None, 0.05))
    img = (torch.rand(8, height, width, device="cuda") < 0.5).to(torch.uint8)
    res["lift_bits_K8_ms"] = timed(lambda: ops.view_lift_bits(xyz, cam, keys, img, 0.05))
    res["visible_fraction"] = round(float(ops.view_lift_bits(xyz, cam, keys, None, 0.05)[1][0]) / N, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1000000,10000000")
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=960)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--torch-repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("views_bench: needs a GPU (a timing taken elsewhere says nothing)")
    out = []
    for N in (int(m) for m in args.points.split(",")):
        res = run(N, args.width, args.height, args.repeats, args.torch_repeats)
        print(json.dumps(res), flush=True)
        out.append(res)
        torch.cuda.empty_cache()
        if args.out:                                       # after every configuration: a run that is cut short keeps what it measured
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
