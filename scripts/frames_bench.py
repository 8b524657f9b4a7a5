"""Times the RGB-D frame kernels (csrc/frames.hip: ops.frames_unproject + ops.frames_finish) next to the torch-composed form of the same definition.

    python scripts/frames_bench.py [--frames 64] [--width 640] [--height 480] [--repeats 20] [--torch-repeats 5] [--out FILE.json] [--readme FILE.md]

One process, one GPU.  The frames: a seeded synthetic room per frame (a far wall, boxes at several depths, millimetre noise, 3 % invalid pixels), uint8
colour, cameras on a circle looking inwards; edge = 0.05.  Both depth formats are run.  The torch-composed form: masks and four shifted compares for the
predicate, `cumsum` for the index, `nonzero` for the kept pixels, gathers of the depth, colour and camera rows, the unprojection and normalisation as
elementwise fp32 operators with every divisor a device tensor (a Python scalar divisor is multiplied by its reciprocal, which is not the IEEE
division the definition asks for), a scatter for the keys.  Its outputs are compared with ours first and must be equal in every bit; the two are then
timed ALTERNATING on the same inputs, device-event times, median with min and max.  Both forms read M back once.

With the times: the bytes the two calls must move at least and the fraction of the HBM rate that is (8.0 TB/s specified, about 6.3 TB/s reached by a
plain copy).  --readme writes the table to a markdown file (the first table of profiles/frames/README.md is one run of this).
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

from point_sam_amd import ops  # noqa: E402
from point_sam_amd.views import Camera  # noqa: E402

HBM_SPEC, HBM_COPY = 8.0e12, 6.3e12


def make_frames(F, H, W, seed):
    """-> (depth [F, H, W] f32 on the device, rgb [F, H, W, 3] uint8, cameras, far)."""
    g = torch.Generator().manual_seed(seed)
    depth = torch.full((F, H, W), 4.0)
    for f in range(F):
        for _ in range(6):
            y0, x0 = int(torch.randint(0, H - H // 4, (1,), generator=g)), int(torch.randint(0, W - W // 4, (1,), generator=g))
            depth[f, y0:y0 + H // 4, x0:x0 + W // 4] = 1.0 + 2.5 * float(torch.rand(1, generator=g))
    depth += 0.002 * torch.randn(F, H, W, generator=g)
    depth[torch.rand(F, H, W, generator=g) < 0.03] = 0.0
    rgb = torch.randint(0, 256, (F, H, W, 3), generator=g, dtype=torch.uint8)
    cams = []
    for f in range(F):
        a = 2 * math.pi * f / F
        cams.append(Camera.look_at((3 * math.cos(a), 0.3, 3 * math.sin(a)), (0, 0, 0), (0, -1, 0), 50.0, W, H, near=0.1))
    return depth.cuda().contiguous(), rgb.cuda().contiguous(), cams, 8.0


def torch_frames(depth, rgb, table, edge, depth_scale, center, scale, nposes):
    """The definition composed from torch operators -> (xyz [M, 3] normalised, rgb [M, 3], index [F, H, W] int32, keys [F, H, W] int64, M)."""
    F, H, W = depth.shape
    dev = depth.device
    if depth.dtype == torch.uint16:
        d = (depth.view(torch.int16).to(torch.int32) & 0xFFFF).to(torch.float32) * depth_scale
    else:
        d = depth
    near, far = table[:, 16].view(F, 1, 1), table[:, 17].view(F, 1, 1)
    valid = torch.isfinite(d) & (d >= near) & (d <= far)
    limit = d * edge
    drop = torch.zeros_like(valid)
    drop[:, :, 1:] |= valid[:, :, :-1] & ((d[:, :, 1:] - d[:, :, :-1]).abs() > limit[:, :, 1:])
    drop[:, :, :-1] |= valid[:, :, 1:] & ((d[:, :, :-1] - d[:, :, 1:]).abs() > limit[:, :, :-1])
    drop[:, 1:] |= valid[:, :-1] & ((d[:, 1:] - d[:, :-1]).abs() > limit[:, 1:])
    drop[:, :-1] |= valid[:, 1:] & ((d[:, :-1] - d[:, 1:]).abs() > limit[:, :-1])
    keep = (valid & ~drop).reshape(-1)
    rank = torch.cumsum(keep, 0, dtype=torch.int32) - 1
    index = torch.where(keep, rank, torch.full_like(rank, -1)).view(F, H, W)
    sel = torch.nonzero(keep)[:, 0]
    M = sel.numel()                                        # the host read
    f = sel // (H * W)
    r = sel - f * (H * W)
    y = r // W
    x = r - y * W
    cam = table.index_select(0, f)                         # [M, 18]
    dk = d.reshape(-1).index_select(0, sel)
    a = ((x.to(torch.float32) + 0.5) - cam[:, 14]) / cam[:, 12]
    b = ((y.to(torch.float32) + 0.5) - cam[:, 15]) / cam[:, 13]
    q = (a * dk - cam[:, 3], b * dk - cam[:, 7], dk - cam[:, 11])
    p = torch.stack([(cam[:, j] * q[0] + cam[:, 4 + j] * q[1]) + cam[:, 8 + j] * q[2] for j in range(3)], 1)
    xyz = (p - center) / scale
    if rgb.dtype == torch.uint8:
        col = (rgb.view(-1, 3).index_select(0, sel).to(torch.float32) / torch.full((), 255.0, device=dev) - 0.5) / torch.full((), 0.5, device=dev)
    else:
        col = rgb.view(-1, 3).index_select(0, sel)
    P = nposes.index_select(0, f)
    z = ((P[:, 8] * xyz[:, 0] + P[:, 9] * xyz[:, 1]) + P[:, 10] * xyz[:, 2]) + P[:, 11]
    key = (z.view(torch.int32).to(torch.int64) << 32) | torch.arange(M, dtype=torch.int64, device=dev)
    key = torch.where(torch.isfinite(z) & (z > 0), key, torch.full_like(key, -1))
    keys = torch.full((F * H * W,), -1, dtype=torch.int64, device=dev)
    keys[sel] = key
    return xyz, col, index, keys.view(F, H, W), M


def run(F, H, W, repeats, torch_repeats, u16):
    depth, rgb, cams, far = make_frames(F, H, W, 11)
    depth_scale = None
    if u16:
        depth_scale = 0.001
        depth = torch.from_numpy(np.clip(np.round(depth.cpu().numpy() * 1000.0), 0, 65535).astype(np.uint16)).cuda()      # millimetres
    edge = 0.05
    world, col, index, M = ops.frames_unproject(depth, rgb, cams, far, edge, depth_scale)
    center = world.double().mean(0).float()
    scale = ((world.double() - center.double()) ** 2).sum(1).max().sqrt().float()
    c_host, s_host = center.cpu().numpy(), float(scale)
    xyz, keys, ncams = ops.frames_finish(world, index, cams, c_host, s_host)
    table = torch.tensor([[float(v) for v in c.pose_words] + [c.fx, c.fy, c.cx, c.cy, c.near, float(np.float32(far))] for c in cams], dtype=torch.float32).cuda()
    nposes = torch.from_numpy(np.stack([c.pose_words for c in ncams])).cuda()
    composed = lambda: torch_frames(depth, rgb, table, edge, depth_scale, center, scale, nposes)
    t_xyz, t_col, t_index, t_keys, t_M = composed()
    words = lambda t: t.view(torch.int32)
    equal = dict(M=t_M == M, xyz=bool(torch.equal(words(t_xyz), words(xyz))), rgb=bool(torch.equal(words(t_col), words(col))),
                 index=bool(torch.equal(t_index, index)), keys=bool(torch.equal(t_keys, keys)))
    assert all(equal.values()), f"native and torch-composed frames disagree: {equal}"
    del t_xyz, t_col, t_index, t_keys

    def native():
        w, c, i, m = ops.frames_unproject(depth, rgb, cams, far, edge, depth_scale)
        return ops.frames_finish(w, i, cams, c_host, s_host)

    N = F * H * W
    unproject_bytes = N * ((2 if u16 else 4) + 3 + 4) + M * 24            # depth and colour in, index out; xyz and rgb of the kept pixels out
    finish_bytes = M * 24 + N * 4 + M * 12 + N * 8                        # normalise in place; index and the pixel's point in, keys out
    res = dict(frames=F, height=H, width=W, pixels=N, depth="uint16" if u16 else "float32", kept=M, kept_fraction=round(M / N, 4), equal=equal,
               unproject_bytes=unproject_bytes, finish_bytes=finish_bytes)
    timed = lambda fn: stat([event(fn)[1] for _ in range(repeats + 2)][2:])
    res["unproject_ms"] = timed(lambda: ops.frames_unproject(depth, rgb, cams, far, edge, depth_scale))
    w, _, i, _ = ops.frames_unproject(depth, rgb, cams, far, edge, depth_scale)
    res["finish_ms"] = timed(lambda: ops.frames_finish(w, i, cams, c_host, 1.0))      # scale 1: repeated in-place normalisation stays finite
    res["both_ms"] = timed(native)
    total = unproject_bytes + finish_bytes
    res["both_gb_per_s"] = round(total / (res["both_ms"]["median"] * 1e6), 1)
    res["hbm_fraction_of_spec"] = round(total / (res["both_ms"]["median"] * 1e-3) / HBM_SPEC, 4)
    res["hbm_fraction_of_copy"] = round(total / (res["both_ms"]["median"] * 1e-3) / HBM_COPY, 4)
    res["alternating"] = pair(*alternate(native, composed, event, torch_repeats))
    return res


def readme(results, args):
    ms = lambda s: f"{s['median']:.3f} [{s['min']:.3f} … {s['max']:.3f}]"
    lines = ["# profiles/frames — RGB-D frames: unproject + finish", "",
             f"`python scripts/frames_bench.py --frames {args.frames} --width {args.width} --height {args.height} --repeats {args.repeats} "
             f"--torch-repeats {args.torch_repeats}`: one MI355X (gfx950), one process, torch {torch.__version__}.  Device-event times in ms, "
             "`median [min … max]` after two warm-up rounds.  Every number in the table is measured by this one run of the script; the byte counts are "
             "what the two calls must move at least (depth, colour and index per pixel, 24 B of xyz and rgb per kept pixel, the normalisation in place, "
             "index and the pixel's point in and 8 B of key out).  The torch-composed form (scripts/frames_bench.py: masks, `cumsum`, `nonzero`, gathers, "
             "elementwise fp32 operators, a scatter) gave **the same bits** in xyz, rgb, index, keys and M before anything was timed.  The repetitions run "
             "back to back on the same buffers, so part of the input may be served by the 256 MB Infinity Cache rather than by HBM: the HBM fraction is "
             "the bytes over the time, not a counter reading.  These are records, not gates.", "",
             "| | " + " | ".join(f"{r['depth']} depth" for r in results) + " |", "|---|" + "---|" * len(results)]
    row = lambda name, fn: lines.append(f"| {name} | " + " | ".join(fn(r) for r in results) + " |")
    row("frames × height × width", lambda r: f"{r['frames']} × {r['height']} × {r['width']} = {r['pixels']} pixels")
    row("kept pixels M (edge = 0.05)", lambda r: f"{r['kept']} ({100 * r['kept_fraction']:.1f} %)")
    row("bytes, unproject / finish", lambda r: f"{r['unproject_bytes'] / 1e6:.0f} MB / {r['finish_bytes'] / 1e6:.0f} MB")
    row("`ops.frames_unproject` (three launches, one host read)", lambda r: ms(r["unproject_ms"]))
    row("`ops.frames_finish` (two launches)", lambda r: ms(r["finish_ms"]))
    row("both calls", lambda r: ms(r["both_ms"]))
    row("bytes / time of both calls", lambda r: f"{r['both_gb_per_s'] / 1e3:.2f} TB/s")
    row("fraction of the HBM rate: of 8.0 TB/s specified / of 6.3 TB/s copied", lambda r: f"{100 * r['hbm_fraction_of_spec']:.0f} % / {100 * r['hbm_fraction_of_copy']:.0f} %")
    row("alternating: native / torch-composed", lambda r: f"{r['alternating']['native_ms']['median']:.3f} / {r['alternating']['torch_ms']['median']:.3f} "
                                                          f"({r['alternating']['torch_over_native']:.1f} ×)")
    lines += ["", "The times of the two calls include their host work: the camera table built and copied per call, the allocation of the outputs at capacity, "
              "and in `frames_unproject` the read of M, which waits for the three launches.  Not measured: frames larger than these, a kept fraction far from "
              "this one, fp32 colour, and the kernels alone without the host work around them.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--torch-repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--readme", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frames_bench: needs a GPU (a timing taken elsewhere says nothing)")
    out = []
    for u16 in (False, True):
        res = run(args.frames, args.height, args.width, args.repeats, args.torch_repeats, u16)
        print(json.dumps(res), flush=True)
        out.append(res)
        torch.cuda.empty_cache()
        for path, text in ((args.out, json.dumps(out, indent=1)), (args.readme, readme(out, args))):
            if path:                                       # after every configuration: a run that is cut short keeps what it measured
                os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
                with open(path, "w") as f:
                    f.write(text)


if __name__ == "__main__":
    main()
