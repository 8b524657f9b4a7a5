"""Times scan map views (csrc/map_view.hip through ops.map_view) and, for orientation, the only way to look at a map without them: point splats of its cloud.

    python scripts/map_view_bench.py [--points 4000000] [--voxel-sizes 0.0078125 0.00390625] [--sizes 640x480 1920x1080] [--max-voxels 4194304]
                                     [--repeats 10] [--out FILE.json] [--readme FILE.md]

One process, one GPU.  The map is carve_bench.py's room seen from inside in raster order -- the walls, floor and ceiling of [-0.9, 0.9]^3 plus a box
standing in it -- added once per voxel size.  The camera stands at carve_bench.py's origin and looks at the box's far corner, 70 degrees of vertical
field of view.  Timed with device events, two warm-up rounds and the median of --repeats: one ops.map_view (the clear of the brick bitmap, the launch
over the voxel ids and the launch over the pixels; the workspace's allocation is inside the call) in its three forms -- as shipped, with the bitmap
read from global memory where the shipped form stages it into LDS (PSAM_MAP_VIEW_NO_LDS), and without the brick gate (PSAM_MAP_VIEW_NO_GATE) -- whose
keys must be equal words before anything is timed.  The visited cells and the table lookups come from the call's own counters (a separate, untimed
call).

For orientation only: ops.map_cloud + ops.view_splat at splat 1 and 2 on the same map and camera, the parent path.  It draws another picture, so
beside its time stands the share of the ray cast's non-empty pixels (the room's silhouette from inside: every pixel) that the splats leave empty.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from carve_bench import ORIGIN, make_room  # noqa: E402
from scene_bench import event, stat  # noqa: E402

from point_sam_amd import ops, scanmap  # noqa: E402
from point_sam_amd.views import Camera  # noqa: E402

TARGET = (0.6, 0.5, -0.2)
FORMS = (("shipped", 0), ("bitmap from global memory", ops.MAP_VIEW_NO_LDS), ("no brick gate", ops.MAP_VIEW_NO_GATE))


def run(voxel_size, size, scan, args):
    width, height = size
    m = scanmap.ScanMap(voxel_size, args.max_voxels)
    m.add(scan, torch.zeros_like(scan))
    V = m.num_voxels
    cam = Camera.look_at(ORIGIN, TARGET, (0.0, 0.0, 1.0), 70.0, width, height)
    lead = (m._block, m.max_voxels, m.max_pairs, V, cam)
    view = lambda flags, stats=None: ops.map_view(*lead, voxel_size=voxel_size, flags=flags, stats=stats)
    res = dict(voxel_size=voxel_size, width=width, height=height, voxels=V, workspace_bytes=ops._lib.load().psam_mapview_ws_bytes(float(ops.map_inv_h(voxel_size))))
    keys = view(0)
    counters = {}
    for name, flags in FORMS:
        stats = torch.zeros(2, dtype=torch.int64, device="cuda")
        assert torch.equal(view(flags, stats), keys), f"the form '{name}' changes the keys"
        counters[name] = stats.tolist()
    res["visited_cells"], res["lookups"], res["lookups_without_gate"] = counters["shipped"][0], counters["shipped"][1], counters["no brick gate"][1]
    res["hit_pixels"] = int((keys != -1).sum())
    timed = lambda fn: stat([event(fn)[1] for _ in range(args.repeats + 2)][2:])
    res["forms_ms"] = {name: timed(lambda: view(flags)) for name, flags in FORMS}
    best = res["forms_ms"]["shipped"]["median"] * 1e-3
    res["visited_cells_per_s"], res["lookups_per_s"] = round(res["visited_cells"] / best), round(res["lookups"] / best)
    xyz = m.cloud()[0]
    res["cloud_ms"] = timed(lambda: ops.map_cloud(m._block, m.max_voxels, m.max_pairs, V))
    res["splat"] = {}
    for s in (1, 2):
        drawn = ops.view_splat(xyz, cam, s)
        holes = int(((drawn == -1) & (keys != -1)).sum())
        res["splat"][s] = dict(ms=timed(lambda: ops.view_splat(xyz, cam, s)), empty_inside_silhouette=round(holes / max(res["hit_pixels"], 1), 4))
    print(json.dumps(res), flush=True)
    return res


def readme(results, args):
    ms = lambda s: f"{s['median']:.3f} [{s['min']:.3f} … {s['max']:.3f}]"
    lines = ["# profiles/map_view — scan map views", "",
             f"`python scripts/map_view_bench.py --points {args.points} --voxel-sizes {' '.join(str(v) for v in args.voxel_sizes)} --sizes {' '.join(args.sizes)} "
             f"--max-voxels {args.max_voxels} --repeats {args.repeats}`: one MI355X (gfx950), one process, torch {torch.__version__}.  Device-event times in ms, "
             "`median [min … max]` after two warm-up rounds.  The map is the synthetic room of scripts/carve_bench.py with a box standing in it, the camera "
             "stands inside and looks at the box.  One `ops.map_view` is the clear of the brick bitmap, the launch over the voxel ids, the launch over the "
             "pixels and the allocation of the workspace.  The three forms gave **equal keys** before anything was timed.  The splat rows are the parent "
             "path (`ops.map_cloud` + `ops.view_splat`), for orientation: it draws another picture.  These are records, not gates.", ""]
    head = "| | " + " | ".join(f"h = {r['voxel_size']}, {r['width']} × {r['height']}" for r in results) + " |"
    lines += [head, "|---|" + "---|" * len(results)]
    row = lambda name, f: lines.append(f"| {name} | " + " | ".join(f(r) for r in results) + " |")
    row("voxels of the map", lambda r: str(r["voxels"]))
    row("bitmap (workspace) bytes", lambda r: str(r["workspace_bytes"]))
    row("pixels that hit a voxel", lambda r: f"{r['hit_pixels']} of {r['width'] * r['height']}")
    row("visited cells", lambda r: str(r["visited_cells"]))
    row("table lookups behind the gate / without it", lambda r: f"{r['lookups']} / {r['lookups_without_gate']}")
    for name, _ in FORMS:
        row(f"`map_view`, {name}", lambda r, name=name: ms(r["forms_ms"][name]))
    row("visited cells per second (shipped)", lambda r: f"{r['visited_cells_per_s']:.3e}")
    row("lookups per second (shipped)", lambda r: f"{r['lookups_per_s']:.3e}")
    row("`map_cloud`", lambda r: ms(r["cloud_ms"]))
    for s in (1, 2):
        row(f"`view_splat`, splat {s}", lambda r, s=s: ms(r["splat"][s]["ms"]))
        row(f"splat {s}: empty pixels inside the silhouette", lambda r, s=s: f"{100 * r['splat'][s]['empty_inside_silhouette']:.1f} %")
    return "\n".join(lines + [""])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=4000000)
    ap.add_argument("--voxel-sizes", type=float, nargs="+", default=[2.0 ** -7, 2.0 ** -8])
    ap.add_argument("--sizes", nargs="+", default=["640x480", "1920x1080"])
    ap.add_argument("--max-voxels", type=int, default=1 << 22)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--readme", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("map_view_bench: needs a GPU (a timing taken elsewhere says nothing)")
    scan = make_room(args.points, 2, box=True)
    results = [run(h, tuple(int(v) for v in size.split("x")), scan, args) for h in args.voxel_sizes for size in args.sizes]
    for path, text in ((args.out, json.dumps(results, indent=1)), (args.readme, readme(results, args))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
