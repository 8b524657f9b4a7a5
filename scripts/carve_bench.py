"""Times scan map carving (csrc/carve.hip through ScanMap.carve) next to the torch-composed form of the same definition.

    python scripts/carve_bench.py [--points 1000000 10000000] [--voxel-size 0.0078125] [--max-voxels 1048576] [--margin 1] [--repeats 10]
                                  [--torch-repeats 3] [--out FILE.json] [--readme FILE.md]

One process, one GPU.  A scan is a room seen from inside, in raster order as a spinning LiDAR or a panoramic depth camera delivers it: a W x W grid over
azimuth and elevation from an origin off the room's middle, every ray ending on a wall, the floor or the ceiling of [-0.9, 0.9]^3 (plus millimetre
noise).  The map is built first from that scan and from a second one that also holds a box standing in the room, so the carve has ghosts to see
through.  Timed, with device events, two warm-up rounds and the median of --repeats: one carve of the scan (four launches and the 64-byte host read);
every repeat carries a new stamp, so every repeat does all of the work.

The torch-composed form on the same inputs (what a caller could do without the library): cells by elementwise operators, `unique` over the keys for
the rays, then all rays advance one crossing per iteration -- the six products compared as tensors, a `searchsorted` of the crossed cells' keys in the
map's sorted keys, the hit / missed rules by masked index writes -- until every ray is within the margin of its end.  Its hits and misses per voxel
and its count of crossed cells must equal the library's before anything is timed.  Then the two alternate on the same inputs.

Form (a) of the walk, one thread per ray, is what the library builds; form (b), threads over fixed chunks of crossings, is not built and not timed.
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scene_bench import alternate, event, pair, stat  # noqa: E402

from point_sam_amd import ops, scanmap  # noqa: E402

ORIGIN = (0.15, -0.25, -0.3)
WALL = 0.9


def make_room(M, seed, box=False):
    """-> xyz [n, 3] f32 in raster order, n = floor(sqrt(M))^2: where the ray of each (elevation, azimuth) from ORIGIN first meets the room (and the box)."""
    W = int(M ** 0.5)
    g = torch.Generator(device="cuda").manual_seed(seed)
    az = torch.linspace(-math.pi, math.pi, W + 1, device="cuda", dtype=torch.float64)[:-1]
    el = torch.linspace(-1.45, 1.45, W, device="cuda", dtype=torch.float64)
    e, a = torch.meshgrid(el, az, indexing="ij")
    d = torch.stack([torch.cos(e) * torch.cos(a), torch.cos(e) * torch.sin(a), torch.sin(e)], -1).reshape(-1, 3)
    o = torch.tensor(ORIGIN, dtype=torch.float64, device="cuda")

    def slab(lo, hi):
        """entry and exit parameters of every ray against the box [lo, hi]"""
        with torch.no_grad():
            t0, t1 = (lo - o) / d, (hi - o) / d
        return torch.minimum(t0, t1).amax(1), torch.maximum(t0, t1).amin(1)
    t = slab(torch.full((3,), -WALL, dtype=torch.float64, device="cuda"), torch.full((3,), WALL, dtype=torch.float64, device="cuda"))[1]      # from inside: the exit
    if box:
        near, far = slab(torch.tensor([0.3, 0.2, -WALL], dtype=torch.float64, device="cuda"), torch.tensor([0.6, 0.5, -0.2], dtype=torch.float64, device="cuda"))
        t = torch.where((near < far) & (near > 0), torch.minimum(t, near), t)
    xyz = o + t[:, None] * d + 0.001 * torch.randn(W * W, 3, generator=g, device="cuda", dtype=torch.float64)
    return xyz.clamp(-0.95, 0.95).float().contiguous()


def cells_of(xyz, inv_h):
    """-> (cell [M, 3] int64, ok [M]): a map point's cell and acceptance test, without a pose."""
    cell = torch.floor((xyz - (-1.0)) * inv_h)
    ok = ((cell >= 0) & (cell < float(1 << 21)) & (xyz >= -1) & (xyz <= 1)).all(1)
    return cell.long(), ok


def key_of(cell):
    return cell[:, 0] | (cell[:, 1] << 21) | (cell[:, 2] << 42)


class TorchCarve:
    """The torch-composed form over the map's keys (id -> key): four int64 vectors per voxel id."""

    def __init__(self, map_keys, inv_h):
        self.inv_h = inv_h
        self.sorted, self.order = torch.sort(map_keys)
        V = map_keys.numel()
        self.hits, self.misses, self.last_hit, self.last_missed = (torch.zeros(V, dtype=torch.int64, device=map_keys.device) for _ in range(4))
        self.carves = 0

    def find(self, key):
        """-> (ids of the keys the map holds, the mask of those keys)"""
        pos = torch.searchsorted(self.sorted, key).clamp_max(self.sorted.numel() - 1)
        found = self.sorted[pos] == key
        return self.order[pos[found]], found

    def carve(self, xyz, origin, margin):
        """-> crossed cells beyond the margin, summed over the rays"""
        self.carves += 1
        stamp = self.carves
        cell, ok = cells_of(xyz, self.inv_h)
        ends = torch.unique(key_of(cell[ok]))
        v, _ = self.find(ends)
        v = v[self.last_hit[v] < stamp]
        self.hits[v] += 1
        self.last_hit[v] = stamp
        o = cells_of(torch.tensor([origin], dtype=torch.float32, device=xyz.device), self.inv_h)[0][0]
        ends = ends[ends != key_of(o[None])[0]]
        e = torch.stack([ends & 0x1fffff, (ends >> 21) & 0x1fffff, ends >> 42], 1)
        n, s = (e - o).abs(), torch.sign(e - o)
        k, cur = torch.zeros_like(n), o.expand_as(n).clone()
        crossed = 0
        while n.numel():
            A = 2 * k + 1
            # t_a <= t_b as (2 k_a + 1) n_b <= (2 k_b + 1) n_a: an axis that has arrived or never moves compares above every axis still on its way
            le = lambda a, b: A[:, a] * n[:, b] <= A[:, b] * n[:, a]
            step = torch.stack([le(0, 1) & le(0, 2), le(1, 0) & le(1, 2), le(2, 0) & le(2, 1)], 1).long()
            k, cur = k + step, cur + s * step
            live = (n - k).amax(1) > margin
            n, s, k, cur = n[live], s[live], k[live], cur[live]
            crossed += int(n.shape[0])
            v, _ = self.find(key_of(cur))
            v = torch.unique(v[self.last_hit[v] != stamp])
            v = v[self.last_missed[v] < stamp]
            self.misses[v] += 1
            self.last_missed[v] = stamp
        return crossed


def run_size(M, args):
    inv_h = float(ops.map_inv_h(args.voxel_size))
    scan, first = make_room(M, 1), make_room(M, 2, box=True)
    n = scan.shape[0]
    rgb = torch.zeros_like(scan)
    m = scanmap.ScanMap(args.voxel_size, args.max_voxels)

    def build():
        m.clear()
        m.add(first, rgb)
        m.add(scan, rgb)
    build()
    t = TorchCarve(m.keys(), inv_h)
    res = dict(points=n, voxel_size=args.voxel_size, margin=args.margin, voxels=m.num_voxels)
    for xyz in (first, scan, scan):                                # the box is there once and then seen through twice
        got = m.carve(xyz, ORIGIN, None, args.margin)
        crossed = t.carve(xyz, ORIGIN, args.margin)
        equal = dict(crossed=got.crossed == crossed, hits=bool(torch.equal(m.hits().long(), t.hits)), misses=bool(torch.equal(m.misses().long(), t.misses)),
                     last_hit=bool(torch.equal(m.last_hit().long(), t.last_hit)), last_missed=bool(torch.equal(m.last_missed().long(), t.last_missed)))
        assert all(equal.values()), f"native and torch-composed carves disagree: {equal}"
    res.update(equal=equal, rays=got.rays, crossed=got.crossed, missed_voxels=got.missed_voxels, free_voxels=int((~m.occupied()).sum()))
    print(json.dumps(res), flush=True)

    timed = lambda fn: stat([event(fn)[1] for _ in range(args.repeats + 2)][2:])
    res["carve_ms"] = timed(lambda: m.carve(scan, ORIGIN, None, args.margin))
    res["crossed_per_s"] = round(got.crossed / (res["carve_ms"]["median"] * 1e-3))
    res["occupied_ms"] = timed(m.occupied)
    res["alternating"] = pair(*alternate(lambda: m.carve(scan, ORIGIN, None, args.margin), lambda: t.carve(scan, ORIGIN, args.margin), event, args.torch_repeats))
    return res


def readme(results, args):
    ms = lambda s: f"{s['median']:.3f} [{s['min']:.3f} … {s['max']:.3f}]"
    alt = lambda a: f"{a['native_ms']['median']:.3f} / {a['torch_ms']['median']:.3f} ({a['torch_over_native']:.1f} ×)"
    lines = ["# profiles/carve — scan map carving", "",
             f"`python scripts/carve_bench.py --points {' '.join(str(p) for p in args.points)} --voxel-size {args.voxel_size} --max-voxels {args.max_voxels} "
             f"--margin {args.margin} --repeats {args.repeats} --torch-repeats {args.torch_repeats}`: one MI355X (gfx950), one process, torch {torch.__version__}.  "
             "Device-event times in ms, `median [min … max]` after two warm-up rounds.  A scan is a synthetic room seen from inside, in raster order "
             "(scripts/carve_bench.py); the map was built from it and from a scan with a box in the room.  The torch-composed form (all rays advance one "
             "crossing per iteration by tensor operators, keys found by `searchsorted` in the map's sorted keys) gave **the same** hits, misses, stamps and "
             "count of crossed cells before anything was timed.  The walk is form (a), one thread per ray over a compacted ray list; form (b), threads "
             "over fixed chunks of crossings, is not built, so there is no (a) / (b) comparison here.  These are records, not gates.", ""]
    head = "| | " + " | ".join(f"{r['points']} points" for r in results) + " |"
    lines += [head, "|---|" + "---|" * len(results)]
    row = lambda name, f: lines.append(f"| {name} | " + " | ".join(f(r) for r in results) + " |")
    row("voxels of the map", lambda r: str(r["voxels"]))
    row("rays (distinct end cells)", lambda r: str(r["rays"]))
    row("crossed cells beyond the margin", lambda r: str(r["crossed"]))
    row("voxels voted free after the three carves", lambda r: str(r["free_voxels"]))
    row("`carve` (four launches, one 64-byte host read)", lambda r: ms(r["carve_ms"]))
    row("crossed cells per second", lambda r: f"{r['crossed_per_s']:.3e}")
    row("`occupied`", lambda r: ms(r["occupied_ms"]))
    row("alternating: native / torch-composed", lambda r: alt(r["alternating"]))
    return "\n".join(lines + [""])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--voxel-size", type=float, default=2.0 ** -7)
    ap.add_argument("--max-voxels", type=int, default=1 << 20)
    ap.add_argument("--margin", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--torch-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--readme", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("carve_bench: needs a GPU (a timing taken elsewhere says nothing)")
    results = [run_size(M, args) for M in args.points]
    print(json.dumps(results), flush=True)
    for path, text in ((args.out, json.dumps(results, indent=1)), (args.readme, readme(results, args))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
