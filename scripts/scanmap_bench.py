"""Times the scan map (csrc/scanmap.hip through point_sam_amd/scanmap.py) next to the torch-composed form of the same definition.

    python scripts/scanmap_bench.py [--points 1000000 10000000] [--voxel-size 0.0078125] [--max-voxels 1048576] [--repeats 10] [--torch-repeats 3]
                                    [--out FILE.json] [--readme FILE.md]

One process, one GPU.  A scan is synthetic and in raster order, as a depth camera or a spinning LiDAR delivers it: a W x W grid over [-0.9, 0.9]^2 lifted
onto a rolling surface, so consecutive points often share a voxel; colours in [-1, 1], labels in -1 .. 4 by region.  Timed, with device events, two
warm-up rounds and the median of --repeats: one add into an empty map (the clear is outside the timed region), the same add into a half-built map (the
map holds the scan's first half), labels, cloud and locate.

The torch-composed form on the same inputs (what a caller could do without the library): cells and fixed point by elementwise operators, `unique` over
the keys, `index_add_` in int64, a re-`unique` of the concatenated keys to merge with the previous map, and the same for the (voxel, label) pairs.  Its
voxels have no permanent ids (they are the ranks of the sorted keys), so the two are compared per key: counts, sums, winning label and votes must be
equal before anything is timed.  Then the two alternate on the same inputs.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scene_bench import alternate, event, pair, stat  # noqa: E402

from point_sam_amd import ops, scanmap  # noqa: E402


def make_scan(M, seed):
    """-> (xyz [n, 3], rgb [n, 3] f32, labels [n] int32) in raster order, n = floor(sqrt(M))^2."""
    W = int(M ** 0.5)
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = torch.linspace(-0.9, 0.9, W, device="cuda")
    y, x = torch.meshgrid(u, u, indexing="ij")
    z = 0.3 * torch.sin(3.0 * x + 0.1 * seed) * torch.cos(2.0 * y) + 0.002 * torch.randn(W, W, generator=g, device="cuda")
    xyz = torch.stack([x, y, z], -1).reshape(-1, 3).float().contiguous()
    rgb = (torch.rand(W * W, 3, generator=g, device="cuda") * 2 - 1).float().contiguous()
    labels = (((x > 0).int() + 2 * (y > 0).int() + (z > 0.15).int()) - (z < -0.25).int() * 5).clamp_min(-1).reshape(-1).int().contiguous()
    return xyz, rgb, labels


class TorchMap:
    """The torch-composed form: sorted keys [V], sums [V, 7] int64 (count, q, c), pairs: sorted (rank of key << 32 | label) is not stable under a
    merge, so pairs are kept as (key, label, count) rows and re-ranked on read."""

    def __init__(self, inv_h, device="cuda"):
        self.inv_h, self.dev = inv_h, device
        self.keys = torch.empty(0, dtype=torch.int64, device=self.dev)
        self.sums = torch.empty(0, 7, dtype=torch.int64, device=self.dev)
        self.pair_key = torch.empty(0, dtype=torch.int64, device=self.dev)
        self.pair_label = torch.empty(0, dtype=torch.int64, device=self.dev)
        self.pair_count = torch.empty(0, dtype=torch.int64, device=self.dev)

    def add(self, xyz, rgb, labels):
        cell = torch.floor((xyz - (-1.0)) * self.inv_h)
        ok = ((cell >= 0) & (cell < float(1 << 21)) & (xyz >= -1) & (xyz <= 1) & (rgb >= -1) & (rgb <= 1)).all(1)
        idx = torch.nonzero(ok)[:, 0]
        c = cell[idx].long()
        key = c[:, 0] | (c[:, 1] << 21) | (c[:, 2] << 42)
        q = torch.floor(xyz[idx].double() * 1048576.0).long() + (1 << 20)
        cq = torch.floor(rgb[idx].double() * 1048576.0).long() + (1 << 20)
        allk, inv = torch.unique(torch.cat([self.keys, key]), return_inverse=True)      # the merge: a re-unique of old and new keys
        V0 = self.keys.numel()
        sums = torch.zeros(allk.numel(), 7, dtype=torch.int64, device=self.dev)
        sums.index_add_(0, inv[:V0], self.sums)
        sums.index_add_(0, inv[V0:], torch.cat([torch.ones(idx.numel(), 1, dtype=torch.int64, device=self.dev), q, cq], 1))
        self.keys, self.sums = allk, sums
        lab = labels[idx].long()
        has = lab >= 0
        # distinct (key, label) pairs: rank the keys (they fit 63 bits, a label 31: no single word holds both)
        rank = inv[V0:][has]
        pk, pn = torch.unique((rank << 32) | lab[has], return_counts=True)
        old_rank = torch.searchsorted(allk, self.pair_key)
        allp, pinv = torch.unique(torch.cat([(old_rank << 32) | self.pair_label, pk]), return_inverse=True)
        count = torch.zeros(allp.numel(), dtype=torch.int64, device=self.dev)
        count.index_add_(0, pinv, torch.cat([self.pair_count, pn]))
        self.pair_key, self.pair_label, self.pair_count = allk[allp >> 32], allp & 0xffffffff, count

    def labels(self):
        """-> (label [V], votes [V]) in the order of the sorted keys: the highest count, ties to the lower label."""
        V = self.keys.numel()
        rank = torch.searchsorted(self.keys, self.pair_key)
        score = (self.pair_count << 32) | (0xffffffff - self.pair_label)
        best = torch.zeros(V, dtype=torch.int64, device=self.dev).scatter_reduce_(0, rank, score, "amax", include_self=True)
        votes = best >> 32
        return torch.where(votes > 0, 0xffffffff - (best & 0xffffffff), torch.full_like(best, -1)).int(), votes.int()


def compare(m, t):
    """The device map against the torch-composed one, per key."""
    order = torch.argsort(m.keys())
    sq, sc = m.sums()
    label, votes = m.labels()
    tl, tv = t.labels()
    return dict(keys=bool(torch.equal(m.keys()[order], t.keys)), count=bool(torch.equal(m.counts()[order].long(), t.sums[:, 0])),
                sums=bool(torch.equal(torch.cat([sq, sc], 1)[order], t.sums[:, 1:])), label=bool(torch.equal(label[order], tl)),
                votes=bool(torch.equal(votes[order], tv)))


def run_size(M, args):
    inv_h = float(ops.map_inv_h(args.voxel_size))
    xyz, rgb, labels = make_scan(M, 1)
    n = xyz.shape[0]
    half = n // 2
    m = scanmap.ScanMap(args.voxel_size, args.max_voxels)

    def fresh_torch(built):
        t = TorchMap(inv_h)
        if built:
            t.add(xyz[:half], rgb[:half], labels[:half])
        return t

    def fresh(built):
        m.clear()
        if built:
            m.add(xyz[:half], rgb[:half], labels[:half])

    res = dict(points=n, voxel_size=args.voxel_size, max_voxels=args.max_voxels)
    for built in (False, True):
        fresh(built)
        m.add(xyz, rgb, labels)
        t = fresh_torch(built)
        t.add(xyz, rgb, labels)
        equal = compare(m, t)
        assert all(equal.values()), f"native and torch-composed maps disagree: {equal}"
        res["equal_" + ("half_built" if built else "empty")] = equal
    res["voxels"] = m.num_voxels
    print(json.dumps(res), flush=True)

    def timed_add(built):
        times = []
        for _ in range(args.repeats + 2):
            fresh(built)
            torch.cuda.synchronize()
            times.append(event(lambda: m.add(xyz, rgb, labels))[1])
        return stat(times[2:])

    res["add_empty_ms"] = timed_add(False)
    res["add_half_built_ms"] = timed_add(True)
    timed = lambda fn: stat([event(fn)[1] for _ in range(args.repeats + 2)][2:])
    res["labels_ms"] = timed(m.labels)
    res["cloud_ms"] = timed(m.cloud)
    res["locate_ms"] = timed(lambda: m.locate(xyz))
    res["clear_ms"] = timed(m.clear)
    # what an add must move at least: positions, colours and labels in, ids out -- against a device copy of as many bytes
    res["add_bytes"] = n * (12 + 12 + 4 + 4)
    src = torch.empty(res["add_bytes"] // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    res["copy_ms"] = timed(lambda: dst.copy_(src))
    del src, dst

    def native(built):
        fresh(built)
        m.add(xyz, rgb, labels)

    def composed(built):
        fresh_torch(built).add(xyz, rgb, labels)

    for built in (False, True):
        # both sides rebuild their starting state inside the timed region: for the half-built case that is one more add of half the scan each
        res["alternating_" + ("half_built" if built else "empty")] = pair(*alternate(lambda: native(built), lambda: composed(built), event, args.torch_repeats))
    return res


def readme(results, args):
    ms = lambda s: f"{s['median']:.3f} [{s['min']:.3f} … {s['max']:.3f}]"
    alt = lambda a: f"{a['native_ms']['median']:.3f} / {a['torch_ms']['median']:.3f} ({a['torch_over_native']:.1f} ×)"
    lines = ["# profiles/scanmap — scan maps", "",
             f"`python scripts/scanmap_bench.py --points {' '.join(str(p) for p in args.points)} --voxel-size {args.voxel_size} --max-voxels {args.max_voxels} "
             f"--repeats {args.repeats} --torch-repeats {args.torch_repeats}`: one MI355X (gfx950), one process, torch {torch.__version__}.  Device-event times "
             "in ms, `median [min … max]` after two warm-up rounds.  A scan is synthetic and in raster order (scripts/scanmap_bench.py).  The torch-composed "
             "form (`unique`, `index_add_` in int64, a re-`unique` to merge) gave **the same** keys, counts, sums, labels and votes before anything was "
             "timed.  The accumulate pass is the run form (a run of equal voxels on consecutive lanes is summed in the wave before its seven atomics); "
             "the plain form, one thread and seven 64-bit atomics per point, measured slower and was removed -- both sets of figures are in DESIGN.md "
             "4.17.  No default was tuned on real scans or a trained checkpoint.  These are records, not gates.", ""]
    head = "| | " + " | ".join(f"{r['points']} points" for r in results) + " |"
    lines += [head, "|---|" + "---|" * len(results)]
    row = lambda name, f: lines.append(f"| {name} | " + " | ".join(f(r) for r in results) + " |")
    row("voxels of the map after the add", lambda r: str(r["voxels"]))
    row("`add` into an empty map (six launches, one host read)", lambda r: ms(r["add_empty_ms"]))
    row("`add` into a half-built map", lambda r: ms(r["add_half_built_ms"]))
    row("a device copy of the add's bytes (32 per point, half in, half out)", lambda r: ms(r["copy_ms"]))
    row("`labels`", lambda r: ms(r["labels_ms"]))
    row("`cloud`", lambda r: ms(r["cloud_ms"]))
    row("`locate` of the scan", lambda r: ms(r["locate_ms"]))
    row("`clear`", lambda r: ms(r["clear_ms"]))
    row("empty map, alternating: native / torch-composed (clear + add each)", lambda r: alt(r["alternating_empty"]))
    row("half-built map, alternating: native / torch-composed (rebuild + add each)", lambda r: alt(r["alternating_half_built"]))
    return "\n".join(lines + [""])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--voxel-size", type=float, default=2.0 ** -7)
    ap.add_argument("--max-voxels", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--torch-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--readme", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scanmap_bench: needs a GPU (a timing taken elsewhere says nothing)")
    results = [run_size(M, args) for M in args.points]
    print(json.dumps(results), flush=True)
    for path, text in ((args.out, json.dumps(results, indent=1)), (args.readme, readme(results, args))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
