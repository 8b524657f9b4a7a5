"""Times the instance-geometry kernels (csrc/geometry.hip) next to the same results composed from torch operators.

    python scripts/geometry_bench.py [--points 131072,4000000] [--masks 256] [--cover 0.01] [--repeats 20] [--out FILE.json]

One process, one GPU, no model.  The scan is scripts/scene_bench.py's synthetic one; mask k is a blob: the `cover` share of the scan nearest to a
random scan point, packed with ops.mask_pack.  Per scan size, native and composed paths ALTERNATE in the same process on the same data after two
warm-up rounds; each figure is the median of `--repeats` device-event times, with min and max.

  moments   ops.mask_moments(xyz, bits, rgb) against: ops.mask_unpack -> bool [rows, N]; count = sum; sums = the fp64 matmul of the mask with the
            [N, 12] fp64 feature columns (x, y, z, xx, .., zz, r, g, b; built once outside the timed region, in the baseline's favour);
            lo / hi = where(mask, xyz, +-inf).amin / amax.  Rows are taken `--chunk-bytes` of boolean-and-float intermediates at a time; the chunk
            size is reported.
  extents   ops.mask_extents(xyz, bits, origin, axes) against: d = xyz - origin per row, p = d @ axes^T, where + amin / amax, r2 = (d d).sum.
  geometry  geometry.mask_geometry end to end (both kernels, the two copies and the host's eigen step), wall clock.

The composed results are compared with the native ones before anything is timed (counts and boxes equal, sums to 1e-12 relative, extents to 1e-5):
faster and different would not be faster."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scene_bench import alternate, event, make_scan, pair, stat  # noqa: E402

from point_sam_amd import geometry, ops  # noqa: E402

HBM_ACHIEVABLE_TBS, HBM_SPEC_TBS = 6.3, 8.0


def make_masks(xyz, K, cover, seed):
    """K blobs of about cover * N points each -> bits [K, W]; 16 rows of distances at a time."""
    N = xyz.shape[0]
    g = torch.Generator().manual_seed(seed)
    centres = xyz[torch.randint(0, N, (K,), generator=g).cuda()]
    W = ops.mask_words(N)
    out = (torch.empty(K, W, dtype=torch.int64, device="cuda"),) + tuple(torch.empty(K, dtype=torch.int32, device="cuda") for _ in range(3))
    want = max(1, int(cover * N))
    for r in range(0, K, 16):
        d = torch.cdist(centres[r:r + 16], xyz)                                   # [16, N]
        thr = d.kthvalue(want, dim=1).values                                      # the blob's radius
        ops.mask_pack((thr[:, None] - d).contiguous(), -1e-30, 0.0, out=out, row=r)
    return out[0], out[1]


def features(xyz, rgb):
    p, c = xyz.double(), rgb.double()
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return torch.stack([x, y, z, x * x, x * y, x * z, y * y, y * z, z * z, c[:, 0], c[:, 1], c[:, 2]], 1).contiguous()


def torch_moments(xyz, bits, feats, chunk):
    K, N = bits.shape[0], xyz.shape[0]
    count = torch.empty(K, dtype=torch.int32, device="cuda")
    sums = torch.empty(K, 12, dtype=torch.float64, device="cuda")
    lo, hi = torch.empty(K, 3, device="cuda"), torch.empty(K, 3, device="cuda")
    inf = torch.full((), float("inf"), device="cuda")
    for r in range(0, K, chunk):
        m = ops.mask_unpack(bits[r:r + chunk], N)
        count[r:r + chunk] = m.sum(1)
        sums[r:r + chunk] = m.double() @ feats
        lo[r:r + chunk] = torch.where(m[:, :, None], xyz[None], inf).amin(1)
        hi[r:r + chunk] = torch.where(m[:, :, None], xyz[None], -inf).amax(1)
    return count, sums, lo, hi


def torch_extents(xyz, bits, origin, axes, chunk):
    K, N = bits.shape[0], xyz.shape[0]
    lo, hi, r2max = torch.empty(K, 3, device="cuda"), torch.empty(K, 3, device="cuda"), torch.empty(K, device="cuda")
    inf = torch.full((), float("inf"), device="cuda")
    for r in range(0, K, chunk):
        m = ops.mask_unpack(bits[r:r + chunk], N)
        d = xyz[None] - origin[r:r + chunk, None]                                 # [rows, N, 3]
        p = torch.einsum("rnj,rij->rni", d, axes[r:r + chunk])
        lo[r:r + chunk] = torch.where(m[:, :, None], p, inf).amin(1)
        hi[r:r + chunk] = torch.where(m[:, :, None], p, -inf).amax(1)
        r2max[r:r + chunk] = torch.where(m, (d * d).sum(-1), -inf).amax(1)
    return lo, hi, r2max


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3


def run(N, K, cover, repeats, chunk_bytes):
    xyz, rgb = make_scan(N, 5)
    bits, area = make_masks(xyz, K, cover, 11)
    W = bits.shape[1]
    # the composed path holds about 8 (unpack's int64) + 1 + 8 (fp64 mask) + 12 + 12 (where) bytes per row and point at its peak
    chunk = max(1, min(K, chunk_bytes // (48 * N)))
    res = dict(points=N, masks=K, words=W, cover=cover, repeats=repeats, torch_row_chunk=chunk, bit_word_bytes=K * W * 8,
               members=dict(min=int(area.min()), max=int(area.max()), total=int(area.sum())))
    feats = features(xyz, rgb)

    count, sums, lo, hi = ops.mask_moments(xyz, bits, rgb)
    tc, ts, tlo, thi = torch_moments(xyz, bits, feats, chunk)
    assert torch.equal(count, tc) and torch.equal(count, area) and torch.equal(lo, tlo) and torch.equal(hi, thi), "count / box disagree with the torch-composed path"
    scale = torch_moments(xyz, bits, feats.abs(), chunk)[1]
    res["sums_max_diff_over_sum_abs"] = float(((sums - ts).abs() / scale).max())
    assert res["sums_max_diff_over_sum_abs"] < 1e-12
    again = ops.mask_moments(xyz, bits, rgb)[1]
    assert torch.equal(again, sums), "two runs of mask_moments differ"
    a, b = alternate(lambda: ops.mask_moments(xyz, bits, rgb), lambda: torch_moments(xyz, bits, feats, chunk), event, repeats)
    res["moments"] = pair(a, b)
    res["moments"]["bit_words_TB_per_s"] = round(K * W * 8 / (stat(a)["median"] * 1e-3) / 1e12, 4)
    res["moments"]["share_of_achievable_hbm"] = round(res["moments"]["bit_words_TB_per_s"] / HBM_ACHIEVABLE_TBS, 4)

    g = geometry.mask_geometry(xyz, bits, rgb)
    origin, axes = g.centroid.float().cuda().contiguous(), g.axes.cuda().contiguous()
    elo, ehi, er = ops.mask_extents(xyz, bits, origin, axes)
    tlo, thi, tr = torch_extents(xyz, bits, origin, axes, chunk)
    res["extents_max_abs_diff"] = float(max((elo - tlo).abs().max(), (ehi - thi).abs().max(), (er - tr).abs().max()))
    assert res["extents_max_abs_diff"] < 1e-5
    a, b = alternate(lambda: ops.mask_extents(xyz, bits, origin, axes), lambda: torch_extents(xyz, bits, origin, axes, chunk), event, repeats)
    res["extents"] = pair(a, b)
    res["extents"]["bit_words_TB_per_s"] = round(K * W * 8 / (stat(a)["median"] * 1e-3) / 1e12, 4)
    res["extents"]["share_of_achievable_hbm"] = round(res["extents"]["bit_words_TB_per_s"] / HBM_ACHIEVABLE_TBS, 4)

    res["mask_geometry_wall_ms"] = stat([wall(lambda: geometry.mask_geometry(xyz, bits, rgb))[1] for _ in range(repeats + 2)][2:])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="131072,4000000")
    ap.add_argument("--masks", type=int, default=256)
    ap.add_argument("--cover", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--chunk-bytes", type=int, default=4 << 30, help="intermediates the torch-composed path may hold at a time")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("geometry_bench.py needs a GPU: a timing taken anywhere else says nothing")
    out = []
    for N in (int(n) for n in args.points.split(",")):
        res = run(N, args.masks, args.cover, args.repeats, args.chunk_bytes)
        res["device"] = torch.cuda.get_device_name(0)
        res["hbm_TB_per_s"] = dict(achievable=HBM_ACHIEVABLE_TBS, spec=HBM_SPEC_TBS)
        print(json.dumps(res), flush=True)
        out.append(res)
        torch.cuda.empty_cache()
        if args.out:                                       # after every configuration: a run that is cut short keeps what it measured
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
