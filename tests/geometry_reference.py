"""Instance geometry, written from include/pointsam_hip.h in plain numpy: the definition the kernels of csrc/geometry.hip are held to.

Independent of the package.  Members come from the bits with every position >= N masked; counts are exact; min / max are taken in the header's
order (-inf < .. < -0 < +0 < .. < +inf); each of the twelve sums is math.fsum over exactly formed fp64 terms, i.e. the correctly rounded value
of the exact sum; the extents are a float32 emulation of the stated operation order."""
import math

import numpy as np

f32 = np.float32


def words(mask: np.ndarray) -> np.ndarray:
    """bool [K, N] -> int64 words [K, ceil(N / 64)]; the bits past N are zero."""
    K, N = mask.shape
    W = (N + 63) // 64
    pad = np.zeros((K, W * 64), dtype=np.uint64)
    pad[:, :N] = mask
    sh = np.arange(64, dtype=np.uint64)
    return (pad.reshape(K, W, 64) << sh).sum(-1, dtype=np.uint64).view(np.int64)


def members(row: np.ndarray, N: int) -> np.ndarray:
    """One row of int64 words -> the indices < N of its set bits, increasing.  Bits at positions >= N are ignored."""
    u = np.ascontiguousarray(row).view(np.uint64)
    b = ((u[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(-1)
    return np.nonzero(b[:N])[0]


def _key(a: np.ndarray) -> np.ndarray:
    u = np.ascontiguousarray(a, dtype=f32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def ordered_min(a: np.ndarray, empty=np.inf) -> np.float32:
    """The minimum of fp32 values in the order that puts -0 below +0."""
    a = np.asarray(a, dtype=f32).reshape(-1)
    return f32(empty) if a.size == 0 else a[np.argmin(_key(a))]


def ordered_max(a: np.ndarray, empty=-np.inf) -> np.float32:
    a = np.asarray(a, dtype=f32).reshape(-1)
    return f32(empty) if a.size == 0 else a[np.argmax(_key(a))]


def moment_terms(xyz: np.ndarray, rgb=None) -> np.ndarray:
    """[n, 3] fp32 points (and colours) -> the [n, 12] fp64 terms x, y, z, xx, xy, xz, yy, yz, zz, r, g, b: every one exact."""
    p = xyz.astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    c = np.zeros_like(p) if rgb is None else rgb.astype(np.float64)
    return np.stack([x, y, z, x * x, x * y, x * z, y * y, y * z, z * z, c[:, 0], c[:, 1], c[:, 2]], 1)


def mask_moments(xyz: np.ndarray, bits: np.ndarray, rgb=None):
    """-> (count [K] int32, sums [K, 12] f64 correctly rounded, lo [K, 3] f32, hi [K, 3] f32, abs_sums [K, 12] f64 = fsum of |term|)."""
    N, K = len(xyz), len(bits)
    count = np.zeros(K, dtype=np.int32)
    sums, abs_sums = np.zeros((K, 12)), np.zeros((K, 12))
    lo, hi = np.full((K, 3), np.inf, dtype=f32), np.full((K, 3), -np.inf, dtype=f32)
    for k in range(K):
        idx = members(bits[k], N)
        count[k] = len(idx)
        t = moment_terms(xyz[idx], None if rgb is None else rgb[idx])
        for c in range(12):
            sums[k, c] = math.fsum(t[:, c])
            abs_sums[k, c] = math.fsum(np.abs(t[:, c]))
        for a in range(3):
            lo[k, a], hi[k, a] = ordered_min(xyz[idx, a]), ordered_max(xyz[idx, a])
    return count, sums, lo, hi, abs_sums


def project(xyz: np.ndarray, origin: np.ndarray, axes=None):
    """The header's fp32 operations for points [n, 3]: -> (p [n, 3], r2 [n]), every operation rounded to fp32 on its own, in the stated order."""
    x, o = xyz.astype(f32), np.asarray(origin, dtype=f32)
    d = (x - o[None]).astype(f32)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    r2 = ((dx * dx).astype(f32) + (dy * dy).astype(f32)).astype(f32)
    r2 = (r2 + (dz * dz).astype(f32)).astype(f32)
    if axes is None:
        return d, r2
    a = np.asarray(axes, dtype=f32)
    p = np.empty_like(d)
    for i in range(3):
        s = ((dx * a[i, 0]).astype(f32) + (dy * a[i, 1]).astype(f32)).astype(f32)
        p[:, i] = (s + (dz * a[i, 2]).astype(f32)).astype(f32)
    return p, r2


def mask_extents(xyz: np.ndarray, bits: np.ndarray, origin: np.ndarray, axes=None):
    """-> (lo [K, 3], hi [K, 3], r2max [K]) f32; +inf / -inf / -inf for an empty row."""
    N, K = len(xyz), len(bits)
    lo, hi = np.full((K, 3), np.inf, dtype=f32), np.full((K, 3), -np.inf, dtype=f32)
    r2max = np.full(K, -np.inf, dtype=f32)
    for k in range(K):
        idx = members(bits[k], N)
        p, r2 = project(xyz[idx], origin[k], None if axes is None else axes[k])
        for a in range(3):
            lo[k, a], hi[k, a] = ordered_min(p[:, a]), ordered_max(p[:, a])
        r2max[k] = ordered_max(r2)
    return lo, hi, r2max
