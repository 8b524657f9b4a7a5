"""Plain numpy reference of the full-resolution scene kernels, written from the definitions in include/pointsam_hip.h and independent of the package.

    cell of a point, per axis, in fp32 with every operation rounded on its own:  c = floor((x - origin) * inv_h),  inv_h = fl32(1) / fl32(h)
    a non-finite coordinate or a cell outside [0, 2^21) raises ValueError
    key = cx | cy << 21 | cz << 42;  the representative of a voxel is its point with the lowest index
    keep_idx = the representatives in increasing order;  inv[i] = the position in keep_idx of point i's representative
"""
import numpy as np

f32 = np.float32
AXIS_BITS = 21


def cells(xyz, h, origin=(-1.0, -1.0, -1.0)):
    """-> (cells [M, 3] fp32 values of floor, bad [M] bool)."""
    xyz = np.asarray(xyz, dtype=f32)
    inv_h = f32(1) / f32(h)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (xyz - np.asarray(origin, dtype=f32)[None]).astype(f32)
        c = np.floor((d * inv_h).astype(f32))
        bad = ~(np.isfinite(xyz).all(1) & (c >= 0).all(1) & (c < f32(1 << AXIS_BITS)).all(1))
    return c, bad


def keys(xyz, h, origin=(-1.0, -1.0, -1.0)):
    c, bad = cells(xyz, h, origin)
    if bad.any():
        raise ValueError("a coordinate is not finite or its cell is outside [0, 2^21)")
    c = c.astype(np.uint64)
    return c[:, 0] | (c[:, 1] << np.uint64(AXIS_BITS)) | (c[:, 2] << np.uint64(2 * AXIS_BITS))


def downsample(xyz, h, origin=(-1.0, -1.0, -1.0)):
    """-> (keep_idx [count] int64, inv [M] int64)."""
    k = keys(xyz, h, origin)
    _, first, inverse = np.unique(k, return_index=True, return_inverse=True)      # first = the lowest index of each key (unique keys sorted by value)
    order = np.argsort(first, kind="stable")                                      # re-rank the voxels by their first index
    rank = np.empty(len(first), dtype=np.int64)
    rank[order] = np.arange(len(first))
    return first[order].astype(np.int64), rank[inverse.reshape(-1)].astype(np.int64)


def expand_rows(src, inv):
    """src [R, Nw] -> [R, M]: a copy, bit for bit."""
    return np.ascontiguousarray(np.asarray(src)[:, inv])


def words(masks):
    """[K, N] bool -> [K, ceil(N / 64)] uint64: bit n % 64 of word n / 64 is point n, bits past N are zero."""
    masks = np.asarray(masks, dtype=bool)
    K, N = masks.shape
    W = (N + 63) // 64
    pad = np.zeros((K, W * 64), dtype=bool)
    pad[:, :N] = masks
    return np.packbits(pad, axis=1, bitorder="little").view("<u8").reshape(K, W)


def unwords(w, N):
    w = np.ascontiguousarray(w).astype("<u8")
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little")[:, :N].astype(bool)


def expand_bits(words_w, inv, Nw):
    """words_w [K, ceil(Nw / 64)] -> (words_f [K, ceil(M / 64)], area_f [K] int32)."""
    full = unwords(words_w, Nw)[:, inv]
    return words(full), full.sum(1).astype(np.int32)
