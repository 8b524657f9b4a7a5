"""Plain numpy reference of the scene-crop kernels, written from the definitions in include/pointsam_hip.h and independent of the package.  Everything is
fp32 with one rounded operation at a time (numpy's float32 arithmetic is exactly that):

    member      d = x - c per axis,  q = (dx dx + dy dy) + dz dz,  member iff q <= r2,  r2 = fl32(r) * fl32(r)  (NaN compares false)
    coordinate  u = min(max(d * inv_r, -1), 1),  inv_r = fl32(1) / fl32(r)
    cell        floor((u - (-1)) * inv_h) per axis,  inv_h = fl32(1) / fl32(h);  key = cx | cy << 21 | cz << 42
    the representative of a voxel is its MEMBER with the lowest scan index; without a voxel size every member is its own representative
    keep_idx = the representatives in increasing order;  inv[i] = the position in keep_idx of member i's representative, -1 for a non-member
    shell       a point is in the outer shell iff q > rs * rs,  rs = fl32((1 - edge_frac) * fl32(r)), the product taken in double precision
"""
import numpy as np

from scene_reference import unwords, words

f32 = np.float32
AXIS_BITS = 21


def ball(xyz, center, radius):
    """-> (d [M, 3] f32, q [M] f32, member [M] bool)."""
    xyz = np.asarray(xyz, dtype=f32)
    c = np.asarray(center, dtype=f32)
    r = f32(radius)
    r2 = f32(r * r)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (xyz - c[None]).astype(f32)
        q = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(f32) + d[:, 2] * d[:, 2]).astype(f32)
        member = q <= r2
    return d, q, member


def normalise(d, radius):
    inv_r = f32(1) / f32(radius)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.minimum(np.maximum((d * inv_r).astype(f32), f32(-1)), f32(1)).astype(f32)


def crop_downsample(xyz, rgb, center, radius, h=None):
    """-> (keep_idx [count] int64, inv [M] int64, wxyz [count, 3] f32, wrgb [count, 3] f32, members)."""
    xyz = np.asarray(xyz, dtype=f32)
    M = len(xyz)
    d, _, member = ball(xyz, center, radius)
    idx = np.nonzero(member)[0]
    u = normalise(d[idx], radius)
    inv = np.full(M, -1, dtype=np.int64)
    if h is None or len(idx) == 0:
        keep = idx.astype(np.int64)
        inv[idx] = np.arange(len(idx))
    else:
        inv_h = f32(1) / f32(h)
        c = np.floor(((u - f32(-1)).astype(f32) * inv_h).astype(f32))
        if not ((c >= 0).all() and (c < f32(1 << AXIS_BITS)).all()):
            raise ValueError("a member's cell is outside [0, 2^21)")
        c = c.astype(np.uint64)
        key = c[:, 0] | (c[:, 1] << np.uint64(AXIS_BITS)) | (c[:, 2] << np.uint64(2 * AXIS_BITS))
        _, first, inverse = np.unique(key, return_index=True, return_inverse=True)      # positions among the members: increasing with the scan index
        order = np.argsort(first, kind="stable")
        rank = np.empty(len(first), dtype=np.int64)
        rank[order] = np.arange(len(first))
        keep = idx[first[order]].astype(np.int64)
        inv[idx] = rank[inverse.reshape(-1)]
    wxyz = normalise(d[keep], radius)
    wrgb = np.asarray(rgb, dtype=f32)[keep]
    return keep, inv, wxyz, wrgb, int(member.sum())


def expand_rows(src, inv, fill):
    """src [R, Nw] -> [R, M]: src[:, inv] bit for bit where inv >= 0, `fill` elsewhere."""
    src = np.asarray(src)
    inv = np.asarray(inv)
    out = np.full((src.shape[0], len(inv)), fill, dtype=src.dtype)
    on = inv >= 0
    out[:, on] = src[:, inv[on]]
    return out


def expand_bits(words_w, inv, Nw):
    """words_w [K, ceil(Nw / 64)] -> (words_f [K, ceil(M / 64)], area_f [K] int32): zero bits where inv < 0."""
    inv = np.asarray(inv)
    work = unwords(words_w, Nw)
    full = np.zeros((work.shape[0], len(inv)), dtype=bool)
    on = inv >= 0
    full[:, on] = work[:, inv[on]]
    return words(full), full.sum(1).astype(np.int32)


def crop_prompts(points, center, radius):
    """points [..., 3] in scan coordinates -> crop coordinates; ValueError for a point outside the ball."""
    p = np.asarray(points, dtype=f32)
    d, _, member = ball(p.reshape(-1, 3), center, radius)
    if not member.all():
        raise ValueError("a prompt lies outside the ball")
    return normalise(d, radius).reshape(p.shape)


def shell(xyz, center, radius, edge_frac):
    """-> [M] bool: q > rs * rs."""
    rs = f32((1.0 - edge_frac) * float(f32(radius)))
    _, q, _ = ball(xyz, center, radius)
    with np.errstate(invalid="ignore"):
        return q > f32(rs * rs)


def drop_shell_masks(masks, shell_row):
    """masks [K, N] bool, shell_row [N] bool -> [K] bool: True for the masks to keep (no point in the shell)."""
    return ~(np.asarray(masks, dtype=bool) & np.asarray(shell_row, dtype=bool)[None]).any(1)
