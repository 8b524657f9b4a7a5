"""Plain-numpy reference of the RGB-D frames (include/pointsam_hip.h, "RGB-D frames"): every fp32 operation rounded on its own (numpy float32 arrays do
that), the compares in fp32, the compaction by np.nonzero in C order -- ascending (f, y, x).  Also the inputs the CPU and the GPU tests share."""
import numpy as np

import view_reference as V

F32 = np.float32
EMPTY = V.EMPTY


# ------------------------------------------------------------------------------------------------ the definition
def depth_values(depth, depth_scale=None):
    """-> d [F, H, W] f32: the word, or (float)raw * depth_scale for uint16."""
    depth = np.asarray(depth)
    if depth.dtype == np.uint16:
        d = depth.astype(np.float32) * F32(depth_scale)
    else:
        assert depth.dtype == np.float32 and depth_scale is None
        d = depth
    assert d.dtype == np.float32 and d.ndim == 3
    return d


def kept(d, cams, far, edge):
    """-> [F, H, W] bool: range-valid and not dropped by the edge filter."""
    near = np.array([c.near for c in cams], dtype=np.float32)[:, None, None]
    with np.errstate(all="ignore"):
        valid = np.isfinite(d) & (d >= near) & (d <= F32(far))
        if edge is None:
            return valid
        limit = F32(edge) * d
        drop = np.zeros_like(valid)
        # (slice of this pixel, slice of its neighbour) on the y axis and on the x axis: a neighbour outside the image does not exist
        lo, hi, al = slice(0, -1), slice(1, None), slice(None)
        for (ys, yn), (xs, xn) in (((al, al), (hi, lo)), ((al, al), (lo, hi)), ((hi, lo), (al, al)), ((lo, hi), (al, al))):
            jump = np.abs(d[:, ys, xs] - d[:, yn, xn]) > limit[:, ys, xs]
            assert (d[:, ys, xs] - d[:, yn, xn]).dtype == np.float32
            drop[:, ys, xs] |= valid[:, yn, xn] & jump
    return valid & ~drop


def colours(rgb):
    rgb = np.asarray(rgb)
    if rgb.dtype == np.uint8:
        return (rgb.astype(np.float32) / F32(255) - F32(0.5)) / F32(0.5)
    assert rgb.dtype == np.float32
    return rgb


def unproject(depth, rgb, cams, far, edge=None, depth_scale=None):
    """-> (xyz_world [M, 3] f32, rgb [M, 3] f32, index [F, H, W] int32, M)."""
    d = depth_values(depth, depth_scale)
    Fn, H, W = d.shape
    assert len(cams) == Fn and all(c.width == W and c.height == H for c in cams)
    keep = kept(d, cams, far, edge)
    M = int(keep.sum())
    index = np.full(keep.shape, -1, dtype=np.int32)
    index[keep] = np.arange(M, dtype=np.int32)                        # boolean assignment runs in C order: ascending (f, y, x)
    xs, ys = np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32)
    world = np.zeros((Fn, H, W, 3), dtype=np.float32)
    with np.errstate(all="ignore"):
        for f, cam in enumerate(cams):
            P = cam.pose_words.reshape(3, 4)
            a = ((xs + F32(0.5)) - F32(cam.cx)) / F32(cam.fx)
            b = ((ys + F32(0.5)) - F32(cam.cy)) / F32(cam.fy)
            c = (a[None, :] * d[f], b[:, None] * d[f], d[f])
            q = [c[i] - P[i, 3] for i in range(3)]
            for j in range(3):
                world[f, :, :, j] = (P[0, j] * q[0] + P[1, j] * q[1]) + P[2, j] * q[2]
                assert ((P[0, j] * q[0] + P[1, j] * q[1]) + P[2, j] * q[2]).dtype == np.float32
    col = colours(rgb)
    return world[keep], np.ascontiguousarray(col[keep]), index, M


def normalise(xyz, center, scale):
    return (xyz - np.asarray(center, dtype=np.float32)) / F32(scale)


def auto_normalisation(xyz):
    """The rule of evaluation.normalize_points in fp64, rounded to fp32 once: -> (center [3] f32, scale f32).  A single point (or coinciding ones)
    has no radius: the scale is then 1, so that the tiniest test shapes still have a normalisation to check."""
    x = np.asarray(xyz, dtype=np.float64)
    m = x.mean(0)
    s = F32(np.sqrt(((x - m) ** 2).sum(1).max()))
    return m.astype(np.float32), s if s > 0 else F32(1)


def normalised_pose(pose_words, center, scale):
    """[R | t] fp32 words, fp32 centre m and scale s -> [R | (R m + t) / s] in fp64 (twelve numbers, row-major)."""
    P = np.asarray(pose_words, dtype=np.float64).reshape(3, 4)
    m, s = np.asarray(center, dtype=np.float32).astype(np.float64), float(F32(scale))
    t = (((P[:, 0] * m[0] + P[:, 1] * m[1]) + P[:, 2] * m[2]) + P[:, 3]) / s
    return np.concatenate([P[:, :3], t[:, None]], axis=1)


def normalised_cam(cam, center, scale):
    return V.Cam(pose=normalised_pose(cam.pose_words, center, scale), fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, width=cam.width, height=cam.height,
                 near=cam.near / float(F32(scale)))


def keys(xyz, index, cams):
    """xyz [M, 3] normalised, index [F, H, W], the NORMALISED cameras -> keys [F, H, W] uint64."""
    out = np.full(index.shape, EMPTY, dtype=np.uint64)
    M = len(xyz)
    with np.errstate(all="ignore"):
        for f, cam in enumerate(cams):
            P = cam.pose_words.reshape(3, 4)
            has = (index[f] >= 0) & (index[f] < M)
            i = index[f][has]
            p = xyz[i]
            z = ((P[2, 0] * p[:, 0] + P[2, 1] * p[:, 1]) + P[2, 2] * p[:, 2]) + P[2, 3]
            assert z.dtype == np.float32
            k = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | i.astype(np.uint64)
            k[~(np.isfinite(z) & (z > 0))] = EMPTY
            out[f][has] = k
    return out


def frames(depth, rgb, cams, far, edge=None, depth_scale=None, center=None, scale=None):
    """Everything at once -> dict(world, xyz, rgb, index, M, center, scale, cams, keys)."""
    world, col, index, M = unproject(depth, rgb, cams, far, edge, depth_scale)
    if center is None:
        center, scale = auto_normalisation(world)
    xyz = normalise(world, center, scale)
    ncams = [normalised_cam(c, center, scale) for c in cams]
    return dict(world=world, xyz=xyz, rgb=col, index=index, M=M, center=np.asarray(center, dtype=np.float32), scale=F32(scale), cams=ncams,
                keys=keys(xyz, index, ncams))


# ------------------------------------------------------------------------------------------------ the shared inputs
def rodrigues(axis, angle, t):
    """-> the pose [R | t] 3 x 4 in fp64, R the rotation by `angle` about `axis`."""
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) * np.cos(angle) + np.sin(angle) * K + (1 - np.cos(angle)) * np.outer(k, k)
    return np.concatenate([R, np.asarray(t, dtype=np.float64)[:, None]], axis=1)


ROOM_POSES = (rodrigues((1, 2, 3), 0.7, (0.3, -0.2, 5.0)), rodrigues((0, 1, 0.2), -0.4, (0.1, -0.05, 0.4)))
ROOM_FAR = 10.0


def room_case(first_pose=None):
    """Two frames of 96 x 128 of a wall at depth 3 with a box at depth 2 in rows 30:60, columns 40:90, noise of 2 mm; rows 0:3 are zero, and (y, x) =
    (10, 10) is a NaN, (11, 11) +inf, (12, 12) 50.0 (beyond far = 10).  -> (depth [2, 96, 128] f32, rgb [2, 96, 128, 3] uint8, [Cam, Cam], far).
    Without the edge filter 2 * (12288 - 384 - 3) = 23802 pixels are kept; with edge = 0.05 the 156 + 160 pixels on either side of the box's outline
    go in each frame: 23170."""
    H, W = 96, 128
    depth = np.full((2, H, W), 3.0)
    depth[:, 30:60, 40:90] = 2.0
    depth += np.random.default_rng(0).normal(0, 0.002, depth.shape)
    depth[:, 0:3] = 0.0
    depth[:, 10, 10], depth[:, 11, 11], depth[:, 12, 12] = np.nan, np.inf, 50.0
    rgb = np.random.default_rng(1).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    poses = (ROOM_POSES[0] if first_pose is None else first_pose, ROOM_POSES[1])
    return depth.astype(np.float32), rgb, [V.Cam(pose=p) for p in poses], ROOM_FAR


ROOM_KEPT, ROOM_KEPT_EDGE = 23802, 23170


def room_case_u16():
    """The room in millimetres: (depth uint16, depth_scale).  The NaN becomes a raw 0, +inf a raw 65535 (65.5: beyond far), 50.0 a raw 50000."""
    depth = room_case()[0]
    with np.errstate(invalid="ignore"):
        mm = np.where(np.isnan(depth), 0.0, np.minimum(np.round(depth.astype(np.float64) * 1000.0), 65535.0))
    return mm.astype(np.uint16), 0.001


def pattern_case(Fn, H, W, seed=0, every_other=False, dead_frame=None):
    """Cheap patterned frames of any shape: depth 1 + a slow ramp + a seeded sprinkle of invalid values and jumps, uint8 colour, cameras whose principal
    point is the image's centre and whose poses are small rotations.  -> (depth f32, rgb uint8, cams, far)."""
    rng = np.random.default_rng(seed)
    n = Fn * H * W
    p = np.arange(n, dtype=np.int64)
    depth = (1.0 + (p % 97) / 970.0 + (p % 7 == 3) * 0.5).astype(np.float32)
    bad = rng.random(n) < 0.1
    depth[bad] = rng.choice(np.array([0.0, np.nan, np.inf, -1.0, 100.0], dtype=np.float32), int(bad.sum()))
    if every_other:
        depth[p % 2 == 1] = 0.0
    depth[0] = 1.0                                                     # the first pixel is always kept: no shape is empty by accident
    depth = depth.reshape(Fn, H, W)
    if dead_frame is not None:
        depth[dead_frame] = np.nan
    rgb = rng.integers(0, 256, (Fn, H, W, 3), dtype=np.uint8)
    cams = [V.Cam(pose=rodrigues((1, f + 1, 0.5), 0.1 * (f + 1), (0.1 * f, -0.2, 0.3 + f)), fx=0.8 * max(W, H), fy=0.8 * max(W, H), cx=W / 2, cy=H / 2,
                  width=W, height=H, near=0.05 * (f + 1)) for f in range(Fn)]
    return depth, rgb, cams, 4.0


def hand_case():
    """Four frames of 1 x 8 (only the x neighbours exist, and none across a frame), near = 0.5, far = 4, edge = 0.25.  -> (depth [4, 1, 8] f32, rgb uint8,
    cams, far, edge, keep [4, 1, 8] bool written out by hand).
      frame 0   NaN, +inf, -inf, 0 and a negative depth between ordinary pixels: invalid themselves, and as neighbours they do not count
      frame 1   near itself is in, one ulp below is out, one ulp above is in
      frame 2   far itself is in, one ulp above is out, one ulp below is in
      frame 3   d = 2 beside 2.5: |d - d_n| = 0.5 = edge * d exactly, kept; beside the fp32 successor of 2.5 the difference 0.5 + 2^-22 is exact and
                larger: dropped.  The 2.5 pixels themselves have the limit 0.625 and stay."""
    nan, inf = np.nan, np.inf
    up, down = (lambda v: np.nextafter(F32(v), F32(np.inf))), (lambda v: np.nextafter(F32(v), F32(-np.inf)))
    T, N = True, False
    d = np.array([[nan, 1, inf, 1, -inf, 1, 0, -1.0],
                  [0.5, 0.5, down(0.5), 0.5, up(0.5), 0.5, 0.5, 0.5],
                  [4.0, 4.0, up(4.0), 4.0, down(4.0), 4.0, 4.0, 4.0],
                  [2.0, 2.5, 2.0, 2.0, up(2.5), 2.0, 2.0, 2.0]], dtype=np.float32)[:, None, :]
    keep = np.array([[N, T, N, T, N, T, N, N],
                     [T, T, N, T, T, T, T, T],
                     [T, T, N, T, T, T, T, T],
                     [T, T, T, N, T, N, T, T]])[:, None, :]
    rgb = np.random.default_rng(2).integers(0, 256, (4, 1, 8, 3), dtype=np.uint8)
    cams = [V.Cam(pose=rodrigues((0, 0, 1), 0.3 * f, (0.0, 0.1 * f, 0.2)), fx=6.0, fy=6.0, cx=4.0, cy=0.5, width=8, height=1, near=0.5) for f in range(4)]
    return d, rgb, cams, 4.0, 0.25, keep
