"""Scan map views' definition (include/pointsam_hip.h, "scan map views") in numpy float32 and Python integers, on top of scanmap_reference.RefMap:
the eye and its cell, the integer direction N of every pixel, the walk from the eye's cell towards o + N in carve_reference.walk_by_differences'
difference form (as a generator: a ray towards a cell 2^21 away is never walked to its end), and `view`, which returns the keys and, per pixel, the
cells the ray visited inside the grid.  Nothing here touches the library.
"""
import numpy as np

import scanmap_reference as SM

F = np.float32
AXIS_CELLS = 1 << SM.AXIS_BITS
EMPTY = -1


def eye_of(pose_words):
    """e = -R^T t in fp64 from the twelve fp32 words, rounded to fp32 once -> [3] float32."""
    w = np.asarray(pose_words, dtype=F).reshape(3, 4).astype(np.float64)
    with np.errstate(all="ignore"):
        return (-(w[:, :3].T @ w[:, 3])).astype(F)


def eye_cell(eye, inv_h):
    """The eye's cell, or None: a map point's cell and acceptance test."""
    eye = np.asarray(eye, dtype=F).reshape(1, 3)
    cell, ok = SM.cells(eye, inv_h)
    with np.errstate(all="ignore"):
        inside = (eye >= F(-1)) & (eye <= F(1))
    return tuple(int(c) for c in cell[0]) if ok.all() and inside.all() else None


def cmax_of(inv_h):
    """The largest cell of an axis: (int)floorf(2 inv_h), below 2^21."""
    with np.errstate(over="ignore"):
        top = np.floor(F(2) * F(inv_h))
    return int(top) if top < F(AXIS_CELLS) else AXIS_CELLS - 1


def directions(camera):
    """-> (N [H, W, 3] int64, ok [H, W] bool): the fp32 recipe, every operation rounded on its own; N = 0 where the pixel has no ray."""
    w = np.asarray(camera.pose_words, dtype=F).reshape(3, 4)
    px, py = np.arange(camera.width, dtype=F)[None, :], np.arange(camera.height, dtype=F)[:, None]
    with np.errstate(all="ignore"):
        a = ((px + F(0.5)) - F(camera.cx)) / F(camera.fx)
        b = ((py + F(0.5)) - F(camera.cy)) / F(camera.fy)
        a, b = np.broadcast_arrays(a, b)
        d = np.stack([(w[0, k] * a + w[1, k] * b) + w[2, k] for k in range(3)], -1).astype(F)
        m = np.abs(d).max(-1)                                      # a NaN propagates
        ok = (m > 0) & (m < np.inf)
        N = np.rint((d / np.where(ok, m, F(1))[..., None]) * F(2097152.0))
    return np.where(ok[..., None], N, 0).astype(np.int64), ok


def walk_cells(o, N):
    """The cells the ray from cell o towards cell o + N crosses, in order, o excluded: carve_reference.walk_by_differences, one cell at a time.  Ends
    before o + N."""
    n = [abs(int(v)) for v in N]
    s = [-1 if v < 0 else 1 for v in N]
    r = list(n)
    D01, D02, D12 = n[1] - n[0], n[2] - n[0], n[2] - n[1]
    cur = [int(v) for v in o]
    for _ in range(sum(n)):
        t0, t1, t2 = D01 <= 0 and D02 <= 0, D01 >= 0 and D12 <= 0, D02 >= 0 and D12 >= 0
        for a, t in enumerate((t0, t1, t2)):
            cur[a] += s[a] * t
            r[a] -= t
        D01 += 2 * n[1] * t0 - 2 * n[0] * t1
        D02 += 2 * n[2] * t0 - 2 * n[0] * t2
        D12 += 2 * n[2] * t1 - 2 * n[1] * t2
        if max(r) <= 0:
            return
        yield tuple(cur)


def truncated(o, N, cmax):
    """walk_cells cut where it first leaves the grid 0 .. cmax -> the list of visited cells."""
    out = []
    for c in walk_cells(o, N):
        if min(c) < 0 or max(c) > cmax:
            break
        out.append(c)
    return out


def depths(ref, pose_words):
    """The fp32 depth of every voxel's mean under the camera: pose_apply's third word."""
    xyz = ref.cloud()[0]
    w = np.asarray(pose_words, dtype=F)
    with np.errstate(all="ignore"):
        return (((w[8] * xyz[:, 0] + w[9] * xyz[:, 1]) + w[10] * xyz[:, 2]) + w[11]).astype(F)


def key_of(depth, v):
    return (int(np.asarray(depth, dtype=F).view(np.uint32)) << 32) | int(v)


def view(ref, camera, skip=None, min_count=1, V=None):
    """-> (keys [H, W] int64, visited: {(px, py): [cells]}).  skip: None or [V] bool."""
    H, W = camera.height, camera.width
    keys = np.full((H, W), EMPTY, dtype=np.int64)
    visited = {}
    V = ref.V if V is None else V
    o = eye_cell(eye_of(camera.pose_words), ref.inv_h)
    if o is None or ref.dead or V == 0:
        return keys, visited
    cmax = cmax_of(ref.inv_h)
    depth = depths(ref, camera.pose_words)
    N, ok = directions(camera)
    near = F(camera.near)
    for py in range(H):
        for px in range(W):
            cells = visited[(px, py)] = []
            if not ok[py, px]:
                continue
            for c in walk_cells(o, N[py, px]):
                if min(c) < 0 or max(c) > cmax:
                    break
                cells.append(c)
                v = ref.id_of.get(c[0] | (c[1] << SM.AXIS_BITS) | (c[2] << (2 * SM.AXIS_BITS)))
                if v is None or v >= V or ref.count[v] < min_count or (skip is not None and skip[v]):
                    continue
                if not (depth[v] >= near and depth[v] < np.inf):
                    continue
                keys[py, px] = key_of(depth[v], v)
                break
    return keys, visited


# ------------------------------------------------------------------------------------------------ the table's home slots
def voxel_hash(key):
    """csrc/voxel_cell.h: the 64-bit finaliser of MurmurHash3."""
    M64 = (1 << 64) - 1
    k = int(key) & M64
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & M64
    return k ^ (k >> 33)


def capacity(max_voxels):
    c = 64
    while c < 2 * max_voxels:
        c <<= 1
    return c


def home_slots(keys, max_voxels):
    """The slot each key is looked for first in a map of max_voxels."""
    mask = capacity(max_voxels) - 1
    return [voxel_hash(k) & 0xffffffff & mask for k in keys]


# ------------------------------------------------------------------------------------------------ cameras of the tests
def axis_camera(eye, width, height, f, cx, cy, near=1e-3):
    """A camera at `eye` looking along +z of the map with x, y as the map's: R = I, t = -eye."""
    from point_sam_amd.views import Camera
    pose = np.concatenate([np.eye(3), -np.asarray(eye, dtype=np.float64)[:, None]], 1)
    return Camera(pose, f, f, cx, cy, width, height, near)


def diagonal_camera(eye, width, height, f, cx, cy, near=1e-3):
    """A camera whose third rotation row is (0.70710677, 0.70710677, 0) in fp32: the principal-point pixel has N = (2^21, 2^21, 0).  Built with
    Camera.from_fp32, so the two words are equal bit for bit."""
    from point_sam_amd.views import Camera
    h = F(0.70710677)
    R = np.array([[h, -h, 0], [0, 0, -1], [h, h, 0]], dtype=F)     # rows x, y (down = -z of the map), z
    t = -(R.astype(np.float64) @ np.asarray(eye, dtype=np.float64))
    words = np.concatenate([R, t.astype(F)[:, None]], 1).reshape(12).astype(F)
    return Camera.from_fp32(words, float(F(f)), float(F(f)), float(F(cx)), float(F(cy)), width, height, float(F(near)))
