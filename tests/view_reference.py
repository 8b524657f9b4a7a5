"""Plain-numpy reference of the camera views (include/pointsam_hip.h, "camera views"): every fp32 operation rounded on its own (numpy float32 arrays do
that), the compares before any conversion to an integer, the splat by np.minimum.at.  Also the inputs the CPU and the GPU tests share."""
import numpy as np

F = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 3]], dtype=np.float32)                  # identity rotation, translation (0, 0, 3)
c_, s_ = np.cos(0.4), np.sin(0.4)
ROTATED = np.array([[c_, 0, s_, 0.1], [0.1 * s_, 0.995, -0.1 * c_, -0.05], [-s_, 0, c_, 3.2]], dtype=np.float32)      # not orthonormal to the last bit: nothing assumes it


class Cam:
    """The camera as the kernels receive it: fp32 words (the attributes of point_sam_amd.views.Camera)."""

    def __init__(self, pose=IDENTITY, fx=160.0, fy=160.0, cx=64.0, cy=48.0, width=128, height=96, near=0.01):
        self.pose_words = np.asarray(pose, dtype=np.float32).reshape(12)
        self.fx, self.fy, self.cx, self.cy, self.near = (float(F(v)) for v in (fx, fy, cx, cy, near))
        self.width, self.height = int(width), int(height)


def project(xyz, cam):
    """-> (in_view [N] bool, px [N] int64, py [N] int64, depth [N] f32); px / py are 0 where the point is not in view."""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    P = cam.pose_words.reshape(3, 4)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all="ignore"):
        c = [((P[a, 0] * x + P[a, 1] * y) + P[a, 2] * z) + P[a, 3] for a in range(3)]
        assert all(v.dtype == np.float32 for v in c)
        u = F(cam.fx) * (c[0] / c[2]) + F(cam.cx)
        v = F(cam.fy) * (c[1] / c[2]) + F(cam.cy)
        ok = (c[2] >= F(cam.near)) & np.isfinite(c[2]) & (u >= F(0)) & (u < F(cam.width)) & (v >= F(0)) & (v < F(cam.height))
    px = np.zeros(len(xyz), dtype=np.int64)
    py = np.zeros(len(xyz), dtype=np.int64)
    px[ok] = np.floor(u[ok]).astype(np.int64)                                      # the conversion only of values already known to be in range
    py[ok] = np.floor(v[ok]).astype(np.int64)
    return ok, px, py, c[2]


def point_keys(depth):
    return (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(len(depth), dtype=np.uint64)


def splat(xyz, cam, s):
    """-> keys [height, width] uint64."""
    ok, px, py, depth = project(xyz, cam)
    key = point_keys(depth)
    keys = np.full(cam.height * cam.width, EMPTY, dtype=np.uint64)
    for dy in range(-s, s + 1):
        for dx in range(-s, s + 1):
            qx, qy = px + dx, py + dy
            m = ok & (qx >= 0) & (qx < cam.width) & (qy >= 0) & (qy < cam.height)
            np.minimum.at(keys, (qy * cam.width + qx)[m], key[m])
    return keys.reshape(cam.height, cam.width)


def index_of(keys):
    return (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32).reshape(keys.shape)


def depth_of(keys):
    d = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32).reshape(keys.shape).copy()
    d[keys == EMPTY] = np.inf
    return d


def pick(keys, pixels, w):
    """pixels [P, 2] (x, y) -> [P] int32."""
    H, W = keys.shape
    out = np.full(len(pixels), -1, dtype=np.int32)
    for c, (qx, qy) in enumerate(np.asarray(pixels).tolist()):
        best = None
        for dy in range(-w, w + 1):
            for dx in range(-w, w + 1):
                x, y = qx + dx, qy + dy
                if 0 <= x < W and 0 <= y < H and keys[y, x] != EMPTY:
                    cand = (dx * dx + dy * dy, int(keys[y, x]))
                    if best is None or cand < best:
                        best = cand
        if best is not None:
            out[c] = np.int64(best[1] & 0xFFFFFFFF).astype(np.int32)
    return out


def unpack(bits, N):
    """bits [K, Wd] uint64 (or int64) -> [K, N] bool."""
    b = np.asarray(bits).view(np.uint64)
    return ((b[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(b.shape[0], -1)[:, :N]


def pack(mask):
    """[K, N] bool -> [K, ceil(N / 64)] int64 words of mask_pack's layout."""
    K, N = mask.shape
    Wd = (N + 63) // 64
    pad = np.zeros((K, Wd * 64), dtype=np.uint64)
    pad[:, :N] = mask
    return (pad.reshape(K, Wd, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64).view(np.int64)


def paint_rows(keys, bits, N):
    """-> rows [K, H, W] uint8."""
    idx = index_of(keys)
    ok = (keys != EMPTY) & (idx.view(np.uint32) < N)
    m = unpack(bits, N)
    return (m[:, np.where(ok, idx, 0)] & ok[None]).astype(np.uint8)


def paint_ids(keys, bits, N):
    rows = paint_rows(keys, bits, N)
    return np.where(rows.any(0), rows.argmax(0), -1).astype(np.int32)


def lift(xyz, cam, keys, img, tau):
    """img [K, H, W] or None -> (bits [K, Wd] int64, area [K] int32)."""
    ok, px, py, depth = project(xyz, cam)
    k = keys[py, px]
    with np.errstate(all="ignore"):
        front = (k >> np.uint64(32)).astype(np.uint32).view(np.float32)
        vis = ok & (k != EMPTY) & (depth <= front + F(tau))
    on = vis[None] if img is None else vis[None] & (np.asarray(img)[:, py, px] != 0)
    return pack(on), on.sum(1).astype(np.int32)


# ------------------------------------------------------------------------------------------------ the shared inputs
def sphere_case(n=20000, radius=0.8, seed=0):
    """n points on a sphere shell at the origin: normalised default_rng(seed).normal."""
    g = np.random.default_rng(seed).normal(size=(n, 3))
    return (radius * g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)


def plane_case():
    """Two copies of a 40 x 40 lattice at spacing 1/64 in the plane z = 0: every occupied pixel has at least two points tied in depth."""
    a = (np.arange(40) - 20) / 64.0
    g = np.stack(np.meshgrid(a, a, indexing="ij"), -1).reshape(-1, 2)
    one = np.concatenate([g, np.zeros((len(g), 1))], 1).astype(np.float32)
    return np.concatenate([one, one])


def ray_case(n=20000, seed=1):
    """n points on the ray through the centre of pixel (70, 50) of Cam(), at distinct depths, near to far."""
    cam = Cam()
    depth = np.linspace(1.0, 5.0, n).astype(np.float32)
    assert len(np.unique(depth)) == n
    dx, dy = (70.5 - cam.cx) / cam.fx, (50.5 - cam.cy) / cam.fy
    pts = np.stack([dx * depth, dy * depth, depth - 3.0], 1).astype(np.float32)
    ok, px, py, _ = project(pts, cam)
    assert ok.all() and (px == 70).all() and (py == 50).all()
    return pts


def hand_points():
    """Cam() at identity rotation, depth 1 (z = -2): u = 160 x + 64, v = 160 y + 48.  -> (points [n, 3] f32, expected in-view pixel or None per point)."""
    inf, nan = np.inf, np.nan
    z = -2.0
    pts = [
        ((0.0, 0.0, z), (64, 48)),                          # the principal point: u = 64 exactly, on the border of pixels 63 | 64 -> 64
        ((-0.4, -0.3, z), (0, 0)),                          # u = 0, v = 0: in pixel (0, 0)
        ((0.4, 0.0, z), None),                              # u == width: out
        ((0.0, 0.3, z), None),                              # v == height: out
        ((0.3999, 0.2999, z), (127, 95)),                   # the last pixel
        ((-0.4001, 0.0, z), None),                          # just left of the image
        ((0.0, 0.0, -3.5), None),                           # behind the camera
        ((0.0, 0.0, -3.0), None),                           # c_z == 0: division by zero, out
        ((nan, 0.0, z), None), ((0.0, nan, z), None), ((0.0, 0.0, nan), None),
        ((inf, 0.0, z), None), ((0.0, -inf, z), None), ((0.0, 0.0, inf), None), ((0.0, 0.0, -inf), None),
        ((1e30, 0.0, z), None), ((-1e30, 1e30, z), None), ((3e38, 3e38, 3e38), None),      # u ~ 1e32: out before any conversion
        ((0.0, 0.0, 3e38), (64, 48)),                       # very far but finite and centred: in
    ]
    return np.array([p for p, _ in pts], dtype=np.float32), [e for _, e in pts]


def negzero_case():
    """u = v = -0.0 exactly: every product and sum of the first two pose rows is -0.0, and so are cx and cy.  -> (Cam, points): in view, pixel (0, 0)."""
    pose = np.array([[1, 0, 0, -0.0], [0, 1, 0, -0.0], [0, 0, 1, 3]], dtype=np.float32)
    return Cam(pose=pose, cx=-0.0, cy=-0.0), np.array([[-0.0, -0.0, -2.0]], dtype=np.float32)


def tiny_case():
    """cx = cy = 0: u = 160 x.  A tiny negative u is out, a tiny positive one is in pixel 0.  -> (Cam, points, expected)."""
    pts = np.array([[-1e-30, 0, -2], [1e-30, 0, -2], [0, -1e-30, -2], [-1e-42, 0, -2]], dtype=np.float32)      # the last: a subnormal
    return Cam(cx=0.0, cy=0.0), pts, [None, (0, 0), None, None]


def near_case():
    """A point whose depth is exactly `near` (in), and the same point under a near one ulp larger (out).  -> (points, Cam in, Cam out)."""
    pts = np.array([[0.001, 0.001, -2.99]], dtype=np.float32)
    depth = F(pts[0, 2] + F(3))
    assert 0 < depth < 0.011
    return pts, Cam(near=depth), Cam(near=np.nextafter(depth, F(1)))


def random_bits(K, N, seed=0, zero_rows=(), one_rows=()):
    rng = np.random.default_rng(seed)
    m = rng.random((K, N)) < 0.3
    for r in zero_rows:
        m[r] = False
    for r in one_rows:
        m[r] = True
    return pack(m)
