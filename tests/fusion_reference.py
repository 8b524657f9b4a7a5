"""Plain-numpy reference of the label fusion (include/pointsam_hip.h, "label fusion"), built on the references of the camera views and the RGB-D frames:
the observation is view_reference.project and the lift rule, the rest is integers.  Also the inputs the CPU and the GPU tests share."""
import numpy as np

import frames_reference as R
import view_reference as V

SLOTS = 8


# ------------------------------------------------------------------------------------------------ the definition
def observe(xyz, cam, keys, labels, tau):
    """One view -> (visible [N] bool, label [N] int32: the label at the centre pixel, -1 where the point is not visible)."""
    ok, px, py, depth = V.project(xyz, cam)
    k = keys[py, px]
    with np.errstate(all="ignore"):
        front = (k >> np.uint64(32)).astype(np.uint32).view(np.float32)
        vis = ok & (k != V.EMPTY) & (depth <= front + V.F(tau))
    return vis, np.where(vis, np.asarray(labels, dtype=np.int32)[py, px], np.int32(-1)).astype(np.int32)


def row_base_of(labels):
    """count_v = max(labels[v]) + 1 (0 if no label is >= 0) -> the exclusive prefix [V + 1] int32."""
    counts = [max(int(np.max(l)) + 1, 0) for l in labels]
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def region_bits(xyz, cams, keys, labels, row_base, tau):
    """-> (bits [R + V, Wd] int64, area [R + V] int32)."""
    N, Vn, Rn = len(xyz), len(cams), int(row_base[-1])
    on = np.zeros((Rn + Vn, N), dtype=bool)
    for v in range(Vn):
        vis, lab = observe(xyz, cams[v], keys[v], labels[v], tau)
        count = int(row_base[v + 1]) - int(row_base[v])
        valid = vis & (lab >= 0) & (lab < count)
        on[int(row_base[v]) + lab[valid].astype(np.int64), np.nonzero(valid)[0]] = True
        on[Rn + v] = vis
    return V.pack(on), on.sum(1).astype(np.int32)


def intersections(bits):
    m = V.unpack(bits, bits.shape[1] * 64).astype(np.int64)
    return (m @ m.T).astype(np.int32)


def link_edges(inter, row_base, overlap, min_points):
    """-> the links as a list of (a, b), a < b."""
    Vn, Rn = len(row_base) - 1, int(row_base[-1])
    view_of = np.repeat(np.arange(Vn), np.diff(row_base))
    edges = []
    for a in range(Rn):
        for b in range(a + 1, Rn):
            u, v = view_of[a], view_of[b]
            if u == v or inter[a, a] == 0 or inter[b, b] == 0:
                continue
            n, ca, cb = int(inter[a, b]), int(inter[a, Rn + v]), int(inter[b, Rn + u])
            if min(ca, cb) >= min_points and float(n) >= float(overlap) * float(max(ca, cb)):
                edges.append((a, b))
    return edges


def components(nonempty, edges):
    """nonempty [R] bool, edges (a, b) -> remap [R] int32: components numbered by their smallest row, -1 for an empty region."""
    Rn = len(nonempty)
    comp = np.arange(Rn)
    for _ in range(Rn):                                            # label propagation to the fixed point: the minimum row of the component
        before = comp.copy()
        for a, b in edges:
            comp[a] = comp[b] = min(comp[a], comp[b])
        if (before == comp).all():
            break
    roots = sorted(set(int(comp[r]) for r in range(Rn) if nonempty[r]))
    number = {r: i for i, r in enumerate(roots)}
    return np.array([number[int(comp[r])] if nonempty[r] else -1 for r in range(Rn)], dtype=np.int32)


def link_regions(inter, row_base, overlap, min_points):
    Rn = int(row_base[-1])
    return components(np.diagonal(inter)[:Rn] > 0, link_edges(inter, row_base, overlap, min_points))


def vote(xyz, cams, keys, labels, tau, row_base=None, remap=None, min_votes=1):
    """-> dict(label, votes, seen, labelled, dropped), [N] int32 each.  The table is walked point by point, as the definition reads."""
    N = len(xyz)
    obs = [observe(xyz, cams[v], keys[v], labels[v], tau) for v in range(len(cams))]
    out = {k: np.zeros(N, dtype=np.int32) for k in ("label", "votes", "seen", "labelled", "dropped")}
    for i in range(N):
        table = []                                                 # [label, count] in first-seen order
        for v, (vis, lab) in enumerate(obs):
            if not vis[i]:
                continue
            out["seen"][i] += 1
            g = int(lab[i])
            if row_base is not None:
                if not 0 <= g < int(row_base[v + 1]) - int(row_base[v]):
                    continue
                if remap is not None:
                    g = int(remap[int(row_base[v]) + g])
            if g < 0:
                continue
            out["labelled"][i] += 1
            slot = [s for s in table if s[0] == g]
            if slot:
                slot[0][1] += 1
            elif len(table) < SLOTS:
                table.append([g, 1])
            else:
                out["dropped"][i] += 1
        best = min(table, key=lambda s: (-s[1], s[0])) if table else None
        if best is None or best[1] < min_votes:
            out["label"][i], out["votes"][i] = -1, 0
        else:
            out["label"][i], out["votes"][i] = best
    return out


def label_bits(labels, K):
    on = np.asarray(labels)[None, :] == np.arange(K)[:, None]
    return V.pack(on), on.sum(1).astype(np.int32)


def fuse(xyz, cams, keys, labels, tau, overlap=0.5, min_points=20, min_votes=1, link_xyz=None):
    """The whole pipeline with per-view ids: rows and links on link_xyz (default: xyz), the vote on xyz -> dict(vote outputs, remap, row_base,
    num_instances)."""
    rb = row_base_of(labels)
    bits, _ = region_bits(xyz if link_xyz is None else link_xyz, cams, keys, labels, rb, tau)
    remap = link_regions(intersections(bits), rb, overlap, min_points)
    out = vote(xyz, cams, keys, labels, tau, rb, remap, min_votes)
    out.update(remap=remap, row_base=rb, num_instances=int(remap.max()) + 1 if len(remap) else 0)
    return out


# ------------------------------------------------------------------------------------------------ the shared inputs
def frames_case(depth, rgb, cams, far, edge=None):
    """RGB-D frames -> (xyz [M, 3], the normalised cameras, keys [F, H, W] uint64) of frames_reference.frames."""
    out = R.frames(depth, rgb, cams, far, edge)
    return out["xyz"], out["cams"], out["keys"]


def pattern_labels(shape, count, seed=0):
    """Blocky seeded labels in -1 .. count (count itself is out of range on purpose), with the four extreme values sprinkled in."""
    Fn, H, W = shape
    rng = np.random.default_rng(seed)
    y, x = np.arange(H)[:, None] // 3, np.arange(W)[None, :] // 4
    lab = np.stack([(y * 5 + x * 3 + f) % (count + 2) - 1 for f in range(Fn)]).astype(np.int32)
    flat = lab.reshape(-1)
    flat[rng.random(flat.size) < 0.02] = np.iinfo(np.int32).max
    flat[rng.random(flat.size) < 0.02] = np.iinfo(np.int32).min
    return lab


def tiled_room(times=10):
    """The first frame of the room fixture `times` times over, pose and depth identical -> (depth, rgb, cams, far)."""
    depth, rgb, cams, far = R.room_case()
    return np.repeat(depth[:1], times, 0), np.repeat(rgb[:1], times, 0), [cams[0]] * times, far


RING_OBJECTS = (((-0.45, 0.0, 0.0), 0.3), ((0.45, 0.0, 0.0), 0.3), ((0.0, 0.1, 0.5), 0.25))
RING_FLOOR, RING_TAU = 3, 0.02


def ring_case(split_floor=False):
    """Three sphere shells on a floor, seen by six cameras on a ring; the depth images are rendered from the world and unprojected again, and every
    frame's 2-D labels are the objects of its pixels under a permutation of its own.  split_floor: in odd frames the floor's right image half
    (columns >= 64) gets a fifth id.  -> dict(xyz [M, 3], cams, keys [6, 96, 128] uint64, labels [6, 96, 128] int32, perm [6, 4], obj [M]: the object
    0 .. 3 of every scan point, depth, rgb, cameras (un-normalised), far, edge, center and scale of the normalisation)."""
    shells = [V.sphere_case(6000, r, seed=o) + np.asarray(c, dtype=np.float32) for o, (c, r) in enumerate(RING_OBJECTS)]
    fl = np.random.default_rng(9).uniform(-1, 1, (12000, 2))
    floor = np.stack([fl[:, 0], np.full(12000, 0.35), fl[:, 1]], 1).astype(np.float32)
    world = np.concatenate(shells + [floor]).astype(np.float32)
    world_obj = np.repeat(np.arange(4), [6000, 6000, 6000, 12000]).astype(np.int32)
    from point_sam_amd.views import Camera
    cams = []
    for f in range(6):
        a = 2 * np.pi * f / 6
        c = Camera.look_at((2.6 * np.sin(a), -1.2, 2.6 * np.cos(a)), (0, 0, 0.1), (0, -1, 0), 40, 128, 96, near=0.05)
        cams.append(V.Cam(pose=c.pose_words, fx=c.fx, fy=c.fy, cx=c.cx, cy=c.cy, width=c.width, height=c.height, near=c.near))
    rng = np.random.default_rng(3)
    depth, pix_obj, perm = [], [], []
    for cam in cams:
        k = V.splat(world, cam, 1)
        d = V.depth_of(k)
        d[k == V.EMPTY] = 0.0
        depth.append(d)
        pix_obj.append(np.where(k == V.EMPTY, -1, world_obj[np.where(k == V.EMPTY, 0, V.index_of(k))]))
        perm.append(rng.permutation(4))
    depth, pix_obj, perm = np.stack(depth).astype(np.float32), np.stack(pix_obj).astype(np.int32), np.stack(perm).astype(np.int32)
    rgb = np.zeros(depth.shape + (3,), dtype=np.float32)
    out = R.frames(depth, rgb, cams, 10.0, 0.05)
    labels = np.where(pix_obj >= 0, np.take_along_axis(perm, np.maximum(pix_obj, 0).reshape(6, -1), 1).reshape(pix_obj.shape), -1).astype(np.int32)
    if split_floor:
        right = (pix_obj == RING_FLOOR) & (np.arange(128)[None, None, :] >= 64) & (np.arange(6)[:, None, None] % 2 == 1)
        labels[right] = 4
    obj = np.zeros(out["M"], dtype=np.int32)
    obj[out["index"][out["index"] >= 0]] = pix_obj[out["index"] >= 0]
    return dict(xyz=out["xyz"], cams=out["cams"], keys=out["keys"], labels=labels, perm=perm, obj=obj, depth=depth, rgb=rgb, cameras=cams, far=10.0,
                edge=0.05, center=out["center"], scale=out["scale"])


def entry_point_refusals(lib, p):
    """Every refusal of the three C entry points, with `p` a non-null pointer aligned to 16 bytes: each call must be refused with its status and a
    message naming the reason, before any launch -- what p points at is never touched.  The CPU test passes host memory, the GPU test device memory
    whose contents it compares afterwards."""
    nan, inf = float("nan"), float("inf")

    def refused(status, code, word):
        assert status == code, (status, lib.psam_last_error_string())
        assert word in lib.psam_last_error_string(), lib.psam_last_error_string()

    good = dict(xyz=p, N=100, cameras=p, V=2, H=24, W=43, keys=p, labels=p, row_base=p, R=5, tau=0.0, bits=p, area=p)
    region = lambda **kw: lib.psam_fuse_region_bits(*{**good, **kw}.values(), None)
    for name in ("xyz", "cameras", "keys", "labels", "row_base", "bits"):
        refused(region(**{name: None}), -1, b"null")
    for bad in (0, -1, (1 << 28) + 1):
        refused(region(N=bad), -1, b"2^28")
    for kw in (dict(V=0), dict(V=-1), dict(V=4097), dict(H=0), dict(W=0), dict(H=8193), dict(W=8193)):
        refused(region(**kw), -1, b"4096")
    for bad in (-1, (1 << 20) + 1):
        refused(region(R=bad), -1, b"region rows")
    for bad in (-0.5, -inf, nan):
        refused(region(tau=bad), -1, b"tau")
    for kw in (dict(keys=p + 4), dict(bits=p + 4), dict(xyz=p + 2), dict(cameras=p + 1), dict(labels=p + 2), dict(row_base=p + 2), dict(area=p + 2)):
        refused(region(**kw), -2, b"aligned")

    good = dict(xyz=p, N=100, cameras=p, V=2, H=24, W=43, keys=p, labels=p, row_base=p, remap=p, R=5, tau=0.0, min_votes=1, label=p, votes=p, seen=p,
                labelled=p, dropped=p)
    vote_ = lambda **kw: lib.psam_fuse_vote(*{**good, **kw}.values(), None)
    for name in ("xyz", "cameras", "keys", "labels", "label", "votes", "seen", "labelled", "dropped"):
        refused(vote_(**{name: None}), -1, b"null")
    refused(vote_(row_base=None), -1, b"remap needs")
    for bad in (0, -1, (1 << 28) + 1):
        refused(vote_(N=bad), -1, b"2^28")
    for kw in (dict(V=0), dict(V=4097), dict(H=0), dict(W=8193)):
        refused(vote_(**kw), -1, b"4096")
    refused(vote_(R=-1), -1, b"region rows")
    for bad in (-1e-9, nan):
        refused(vote_(tau=bad), -1, b"tau")
    for bad in (0, -3):
        refused(vote_(min_votes=bad), -1, b"min_votes")
    for name in ("keys", "xyz", "cameras", "labels", "row_base", "remap", "label", "votes", "seen", "labelled", "dropped"):
        refused(vote_(**{name: p + (4 if name == "keys" else 2)}), -2, b"aligned")

    good = dict(labels=p, N=100, K=3, bits=p, area=p)
    rows = lambda **kw: lib.psam_label_bits(*{**good, **kw}.values(), None)
    for name in ("labels", "bits"):
        refused(rows(**{name: None}), -1, b"null")
    for bad in (0, -1, (1 << 28) + 1):
        refused(rows(N=bad), -1, b"2^28")
    for bad in (0, -1, (1 << 20) + 1):
        refused(rows(K=bad), -1, b"K")
    for kw in (dict(bits=p + 4), dict(labels=p + 2), dict(area=p + 1)):
        refused(rows(**kw), -2, b"aligned")


def ring_disagreement(label, remap, row_base, perm, obj):
    """How many points carry an instance other than their object's: the instance of object o is the one most frames' region (f, perm[f][o]) maps to."""
    inst = []
    for o in range(4):
        ids = [int(remap[int(row_base[f]) + int(perm[f][o])]) for f in range(len(perm))]
        ids = [g for g in ids if g >= 0]
        inst.append(max(set(ids), key=ids.count) if ids else -1)
    return int((np.asarray(label) != np.asarray(inst, dtype=np.int32)[obj]).sum())
