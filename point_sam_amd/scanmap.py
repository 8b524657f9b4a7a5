"""Scan maps: posed scans accumulate into one persistent, labelled voxel map (csrc/scanmap.hip, predictor.map_add / map_lookup).

A walk through a room gives fifty scans, each with the masks propagate() or fuse_labels() gave it; a `ScanMap` holds them together.  It lives in the
common normalised frame ([-1, 1]^3, the same centre and scale for every scan), and its voxels are those of set_scene(voxel_size=h): every add puts each
accepted point of a scan, under the scan's pose, into its voxel, and the voxel keeps exact integer sums of positions and colours and one count per
instance label seen there.  Out of it come

    cloud()     one denoised cloud: the mean position and mean colour per voxel;
    labels()    one instance label per voxel, voted over everything ever seen there (ties to the lower label);
    ids         voxel ids that never change: a voxel keeps the id its first add gave it, so packed masks over the map (bits()) stay valid as it grows.

Every sum is an integer, so every output is the same bits from run to run and for any order of the points inside an add (ids follow the order).  The
definition is in include/pointsam_hip.h ("scan map"); tests/scanmap_reference.py states it again in numpy.

Overflow is an error, never a silent drop: an add that would take the map past max_voxels, or its distinct (voxel, label) pairs past max_pairs,
raises MapOverflow, and so does every later call until clear().

Free space (csrc/carve.hip): carve() walks the ray from the sensor's cell to the cell of every point of a scan and counts, per voxel and per carve,
whether the voxel held a point (a hit) or was seen through (a miss); occupied() reads the two counts.  What walked through the room once -- a person,
a chair since moved, depth noise at an edge -- is then voted free, and cloud()[occupied()] shows no ghosts.  The walk is exact integer arithmetic
between cell centres (at most half a voxel off the true ray); the counts live in a second block, and the map's own block is never written by a carve.

Tracking (csrc/track.hip): the poses of a walk are otherwise frame to frame, and their errors add up.  track() registers a scan against the MAP, the one
object that has seen the whole walk: align.icp's loop, where a step (track_step) pairs every point of the scan with the nearest map voxel -- its
mean position, cloud()'s bits -- by probing the map's own voxel table.  No cloud is read out and no index is built; the step sums ops.align_step's
twenty words, so the solve and the loop are align.py's unchanged.

Point to plane (csrc/map_normals.hip, track.hip): a room is floors, walls and table tops, and a scan slides along a plane of voxel means.  normals() gives
every voxel a normal from the means of the voxels around it -- an exact integer scatter matrix, probed out of the map's own table -- and
track(normals=True) minimises the distance to the pair's tangent plane instead: track_plane_step sums ops.align_plane_step's thirty-two words over
track_step's pairs, and the loop and solve are align.icp's point-to-plane ones unchanged.  Normals are not kept: they describe the map at the time of
the call, and the caller asks again after an add.

Relocalisation (csrc/track_score.hip): track() refines a pose that is within a few voxels of the truth; a walk whose odometry dropped out, a second
session in a room mapped yesterday or a scan that starts elsewhere in the map has none.  relocalize(xyz, cfg, SearchConfig) is align.search with the map in
place of the index: track_score counts, for every pose of a grid at once, the sampled points that land within a radius of a pairable voxel's mean --
exactly track_step's pair count under that pose, with the same occupied / min_count, so ghosts do not attract -- the best few are refined by the loop
above and the refinement with the most pairs wins.  anchors() lists where a scan may land in a map larger than itself (the centres of the map's
coarse cells), for SearchConfig(anchors=...).

Views (csrc/map_view.hip): view(camera) casts one ray per pixel from the camera's cell through the map's own table -- carve()'s exact integer walk,
ended by the first pairable voxel instead of by a measured point -- and returns a views.View whose keys hold the VOXEL ID and the depth of its mean:
the map drawn without the holes and the bleed-through of point splats of cloud(), with occupied / min_count honoured, and a predicted depth image.
Every reader of a rendered scan's keys (ops.view_pick, ops.view_paint_ids, View.colour) takes it unchanged; label_image() is labels() per pixel.

Not built: removing or decaying voxels (occupied() is a read-out; a freed voxel keeps its id, sums and votes), rays from an origin outside
[-1, 1]^3 (carve()'s sensor and view()'s eye alike), a far limit for view(), sub-voxel rays from the true eye (every ray of a view starts at the centre
of the eye's cell), shading a view by the map's normals, skipping whole empty bricks of a view's walk instead of only their lookups, TSDF surfaces, maps beyond [-1, 1]^3, soft votes, pose-graph optimisation (track() places a scan against the map, it does not go back and
move the scans already added), a multi-resolution or branch-and-bound search (the grid of relocalize() is scored pose by pose at one resolution),
scoring on a coarser copy of the map, a search that reaches more than 4 voxels from a query's own, a viewpoint sign for map normals (the sign is the largest component's),
normals kept in the block and updated per add, a normal neighbourhood that reaches more than 2 cells, a switch for point-to-plane in the demo
server.  No default here has been
tuned on real scans or a trained checkpoint.  Beyond the voxel and pair capacities a map takes at most 2^31 - 1 accepted points in all (the bound that
keeps counts and votes in int32 and every sum in one 64-bit word); that refusal is not exercised by any test.
"""
from dataclasses import dataclass

import torch

from . import ops


class MapOverflow(RuntimeError):
    """An add went past the map's max_voxels or max_pairs (or 2^31 - 1 accepted points in all): the map is dead until clear()."""


@dataclass
class AddResult:
    ids: torch.Tensor         # [M] int32: the voxel of every accepted point, -1 for a rejected one
    new_voxels: int
    accepted: int
    rejected: int


@dataclass
class MapNormals:
    normal: torch.Tensor      # [V, 3] f32: unit, the largest component positive; (0, 0, 0) without enough neighbours
    curvature: torch.Tensor   # [V] f32: l0 / (l0 + l1 + l2) of the neighbourhood's scatter matrix
    count: torch.Tensor       # [V] int32: the voxels of the neighbourhood, the voxel itself among them; 0 for a voxel that is not allowed


@dataclass
class CarveResult:
    rays: int                 # distinct endpoint cells other than the origin's
    accepted: int
    rejected: int
    hit_voxels: int           # voxels whose hits this carve raised
    missed_voxels: int        # voxels whose misses this carve raised
    crossed: int              # cells crossed beyond the margin, summed over the rays: a function of the inputs


def occupied_from_counts(hits: torch.Tensor, misses: torch.Tensor, min_misses: int = 2, num: int = 1, den: int = 1) -> torch.Tensor:
    """not free, free iff misses >= min_misses and misses * den > hits * num, in int64.  Plain torch."""
    h, m = hits.to(torch.int64), misses.to(torch.int64)
    return ~((m >= min_misses) & (m * den > h * num))


def labels_from_logits(logits: torch.Tensor, ids=None, threshold: float = 0.0) -> torch.Tensor:
    """logits [K, M] float32, ids [K] integers (None: 0 .. K - 1), threshold -> [M] int32: per point ids[argmax over k] where the column's maximum is
    > threshold, else -1.  A NaN or -inf never wins: rows of propagate()'s lost objects take no point.  Plain torch."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError(f"labels_from_logits: logits must be a [K, M] tensor with K, M >= 1, got "
                         f"{tuple(logits.shape) if isinstance(logits, torch.Tensor) else type(logits).__name__}")
    if logits.dtype != torch.float32:
        raise TypeError(f"labels_from_logits: logits of float32, got {logits.dtype}")
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or threshold != threshold:
        raise ValueError(f"labels_from_logits: threshold must be a number, got {threshold!r}")
    K = logits.shape[0]
    if ids is not None:
        ids = torch.as_tensor(ids)
        if ids.dtype not in (torch.int32, torch.int64) or tuple(ids.shape) != (K,):
            raise ValueError(f"labels_from_logits: ids must be [{K}] integers, got {tuple(ids.shape)} {ids.dtype}")
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) > 2 ** 31 - 1):
            raise ValueError("labels_from_logits: ids must lie in 0 .. 2^31 - 1")
        ids = ids.to(device=logits.device, dtype=torch.int32)
    clean = torch.where(torch.isnan(logits), torch.full_like(logits, float("-inf")), logits)
    best, arg = clean.max(dim=0)
    label = arg.to(torch.int32) if ids is None else ids.index_select(0, arg)
    return torch.where(best > threshold, label, torch.full_like(label, -1)).contiguous()


def _overflow_message(flags: int, max_voxels: int, max_pairs: int) -> str:
    why = []
    if flags & ops.MAP_FLAG_VOXELS:
        why.append(f"more than max_voxels = {max_voxels} voxels")
    if flags & ops.MAP_FLAG_PAIRS:
        why.append(f"more than max_pairs = {max_pairs} (voxel, label) pairs")
    if flags & ops.MAP_FLAG_COUNTS:
        why.append("more than 2^31 - 1 accepted points in all")
    return "ScanMap: " + " and ".join(why or [f"flags {flags}"]) + ": the map is dead until clear()"


class ScanMap:
    """ScanMap(voxel_size, max_voxels, max_pairs=None (2 * max_voxels), device="cuda").  The arguments are checked before any device work; the block
    (ops.map_bytes) is allocated once and cleared."""

    def __init__(self, voxel_size, max_voxels: int, max_pairs: int = None, device="cuda"):
        ops.map_inv_h(voxel_size)
        self.max_voxels, self.max_pairs = ops.map_capacities(max_voxels, max_pairs)
        self.voxel_size = float(voxel_size)
        self._block = torch.empty(ops.map_bytes(self.max_voxels, self.max_pairs) // 8 + 2, dtype=torch.int64, device=device)
        self._V = self._adds = self._flags = 0
        self._carve, self._carves = None, 0                        # the carve block: allocated by the first carve()
        self.clear()

    # -- state ---------------------------------------------------------------------------------------------
    @property
    def num_voxels(self) -> int:
        return self._V

    @property
    def num_adds(self) -> int:
        return self._adds

    @property
    def device(self):
        return self._block.device

    def clear(self) -> None:
        """Empties the map and its carve block; a dead map lives again."""
        ops.map_clear(self._block, self.max_voxels, self.max_pairs, self.voxel_size)
        self._V = self._adds = self._flags = 0
        if self._carve is not None:
            ops.carve_clear(self._carve, self.max_voxels)
        self._carves = 0

    def _alive(self, what: str):
        if self._flags:
            raise MapOverflow(f"{what}: " + _overflow_message(self._flags, self.max_voxels, self.max_pairs))
        return self._block, self.max_voxels, self.max_pairs

    def _filled(self, what: str):
        lead = self._alive(what)
        if self._V == 0:
            raise ValueError(f"{what}: the map is empty")
        return lead + (self._V,)

    # -- growing -------------------------------------------------------------------------------------------
    @torch.no_grad()
    def add(self, xyz: torch.Tensor, rgb: torch.Tensor, labels: torch.Tensor = None, pose=None) -> AddResult:
        """One scan: xyz, rgb [M, 3] f32, labels [M] int32 or None (a negative label is an unlabelled observation), pose 3 x 4 or 4 x 4 from the
        scan's frame to the map's, or None.  One host read, of the map's header.  MapOverflow past a capacity."""
        lead = self._alive("add")
        ids, header = ops.map_add(*lead, xyz, rgb, labels, pose)
        self._flags = header[ops.MAP_H_FLAGS]
        if self._flags:
            raise MapOverflow("add: " + _overflow_message(self._flags, self.max_voxels, self.max_pairs))
        self._V, self._adds = header[ops.MAP_H_V], header[ops.MAP_H_ADDS]
        return AddResult(ids, header[ops.MAP_H_NEW], header[ops.MAP_H_ACCEPTED], header[ops.MAP_H_REJECTED])

    # -- reading -------------------------------------------------------------------------------------------
    @torch.no_grad()
    def locate(self, xyz: torch.Tensor, pose=None) -> torch.Tensor:
        """ids [M] int32 of xyz under the pose: -1 where the map has no such voxel or the position is not accepted.  No host read."""
        return ops.map_locate(*self._alive("locate"), xyz, pose)

    @torch.no_grad()
    def labels(self, min_votes: int = 1):
        """(label [V] int32, votes [V] int32); -1 and 0 where the best count is below min_votes."""
        return ops.map_labels(*self._filled("labels"), min_votes)

    @torch.no_grad()
    def cloud(self):
        """(xyz [V, 3] f32, rgb [V, 3] f32): the voxels' mean positions and colours -- a scan like any other."""
        return ops.map_cloud(*self._filled("cloud"))

    def _fields(self, what: str):
        return ops.map_fields(*self._filled(what))

    def counts(self) -> torch.Tensor:
        return self._fields("counts")[0]

    def first_seen(self) -> torch.Tensor:
        return self._fields("first_seen")[1]

    def last_seen(self) -> torch.Tensor:
        return self._fields("last_seen")[2]

    def keys(self) -> torch.Tensor:
        return self._fields("keys")[3]

    def sums(self):
        """(sum_q [V, 3] int64, sum_c [V, 3] int64): the exact fixed-point sums behind cloud(), q = floor(v * 2^20) + 2^20 per observation."""
        s = self._fields("sums")[4]
        return s[:, :3], s[:, 3:]

    # -- carving (csrc/carve.hip) ---------------------------------------------------------------------------
    @property
    def num_carves(self) -> int:
        return self._carves

    @torch.no_grad()
    def carve(self, xyz: torch.Tensor, origin, pose=None, margin: int = 1) -> CarveResult:
        """Clears the free space a scan saw through: xyz [M, 3] f32 and pose as add()'s, origin = the sensor's position in the scan's frame (three
        numbers).  Every map voxel that holds a point of the scan is hit; every map voxel that a ray from the origin's cell to a point's cell
        crosses, more than `margin` cells (Chebyshev) before the ray's end and not itself hit by this scan, is missed.  Each counts once per carve:
        hits() counts CARVES, not points, so carve a map from its first scan on -- a voxel added without a carve has hits = 0.  Rays run from cell
        centre to cell centre, at most half a voxel off the true ray.  The map itself is never written.  ValueError before any launch for an origin
        that lands outside [-1, 1]^3; MapOverflow for a dead map.  One 64-byte host read, the carve block's header; the block (ops.carve_bytes) is
        allocated by the first carve."""
        lead = self._alive("carve")
        ops.carve_origin(origin, pose, self.voxel_size)
        if self._carve is None:
            self._carve = torch.empty(ops.carve_bytes(self.max_voxels) // 8, dtype=torch.int64, device=self.device)
            ops.carve_clear(self._carve, self.max_voxels)
        h = ops.carve_scan(*lead, self._carve, xyz, origin, pose, margin, self._carves + 1)
        self._carves = h[ops.CARVE_H_CARVES]
        return CarveResult(h[ops.CARVE_H_RAYS], h[ops.CARVE_H_ACCEPTED], h[ops.CARVE_H_REJECTED], h[ops.CARVE_H_HIT], h[ops.CARVE_H_MISSED],
                           h[ops.CARVE_H_CROSSED])

    def _carve_fields(self, what: str):
        block, max_voxels, _, V = self._filled(what)
        if self._carve is None:                                    # never carved: nothing was ever seen through
            return tuple(torch.zeros(4, V, dtype=torch.int32, device=self.device))
        return ops.carve_fields(self._carve, max_voxels, V)

    def hits(self) -> torch.Tensor:
        """[V] int32: the carves in which the voxel held a point."""
        return self._carve_fields("hits")[0]

    def misses(self) -> torch.Tensor:
        """[V] int32: the carves in which a ray passed through the voxel and no point of that scan lay in it."""
        return self._carve_fields("misses")[1]

    def last_hit(self) -> torch.Tensor:
        """[V] int32: the number of the last carve that hit the voxel (from 1), 0 for none."""
        return self._carve_fields("last_hit")[2]

    def last_missed(self) -> torch.Tensor:
        return self._carve_fields("last_missed")[3]

    @torch.no_grad()
    def occupied(self, min_misses: int = 2, num: int = 1, den: int = 1) -> torch.Tensor:
        """[V] bool.  A voxel is FREE iff misses >= min_misses and misses * den > hits * num (int64): seen through at least min_misses times, and
        more than num / den times as often as it was hit.  Before any carve everything is occupied.  hits counts carves, not points (carve())."""
        for name, v, lo in (("min_misses", min_misses, 0), ("num", num, 0), ("den", den, 1)):
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= 2 ** 31 - 1:
                raise ValueError(f"occupied: {name} must be an integer in {lo} .. 2^31 - 1, got {v!r}")
        hits, misses = self._carve_fields("occupied")[:2]
        return occupied_from_counts(hits, misses, min_misses, num, den)

    def bits(self, K: int):
        """ops.label_bits of labels(): (bits [K, ceil(V / 64)] int64, area [K] int32), row k the voxels voted k."""
        return ops.label_bits(self.labels()[0].contiguous(), K)

    # -- tracking (csrc/track.hip) ---------------------------------------------------------------------------
    @torch.no_grad()
    def track_step(self, xyz: torch.Tensor, pose=None, radius=None, bits: torch.Tensor = None, skip: torch.Tensor = None, min_count: int = 1,
                   return_nearest: bool = False):
        """One ICP step of a scan against the map (ops.track_step): xyz [M, 3] f32, pose from the scan's frame to the map's -> sums [20] float64 on
        the device, ops.align_step's words over the pairs (point, nearest voxel mean within `radius` of the posed point; None: the voxel size), and
        with return_nearest the voxel id per point, -1 without a pair.  bits: a packed row over the points that take part; skip: a packed row over
        voxel ids that are never paired; min_count: the fewest observations of a voxel that is.  MapOverflow for a dead map, ValueError for an empty
        one.  No host read."""
        block, max_voxels, max_pairs, V = self._filled("track_step")
        return ops.track_step(block, max_voxels, max_pairs, V, xyz, pose, radius, bits, skip, min_count, return_nearest, voxel_size=self.voxel_size)

    def _skip(self, what: str, occupied, V: int):
        """occupied (None, True or a [V] bool tensor) -> the packed row of the voxels that are NOT, or None."""
        if occupied is None:
            return None
        if occupied is True:
            occupied = self.occupied()
        if occupied.dtype != torch.bool or tuple(occupied.shape) != (V,) or occupied.device != self.device:
            raise ValueError(f"{what}: occupied must be [{V}] bool on {self.device}, got {tuple(occupied.shape)} {occupied.dtype} on {occupied.device}")
        return ops.mask_pack((~occupied).to(torch.float32)[None].contiguous(), 0.5, 0.0)[0][0]

    @torch.no_grad()
    def normals(self, reach: int = 1, min_voxels: int = 5, occupied=None, min_count: int = 1) -> MapNormals:
        """One normal per voxel (ops.map_normals): the eigenvector of the smallest eigenvalue of the exact scatter matrix of the means of the voxels in
        the (2 reach + 1)^3 cells around it, reach 1 or 2; (0, 0, 0) where fewer than min_voxels are there.  occupied (None, True or a [V] bool
        tensor, as track()'s) and min_count say which voxels count: one that does not has no normal and enters no other's.  Nothing is kept: the
        normals describe the map at the time of the call.  MapOverflow for a dead map, ValueError for an empty one.  No host read."""
        if occupied is not None and occupied is not True and not isinstance(occupied, torch.Tensor):
            raise TypeError(f"normals: occupied must be None, True or a [V] bool tensor, got {type(occupied).__name__}")
        block, max_voxels, max_pairs, V = self._filled("normals")
        count, normal, curvature = ops.map_normals(block, max_voxels, max_pairs, V, reach, min_voxels, self._skip("normals", occupied, V), min_count)
        return MapNormals(normal, curvature, count)

    @torch.no_grad()
    def track_plane_step(self, xyz: torch.Tensor, normals: torch.Tensor, pose=None, radius=None, bits: torch.Tensor = None, skip: torch.Tensor = None,
                         min_count: int = 1, return_nearest: bool = False):
        """One point-to-plane ICP step of a scan against the map (ops.track_plane_step): track_step's arguments and pairs, and normals [V, 3] f32, one
        per voxel id (normals().normal) -> sums [32] float64 on the device, ops.align_plane_step's words.  MapOverflow for a dead map, ValueError
        for an empty one.  No host read."""
        block, max_voxels, max_pairs, V = self._filled("track_plane_step")
        return ops.track_plane_step(block, max_voxels, max_pairs, V, xyz, normals, pose, radius, bits, skip, min_count, return_nearest,
                                    voxel_size=self.voxel_size)

    # -- relocalisation (csrc/track_score.hip) ----------------------------------------------------------------
    @torch.no_grad()
    def track_score(self, xyz: torch.Tensor, poses, radius=None, skip: torch.Tensor = None, min_count: int = 1) -> torch.Tensor:
        """The score of a grid of poses (ops.track_score): xyz [M, 3] f32, poses [P, 3, 4] / [P, 4, 4] host numbers or a [P, 12] float32 device tensor
        (ops.align_score's forms), scan frame -> map frame -> counts [P] int32 on the device: under pose p the points with at least one map voxel
        within `radius` (None: the voxel size), int(track_step(xyz, pose_p, radius, None, skip, min_count)[0]) for every p from one call.
        MapOverflow for a dead map, ValueError for an empty one.  No host read."""
        block, max_voxels, max_pairs, V = self._filled("track_score")
        return ops.track_score(block, max_voxels, max_pairs, V, xyz, poses, radius, skip, min_count, voxel_size=self.voxel_size)

    def _pairable(self, what: str, occupied, min_count, V: int) -> torch.Tensor:
        """[V] bool: the voxels track() may pair under `occupied` (None, True or a [V] bool tensor) and `min_count`."""
        min_count = ops._superpoint_int(min_count, 1, 2 ** 31 - 1, f"{what}: min_count")
        if occupied is not None and occupied is not True and not isinstance(occupied, torch.Tensor):
            raise TypeError(f"{what}: occupied must be None, True or a [V] bool tensor, got {type(occupied).__name__}")
        if occupied is True:
            occupied = self.occupied()
        if occupied is not None and (occupied.dtype != torch.bool or tuple(occupied.shape) != (V,) or occupied.device != self.device):
            raise ValueError(f"{what}: occupied must be [{V}] bool on {self.device}, got {tuple(occupied.shape)} {occupied.dtype} on {occupied.device}")
        ok = self.counts() >= min_count
        return ok if occupied is None else ok & occupied

    @torch.no_grad()
    def anchors(self, cells: int = 8, occupied=None, min_count: int = 1, min_voxels: int = 8):
        """Where a scan may land in a map larger than itself -> [A, 3] float64 on the host, for align.SearchConfig(anchors=...): the pairable voxels
        (occupied, min_count: track()'s) grouped by coarse cell -- each coordinate of the voxel's cell (keys(): cx | cy << 21 | cz << 42)
        integer-divided by `cells` -- and per coarse cell with at least min_voxels of them the fp64 mean of their means (summed in id order), ordered
        by coarse (cz, cy, cx).  Plain torch and one host read.  MapOverflow for a dead map, ValueError for an empty one or bad arguments."""
        V = self._filled("anchors")[3]
        _anchor_arguments(cells, min_voxels)
        ok = self._pairable("anchors", occupied, min_count, V)
        return anchors_from_voxels(self.keys(), self.cloud()[0], ok, cells, min_voxels)

    @torch.no_grad()
    def track(self, xyz: torch.Tensor, cfg, init=None, bits: torch.Tensor = None, occupied=None, min_count: int = 1, normals=None, plane=None):
        """The pose of a scan against the map, by ICP -> align.Alignment; its `pose` maps the scan's frame to the map's: what add() and carve() take.
        Exactly align.icp(self, xyz, cfg, init, bits, step=...) with track_step as the step: cfg an align.AlignConfig whose radius is at most 4 voxels
        (ops.track_reach; ValueError before any launch), init the pose to refine (odometry, or the last scan's pose).  occupied: None, True
        (self.occupied()) or a [V] bool tensor: only those voxels are paired (a scan is not pulled towards ghosts); the mask is packed once.  One
        160-byte host read per step.
        normals: None = point to point, as above.  True = point to plane on self.normals(occupied=occupied, min_count=min_count).normal, computed
        once before the loop; a [V, 3] f32 tensor on the map's device is used as given (ValueError before any launch for anything else).  The run
        is then align.icp's point-to-plane loop with track_plane_step as the step: one 256-byte host read per step, align.solve_plane, and
        `plane` an align.PlaneConfig (None: the defaults; without normals a ValueError)."""
        return self._register("track", xyz, cfg, init, None, bits, occupied, min_count, normals, plane)

    @torch.no_grad()
    def relocalize(self, xyz: torch.Tensor, cfg, search, bits: torch.Tensor = None, occupied=None, min_count: int = 1, normals=None, plane=None):
        """The pose of a scan against the map WITHOUT a pose to refine (odometry dropped out, a second session, a scan from elsewhere in the map)
        -> align.Alignment, its `search` the align.SearchRecord.  track()'s arguments with `search`, an align.SearchConfig, in the place of `init`:
        the search IS the start.  Exactly align.search with the map in place of the index -- its score is track_score at search.radius (None:
        cfg.radius; at most cfg.radius, and both pass ops.track_reach before any launch), its refinement track()'s loop with the same skip,
        min_count, normals and plane, its source centroid the fp64 mean of the pairable voxels' means.  On a map larger than the scan give
        SearchConfig(anchors=self.anchors(...))."""
        from . import align as A
        if not isinstance(search, A.SearchConfig):
            raise TypeError(f"relocalize: search must be an align.SearchConfig, got {type(search).__name__}")
        return self._register("relocalize", xyz, cfg, None, search, bits, occupied, min_count, normals, plane)

    # -- views (csrc/map_view.hip) -----------------------------------------------------------------------------
    @torch.no_grad()
    def view(self, camera, occupied=None, min_count: int = 1):
        """The map as `camera` (a views.Camera, its pose from the map's frame to the camera's) sees it from inside -> views.View with num_points =
        num_voxels and splat = 0: its keys hold, per pixel, the depth and the ID of the first voxel the pixel's ray meets (ops.map_view), so
        view.index is a voxel id per pixel and view.depth the predicted depth image; ops.view_pick, ops.view_paint_ids / _rows on bits(K), and
        view.colour(cloud()[1]) take it as they take a rendered scan.  occupied (None, True or a [V] bool tensor) and min_count: track()'s -- a voxel
        that is not pairable is seen through, so ghosts are not drawn.  Rays start at the centre of the eye's cell (at most half a voxel from the
        true eye).  ValueError before any launch for a camera whose centre lies outside [-1, 1]^3 or an empty map, MapOverflow for a dead one.  No
        host read (occupied=True reads the carve block on the device)."""
        from .views import View
        ops.map_view_eye(camera, self.voxel_size)
        if occupied is not None and occupied is not True and not isinstance(occupied, torch.Tensor):
            raise TypeError(f"view: occupied must be None, True or a [V] bool tensor, got {type(occupied).__name__}")
        block, max_voxels, max_pairs, V = self._filled("view")
        keys = ops.map_view(block, max_voxels, max_pairs, V, camera, self._skip("view", occupied, V), min_count, voxel_size=self.voxel_size)
        return View(keys, camera, V, 0)

    @torch.no_grad()
    def label_image(self, view, min_votes: int = 1) -> torch.Tensor:
        """view (ScanMap.view of this map as it is now) -> [height, width] int32: labels(min_votes)[0] at every pixel's voxel, -1 on an empty pixel
        and on a voxel without a label of min_votes votes.  Plain torch."""
        from .views import check_view
        V = self._filled("label_image")[3]
        idx = check_view(view, V, "label_image").index
        label = self.labels(min_votes)[0]
        return torch.where(idx >= 0, label.index_select(0, idx.reshape(-1).clamp_min(0).long()).reshape(idx.shape), torch.full_like(idx, -1)).contiguous()

    def _register(self, what: str, xyz, cfg, init, search, bits, occupied, min_count, normals, plane):
        """track (search None) and relocalize (init None): one set of checks, one pair of step closures, align.icp or align.search around them."""
        from . import align as A
        if not isinstance(cfg, A.AlignConfig):
            raise TypeError(f"{what}: cfg must be an align.AlignConfig, got {type(cfg).__name__}")
        ops.track_reach(cfg.radius, self.voxel_size)
        if search is not None and search.radius is not None:
            ops.track_reach(search.radius, self.voxel_size)
            if search.radius > cfg.radius:
                raise ValueError(f"{what}: the scoring radius {search.radius} exceeds the AlignConfig's {cfg.radius}")
        if occupied is not None and occupied is not True and not isinstance(occupied, torch.Tensor):
            raise TypeError(f"{what}: occupied must be None, True or a [V] bool tensor, got {type(occupied).__name__}")
        V = self._filled(what)[3]
        if normals is None:
            if plane is not None:
                raise ValueError(f"{what}: plane configures point-to-plane tracking and needs normals")
        elif normals is not True and not (isinstance(normals, torch.Tensor) and normals.dtype == torch.float32 and tuple(normals.shape) == (V, 3) and
                                          normals.device == self.device):
            raise ValueError(f"{what}: normals must be None, True or a [{V}, 3] float32 tensor on {self.device}, got "
                             f"{(tuple(normals.shape), normals.dtype, normals.device) if isinstance(normals, torch.Tensor) else repr(normals)}")
        elif plane is not None and not isinstance(plane, A.PlaneConfig):
            raise TypeError(f"{what}: plane must be an align.PlaneConfig or None, got {type(plane).__name__}")
        if occupied is True:
            occupied = self.occupied()                             # read once, for the normals and for the pairs
        skip = self._skip(what, occupied, V)
        if search is not None:
            sources = _SearchSources(self.cloud()[0][self._pairable(what, occupied, min_count, V)])

            def score(_, points, poses, radius):
                return self.track_score(points, poses, radius, skip, min_count)
        if normals is not None:
            if normals is True:
                normals = self.normals(occupied=occupied, min_count=min_count).normal

            def plane_step(_, points, nrm, pose, radius, row):
                return self.track_plane_step(points, nrm, pose, radius, row, skip, min_count)
            if search is not None:
                return A.search(sources, xyz, search, cfg, bits, score=score, step=plane_step, normals=normals.contiguous(), plane=plane)
            return A.icp(self, xyz, cfg, init, bits, step=plane_step, normals=normals.contiguous(), plane=plane)

        def step(_, points, pose, radius, row):
            return self.track_step(points, pose, radius, row, skip, min_count)
        if search is not None:
            return A.search(sources, xyz, search, cfg, bits, score=score, step=step)
        return A.icp(self, xyz, cfg, init, bits, step=step)


class _SearchSources:
    """What align.search reads of its `index` when score and step are stand-ins: src_xyz, for the source centroid."""

    def __init__(self, src_xyz: torch.Tensor):
        self.src_xyz = src_xyz


def _anchor_arguments(cells, min_voxels) -> None:
    for name, v, hi in (("cells", cells, 1 << 21), ("min_voxels", min_voxels, 1 << 28)):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= hi:
            raise ValueError(f"anchors: {name} must be an integer in 1 .. {hi}, got {v!r}")


def anchors_from_voxels(keys: torch.Tensor, xyz: torch.Tensor, ok: torch.Tensor, cells: int = 8, min_voxels: int = 8):
    """ScanMap.anchors' arithmetic on any device: keys [V] int64 (cx | cy << 21 | cz << 42), xyz [V, 3] f32 the voxels' means, ok [V] bool the voxels
    that count -> [A, 3] float64 numpy.  The coarse cell of a voxel is (cx // cells, cy // cells, cz // cells); a coarse cell with at least
    min_voxels counted voxels gives one anchor, the fp64 sum of their means taken in id order, divided by their number; the anchors are ordered by
    coarse (cz, cy, cx).  One host read: the counted voxels' means and coarse codes in one array."""
    import numpy as np
    _anchor_arguments(cells, min_voxels)
    V = keys.shape[0]
    if keys.dtype != torch.int64 or keys.dim() != 1 or tuple(xyz.shape) != (V, 3) or xyz.dtype != torch.float32 or tuple(ok.shape) != (V,) or \
            ok.dtype != torch.bool:
        raise ValueError("anchors: keys [V] int64, xyz [V, 3] float32 and ok [V] bool are needed")
    low = (1 << 21) - 1
    coarse = [torch.div((keys >> (21 * a)) & low, cells, rounding_mode="floor") for a in range(3)]
    code = (coarse[2] << 42) | (coarse[1] << 21) | coarse[0]       # sorts as (cz, cy, cx)
    rows = torch.cat([xyz.double(), code.view(torch.float64)[:, None]], 1)[ok].cpu().numpy()      # the code's bits ride along as a float64 word
    if len(rows) == 0:
        return np.zeros((0, 3))
    _, inverse, count = np.unique(np.ascontiguousarray(rows[:, 3]).view(np.int64), return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    total = np.stack([np.bincount(inverse, weights=rows[:, a], minlength=len(count)) for a in range(3)], 1)      # sequential: id order
    keep = count >= min_voxels
    return total[keep] / count[keep, None]
