"""Connected components of masks on the GPU (csrc/regions.hip, point_sam_amd/regions.py): every result is an integer or a bit, so every comparison is
equality -- against the plain numpy / scipy reference in tests/region_reference.py, the existing `decode` and the existing mask_* ops, never against
the new code's other path."""
import numpy as np
import pytest
import torch

import mask_reference as MR
import region_reference as R
import scene_reference as SR

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd import ops
    return ops


def _np_words(t):
    return t.cpu().numpy().view(np.uint64)


def _dev_words(masks):
    return torch.from_numpy(SR.words(masks).view(np.int64)).cuda()


class Cloud:
    """A cloud, its reference graph and the device graph built by the code under test from the same points and voxel size."""

    def __init__(self, ops, xyz, h):
        from point_sam_amd import regions
        self.xyz, self.h = np.ascontiguousarray(xyz, dtype=f32), h
        self.ref = R.Graph(self.xyz, h)
        self.dev = regions.build_graph(torch.from_numpy(self.xyz).cuda(), voxel_size=h)
        self.N, self.V = len(self.xyz), len(self.ref.keep_idx)


_CLOUDS = {}


def _cloud(ops, name):
    """Built once per session and never modified."""
    if name not in _CLOUDS:
        rng = np.random.default_rng(sum(map(ord, name)))
        if name.startswith("uniform"):
            N = int(name[7:])
            xyz, h = rng.uniform(-1, 1, (N, 3)), 0.2 if N <= 1000 else 0.09
        elif name == "sparse20000":                       # 50^3 cells, 15 % occupied: a half-density mask is below the percolation threshold
            xyz, h = rng.uniform(-1, 1, (20000, 3)), 0.04
        elif name == "duplicates":                        # every point three times, shuffled
            base = rng.uniform(-1, 1, (700, 3)).astype(f32)
            xyz, h = base[rng.permutation(np.repeat(np.arange(700), 3))], 0.17
        elif name == "edge":                              # points exactly at -1 on one, two or three axes: cell 0 has out-of-range neighbours
            xyz = rng.uniform(-1, 1, (1500, 3))
            for a in range(3):
                xyz[rng.choice(1500, 500, replace=False), a] = -1.0
            xyz[0] = -1.0
            h = 0.125
        elif name == "large":                             # 50^3 cells, ~62 % occupied: V > 70 000
            xyz, h = rng.uniform(-1, 1, (120000, 3)), 0.04
        else:
            raise KeyError(name)
        _CLOUDS[name] = Cloud(ops, xyz, h)
    return _CLOUDS[name]


def _cells_cloud(ops, cells, h, seed):
    """One point at the centre of every listed cell (a cell listed twice holds two points), in shuffled order: ranks are random along any path."""
    cells = np.asarray(cells, dtype=np.int64)
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(cells))
    xyz = (-1.0 + (cells[perm] + 0.5) * h).astype(f32)
    return Cloud(ops, xyz, h), perm


# ------------------------------------------------------------------------------------------------ 1. neighbours
@pytest.mark.parametrize("name", ["uniform1", "uniform64", "uniform1000", "uniform20000", "duplicates", "edge", "large"])
def test_neighbors_equal_reference(ops, name):
    c = _cloud(ops, name)
    assert np.array_equal(c.dev.keep_idx.cpu().numpy(), c.ref.keep_idx) and np.array_equal(c.dev.inv.cpu().numpy(), c.ref.inv)
    nbr = c.dev.nbr.cpu().numpy()
    assert nbr.dtype == np.int32 and nbr.shape == (c.V, 26)
    assert np.array_equal(nbr, c.ref.nbr)
    v, o = np.nonzero(nbr >= 0)
    assert np.array_equal(nbr[nbr[v, o], 25 - o], v), "offset 25 - o must lead back"
    if name == "large":
        assert c.V > 70000
    if name == "edge":
        low = (c.ref.cells == 0).any(1)
        assert low.sum() > 100 and (c.ref.cells[0] == 0).all()
        for axis, offs in enumerate(([o for o, d in enumerate(R.OFFSETS) if d[2 - a] == -1] for a in range(3))):
            assert (nbr[c.ref.cells[:, axis] == 0][:, offs] == -1).all()      # a step below cell 0 is out of range
    if name == "duplicates":
        assert c.V <= 700 < c.N
    if name == "uniform1":
        assert (nbr == -1).all()


# ------------------------------------------------------------------------------------------------ 2. labels
def _check_labels(ops, c, masks, tag=""):
    """Mask and complement of every row against the reference; returns the device labels (mask, complement)."""
    from point_sam_amd import regions
    bits = _dev_words(masks)
    out = []
    for comp in (False, True):
        got = regions.components(c.dev, bits, complement=comp).cpu().numpy()
        assert got.dtype == np.int32 and got.shape == masks.shape
        for k in range(len(masks)):
            want, _ = R.components(c.ref, ~masks[k] if comp else masks[k])
            assert np.array_equal(got[k], want), (tag, k, comp)
        out.append(got)
    return out


def _snake(ops):
    """A serpentine in the plane z = 3 of a 128^3 grid: rows y = 0, 2, ..., 126 joined by one cell at alternating ends: 8255 cells, every cell touching
    only its predecessor and successor (rows two apart do not touch)."""
    if "snake" not in _CLOUDS:
        cells = []
        for j in range(64):
            xs = range(128) if j % 2 == 0 else range(127, -1, -1)
            cells += [(x, 2 * j, 3) for x in xs]
            if j < 63:
                cells.append((127 if j % 2 == 0 else 0, 2 * j + 1, 3))
        _CLOUDS["snake"] = _cells_cloud(ops, cells, 2.0 / 128, 5) + (len(cells),)
    return _CLOUDS["snake"]


def _snake_masks(ops):
    c, perm, L = _snake(ops)
    assert L >= 4096 and c.V == L == c.N
    pos = np.empty(L, dtype=np.int64)
    pos[np.arange(L)] = perm                              # point i sits at path position perm[i]
    masks = np.ones((3, L), dtype=bool)
    masks[1, pos == 129 * 38 + 64] = False                # cut once in the middle of a row: two components
    masks[2, (pos % 129) == 64] = False                   # every row cut in its middle: 65 components
    return c, masks


def test_labels_single_snake(ops):
    """2(a): one component whose diameter is the whole path; ranks along the path are random.  A scheme with a fixed number of sweeps cannot pass."""
    c, masks = _snake_masks(ops)
    got, _ = _check_labels(ops, c, masks, "snake")
    assert (got[0] == 0).all(), "the whole snake is one component, id 0"
    assert len(np.unique(got[1][got[1] >= 0])) == 2 and len(np.unique(got[2][got[2] >= 0])) == 65


@pytest.mark.parametrize("N", [65, 64 * 5 + 37])
def test_labels_complement_ignores_tail_bits(ops, N):
    """2(b): the last word holds 1 / 37 points; the complement of a row is the points below N only."""
    rng = np.random.default_rng(N)
    c = Cloud(ops, rng.uniform(-1, 1, (N, 3)), 0.4)
    masks = rng.random((6, N)) < 0.5
    masks[0] = False; masks[1] = True; masks[2, -1] = False; masks[3, -1] = True
    _, comp = _check_labels(ops, c, masks, f"N={N}")
    assert (comp[1] == -1).all() and (comp[0] >= 0).all()


def _random_half_masks(c, K, seed):
    return np.random.default_rng(seed).random((K, c.N)) < 0.5


def test_labels_random_half_density(ops):
    """2(c): thousands of tiny components on a sparse cloud; on a dense one (several points per voxel) a giant component and a few small ones."""
    c = _cloud(ops, "sparse20000")
    got, _ = _check_labels(ops, c, _random_half_masks(c, 4, 1), "half, sparse")
    assert len(np.unique(got[0])) > 1000
    c = _cloud(ops, "uniform20000")
    _check_labels(ops, c, _random_half_masks(c, 2, 1), "half, dense")


def test_labels_empty_and_full_rows_among_ordinary_ones(ops):
    """2(d)."""
    c = _cloud(ops, "uniform1000")
    masks = _random_half_masks(c, 5, 2)
    masks[1] = False; masks[3] = True
    got, comp = _check_labels(ops, c, masks, "empty/full")
    assert (got[1] == -1).all() and (got[3] >= 0).all() and (comp[3] == -1).all()


def test_labels_plates(ops):
    """2(e): two 6 x 6 plates with one empty voxel layer between them are two components; two plates in adjacent layers that touch only at a corner
    (cells (5, 5, z) and (6, 6, z + 1)) are one."""
    plate = [(x, y) for x in range(6) for y in range(6)]
    apart = [(x, y, 10) for x, y in plate] + [(x, y, 12) for x, y in plate]
    corner = [(x, y, 20) for x, y in plate] + [(x + 6, y + 6, 21) for x, y in plate]
    c, _ = _cells_cloud(ops, apart + corner, 2.0 / 32, 9)
    got, _ = _check_labels(ops, c, np.ones((1, c.N), dtype=bool), "plates")
    z = c.ref.cells[c.ref.inv][:, 2]
    assert len(np.unique(got[0][z == 10])) == 1 and len(np.unique(got[0][z == 12])) == 1 and got[0][z == 10][0] != got[0][z == 12][0]
    assert len(np.unique(got[0][z >= 20])) == 1


def test_labels_large_cloud(ops):
    """2(f): V > 70 000, the voxel blocks of a row spread over the whole chip."""
    c = _cloud(ops, "large")
    masks = _random_half_masks(c, 2, 3)
    masks[1] = True
    _check_labels(ops, c, masks, "large")


# ------------------------------------------------------------------------------------------------ 3. clean
M = 5                                                     # the threshold of the clean tests


def _line(x0, y0, z, n):
    return [(x0 + i, y0, z) for i in range(n)]


def _rect(x0, y0, z, nx, ny):
    return [(x0 + i, y0 + j, z) for i in range(nx) for j in range(ny)]


def _clean_case(ops):
    """A cloud of separate patches on a 64^3 grid (patches are at least two cells apart, so they never touch) and mask rows on it.  Cells listed twice
    hold two points: sizes count points."""
    if "clean" in _CLOUDS:
        return _CLOUDS["clean"]
    patches = {
        "sheet": _rect(0, 0, 0, 24, 24),                                  # a 24 x 24 sheet: the playground of the island / seed rows
        "double": _line(30, 0, 0, 3) + _line(30, 0, 0, 3),                # three cells with two points each
        "strip": _rect(0, 0, 10, 7, 3),                                   # 7 x 3: two 3 x 3 blobs and the 3-point gap between them
        "holes": _rect(0, 0, 20, 12, 12),
    }
    names, cells = [], []
    for n, cs in patches.items():
        names += [n] * len(cs)
        cells += cs
    c, perm = _cells_cloud(ops, cells, 2.0 / 64, 11)
    names = np.array(names)[perm]
    cell = np.asarray(cells)[perm]

    def pick(name, pred):
        return (names == name) & np.array([bool(pred(*xyz)) for xyz in cell.tolist()])

    rows = {}
    # sizes exactly at the threshold: 36 stays, M stays, M - 1 goes (with min_island = M)
    rows["threshold"] = pick("sheet", lambda x, y, z: (x < 6 and y < 6) or (y == 10 and x < M) or (y == 14 and x < M - 1))
    # all small, a size tie between the two 3-point components: the one with the lower id stays, alone
    rows["all_small_tie"] = pick("sheet", lambda x, y, z: (y == 0 and x < 3) or (y == 4 and x < 3) or (y == 8 and x < 2))
    # two points per voxel: 6 points in 3 voxels stay at min_island = M (a count of voxels would remove them), next to a big blob
    rows["double"] = pick("double", lambda x, y, z: True) | pick("sheet", lambda x, y, z: x < 5 and y < 5)
    # holes: a 12 x 12 patch fully in the mask but for a hole of M points (stays open) and one of M - 1 (filled)
    rows["holes"] = pick("holes", lambda x, y, z: not ((y == 3 and 2 <= x < 2 + M) or (y == 7 and 2 <= x < 2 + M - 1)))
    # both: the strip's two 3 x 3 blobs (9 points each: below min_island = 10, a tie) and a gap of 3 points between them (below min_hole = 4)
    rows["join"] = pick("strip", lambda x, y, z: x != 3)
    rows["empty"] = np.zeros(c.N, dtype=bool)
    rows["full"] = np.ones(c.N, dtype=bool)
    # seeds: two big components, a small one
    rows["seeds"] = pick("sheet", lambda x, y, z: (x < 8 and y < 8) or (x >= 12 and y >= 12) or (x == 20 and y < 2))
    first = lambda m: int(np.flatnonzero(m)[0])
    pts = dict(a=first(pick("sheet", lambda x, y, z: x == 2 and y == 2)), b=first(pick("sheet", lambda x, y, z: x == 15 and y == 15)),
               out=first(pick("sheet", lambda x, y, z: x == 10 and y == 3)), small=first(pick("sheet", lambda x, y, z: x == 20 and y == 0)))
    _CLOUDS["clean"] = (c, rows, pts)
    return _CLOUDS["clean"]


def _run_clean(ops, c, masks, min_island, min_hole, select=None, seeds=None, chunk=None):
    from point_sam_amd import regions
    cfg = regions.RegionConfig(min_island=min_island, min_hole=min_hole)
    sel = None if select is None else torch.from_numpy(np.asarray(select, dtype=np.uint8)).cuda()
    sd = None if seeds is None else torch.from_numpy(np.asarray(seeds, dtype=np.int32)).cuda()
    bits_in = _dev_words(masks)
    bits, area, changed = regions.clean_bits(c.dev, bits_in, select=sel, seeds=sd, cfg=cfg, chunk=chunk)
    assert bits.data_ptr() != bits_in.data_ptr() and np.array_equal(_np_words(bits_in), SR.words(masks)), "the input rows must stay as they were"
    return _np_words(bits), area.cpu().numpy(), changed.cpu().numpy()


def _check_clean(ops, c, masks, min_island, min_hole, select=None, seeds=None, chunk=None, tag=""):
    want, area, changed, traces = R.clean(c.ref, masks, min_island, min_hole, select, seeds)
    bits, got_area, got_changed = _run_clean(ops, c, masks, min_island, min_hole, select, seeds, chunk)
    assert bits.shape == (len(masks), (c.N + 63) // 64)
    got = SR.unwords(bits, c.N)
    for k in range(len(masks)):
        assert np.array_equal(got[k], want[k]), (tag, k, int(got[k].sum()), int(want[k].sum()))
    assert np.array_equal(bits, SR.words(want)), "tail bits must be zero"
    assert got_area.dtype == np.int32 and np.array_equal(got_area, area) and np.array_equal(got_area, got.sum(1)), tag
    assert got_changed.dtype == np.uint8 and np.array_equal(got_changed, changed), tag
    return want, traces, (bits, got_area, got_changed)


def test_clean_islands_at_the_thresholds(ops):
    c, rows, _ = _clean_case(ops)
    names = ["threshold", "all_small_tie", "double", "empty", "full"]
    masks = np.stack([rows[n] for n in names])
    want, tr, _ = _check_clean(ops, c, masks, M, 0, tag="islands")
    # the reference itself took every branch
    assert tr[0]["removed"] == 1 and int(masks[0].sum()) - int(want[0].sum()) == M - 1 and not tr[0]["kept_small_largest"]
    assert tr[1]["tie"] and tr[1]["kept_small_largest"] and tr[1]["removed"] == 2 and int(want[1].sum()) == 3
    lab, sizes = R.components(c.ref, masks[1])
    tied = sorted(cid for cid, s in sizes.items() if s == 3)
    assert len(tied) == 2 and (lab[want[1]] == tied[0]).all(), "on a size tie the lowest id is the largest"
    assert tr[2]["removed"] == 0 and int(want[2].sum()) == 31
    assert not want[3].any() and want[4].all()


def test_clean_holes_at_the_thresholds(ops):
    c, rows, _ = _clean_case(ops)
    masks = np.stack([rows["holes"], rows["empty"], rows["full"], rows["threshold"]])
    want, tr, _ = _check_clean(ops, c, masks, 0, M, tag="holes")
    assert tr[0]["filled"] == 1 and int(want[0].sum()) - int(masks[0].sum()) == M - 1
    assert not want[1].any(), "an empty mask stays empty"
    # row 3: the six unmasked points of the `double` patch are a complement component of 6 points (3 voxels): not below M, so not filled
    assert tr[3]["filled"] == 0


def test_clean_holes_islands_and_both_where_a_filled_hole_joins_two_islands(ops):
    c, rows, _ = _clean_case(ops)
    masks = np.stack([rows["join"], rows["holes"], rows["threshold"]])
    only_islands, tr_i, _ = _check_clean(ops, c, masks, 10, 0, tag="islands only")
    only_holes, tr_h, _ = _check_clean(ops, c, masks, 0, 4, tag="holes only")
    both, tr_b, _ = _check_clean(ops, c, masks, 10, 4, tag="both")
    assert tr_i[0]["tie"] and tr_i[0]["removed"] == 1 and int(only_islands[0].sum()) == 9
    assert tr_h[0]["filled"] == 1 and int(only_holes[0].sum()) == 21
    assert tr_b[0]["filled"] == 1 and tr_b[0]["removed"] == 0 and int(both[0].sum()) == 21, "holes are filled before islands are judged"


def test_clean_select_copies_rows_bit_for_bit(ops):
    c, rows, _ = _clean_case(ops)
    names = ["threshold", "holes", "join", "all_small_tie", "threshold", "holes"]
    masks = np.stack([rows[n] for n in names])
    select = np.array([1, 0, 1, 0, 0, 1], dtype=np.uint8)
    want, tr, (bits, area, changed) = _check_clean(ops, c, masks, M, M, select=select, tag="select")
    for k in np.flatnonzero(select == 0):
        assert np.array_equal(bits[k], SR.words(masks[k:k + 1])[0]) and changed[k] == 0 and area[k] == masks[k].sum()
    assert changed[select == 1].all(), "every selected row of this case changes"
    # without select every row changes: the unselected ones were not left alone by accident
    assert R.clean(c.ref, masks, M, M)[2].all()


def test_clean_seeds(ops):
    c, rows, pts = _clean_case(ops)
    m = rows["seeds"]
    assert m[pts["a"]] and m[pts["b"]] and m[pts["small"]] and not m[pts["out"]]
    seeds = np.array([[pts["out"], -1, -1],               # none in the mask: the row is left as step 2 made it
                      [-1, pts["a"], -1],                 # one in the mask
                      [pts["a"], pts["out"], pts["b"]],   # two in different components
                      [pts["small"], -1, pts["a"]],       # a seed in a component that step 2 removes does not count
                      [-1, -1, -1]], dtype=np.int32)
    masks = np.stack([m] * 5)
    want, tr, _ = _check_clean(ops, c, masks, M, 0, seeds=seeds, tag="seeds")
    assert not tr[0]["seeded"] and tr[0]["removed"] == 1 and int(want[0].sum()) == 64 + 144
    assert tr[1]["seeded"] and tr[1]["seed_dropped"] == 1 and int(want[1].sum()) == 64
    assert tr[2]["seeded"] and tr[2]["seed_dropped"] == 0 and int(want[2].sum()) == 64 + 144
    assert tr[3]["seeded"] and int(want[3].sum()) == 64
    assert not tr[4]["seeded"]
    # seeds without an island threshold: the small component survives step 2 and can be the clicked one
    want, tr, _ = _check_clean(ops, c, masks, 0, 0, seeds=seeds, tag="seeds, no islands")
    assert int(want[3].sum()) == 64 + 2 and int(want[0].sum()) == int(m.sum())


def _all_clean_rows(ops):
    c, rows, pts = _clean_case(ops)
    names = ["threshold", "all_small_tie", "double", "holes", "join", "empty", "full", "seeds", "seeds"]
    masks = np.stack([rows[n] for n in names])
    seeds = np.full((len(names), 2), -1, dtype=np.int32)
    seeds[7] = [pts["a"], -1]; seeds[8] = [pts["out"], pts["b"]]; seeds[0] = [pts["out"], pts["out"]]
    select = np.ones(len(names), dtype=np.uint8); select[2] = 0
    return c, masks, seeds, select


def test_clean_chunked_over_rows_equals_the_whole_call(ops):
    c, masks, seeds, select = _all_clean_rows(ops)
    _, _, whole = _check_clean(ops, c, masks, M, M, select=select, seeds=seeds, tag="whole")
    for chunk in (1, 4):
        _, _, part = _check_clean(ops, c, masks, M, M, select=select, seeds=seeds, chunk=chunk, tag=f"chunk {chunk}")
        assert all(np.array_equal(a, b) for a, b in zip(whole, part))


def test_clean_random_masks_on_a_random_cloud(ops):
    """Random masks at densities 0.5, 0.9, 0.1 and 0.97 on a random cloud with several points per voxel: at 0.9 the complement falls apart into many
    small holes, at 0.1 the mask into many small islands; holes, islands and seeds at once."""
    c = _cloud(ops, "uniform20000")
    rng = np.random.default_rng(4)
    masks = rng.random((4, c.N)) < np.array([0.5, 0.9, 0.1, 0.97])[:, None]
    seeds = rng.integers(0, c.N, (4, 4)).astype(np.int32)
    want, tr, _ = _check_clean(ops, c, masks, 30, 30, seeds=seeds, tag="random")
    print([{k: int(v) for k, v in t.items()} for t in tr])
    assert tr[1]["filled"] > 20 and tr[3]["filled"] > 20 and tr[2]["removed"] > 20 and any(t["seeded"] for t in tr)


# ------------------------------------------------------------------------------------------------ 4. repeatability
def test_repeatability(ops):
    """2(a), 2(c) and 3 twice: bit-identical outputs, whatever order the waves arrived in."""
    from point_sam_amd import regions
    snake, snake_masks = _snake_masks(ops)
    rnd = _cloud(ops, "sparse20000")
    rnd_masks = _random_half_masks(rnd, 4, 1)
    c, masks, seeds, select = _all_clean_rows(ops)

    def once():
        out = [regions.components(snake.dev, _dev_words(snake_masks)), regions.components(rnd.dev, _dev_words(rnd_masks)),
               regions.components(rnd.dev, _dev_words(rnd_masks), complement=True)]
        out += list(regions.clean_bits(c.dev, _dev_words(masks), select=torch.from_numpy(select).cuda(), seeds=torch.from_numpy(seeds).cuda(),
                                       cfg=regions.RegionConfig(min_island=M, min_hole=M)))
        out += list(regions.clean_bits(rnd.dev, _dev_words(rnd_masks), cfg=regions.RegionConfig(min_island=30, min_hole=30)))
        return out

    first, second = once(), once()
    assert all(torch.equal(a, b) for a, b in zip(first, second))


# ------------------------------------------------------------------------------------------------ 5. proposals
def _decode_reference_run(model, ops, st, num_prompts, chunk):
    """The existing decode with the same chunking as generate_proposals (same Z per call: the same bits), logits to the host."""
    B, N, _ = st.coords.shape
    _, prompts = ops.fps(st.coords, num_prompts)
    logits, scores = [[] for _ in range(B)], [[] for _ in range(B)]
    for m0 in range(0, num_prompts, chunk):
        c = min(chunk, num_prompts - m0)
        pts = prompts[:, m0:m0 + c].reshape(B * c, 1, 3)
        masks, iou = model.decode(st, pts, torch.ones(B * c, 1, dtype=torch.int64, device="cuda"), None, True)
        for b in range(B):
            logits[b].append(masks[b * c:(b + 1) * c].reshape(-1, N).cpu().numpy())
            scores[b].append(iou[b * c:(b + 1) * c].reshape(-1).cpu().numpy())
    model.check_coordinate_range()
    return [np.concatenate(x) for x in logits], [np.concatenate(x) for x in scores]


def test_generate_proposals_with_region_cleanup_equals_decode_plus_reference(ops):
    """Tiny model, random weights (seed 3), 2048 points (seed 8), 32 prompts, threshold = the median logit, score and stability cuts at -inf,
    min_region_points = 10 on cells of 0.08.  On the oracle's logits of this setting (B = 1) 63 of the 96 candidates are selected, and the reference
    clean-up changes 53 of them and leaves 10 as they are; the test asserts at least 4 of each among the selected rows before anything is compared,
    so a cleaner that does nothing, or one that rewrites everything, fails."""
    from oracle import pointsam_oracle as O
    from point_sam_amd.config import get_config
    from point_sam_amd.model import PointCloudSAM
    from point_sam_amd.proposals import ProposalConfig, generate_proposals
    from point_sam_amd.weights import random_state_dict
    cfg = get_config("tiny")
    model = PointCloudSAM(cfg, random_state_dict(cfg, 3), "cuda", precision="f16x3")
    N, P, chunk, m, h = 2048, 32, 16, 10, 0.08
    ninf = float("-inf")
    for B in (1, 2):
        xyz, rgb, _, _ = O.synthetic_batch(B, N, seed=8)
        st = model.encode(xyz.cuda(), rgb.cuda())
        logits, scores = _decode_reference_run(model, ops, st, P, chunk)
        thr = float(f32(np.median(np.concatenate(logits))))
        pc = ProposalConfig(num_prompts=P, prompt_chunk=chunk, mask_threshold=thr, pred_iou_thresh=ninf, stability_thresh=ninf, stability_offset=1.0,
                            nms_thresh=0.7, min_points=1, max_area_frac=1.0001, min_region_points=m, region_voxel_size=h)
        got = generate_proposals(model, st, pc)
        assert len(got) == B
        for b in range(B):
            masks, area, hi, lo = MR.pack(logits[b], thr, 1.0)
            select = MR.validity(area, hi, lo, scores[b], N, 0, 2.0, ninf, ninf)
            g = R.Graph(st.coords[b].cpu().numpy(), h)
            cleaned, area2, changed, _ = R.clean(g, masks, m, m, select=select)
            n_changed, n_same = int(changed[select].sum()), int((changed[select] == 0).sum())
            print(f"B={B} cloud {b}: selected {int(select.sum())} of {len(select)}, reference changes {n_changed}, leaves {n_same}")
            assert n_changed >= 4 and n_same >= 4, (n_changed, n_same)
            assert (changed[~select] == 0).all()
            valid = MR.validity(area2, hi, lo, scores[b], N, 1, 1.0001, ninf, ninf)
            order = MR.order_of(scores[b])
            keep = MR.nms(order, valid, area2, MR.intersections(cleaned, cleaned), 0.7)
            cand = np.array([i for i in order if keep[i]], dtype=np.int64)
            p = got[b]
            assert len(cand) >= 1 and np.array_equal(p.candidate.cpu().numpy(), cand)
            assert np.array_equal(_np_words(p.bits), SR.words(cleaned[cand]))
            assert np.array_equal(p.area.cpu().numpy(), area2[cand])
            assert p.changed is not None and p.changed.dtype == torch.uint8 and np.array_equal(p.changed.cpu().numpy(), changed[cand])
            assert np.array_equal(p.labels.cpu().numpy(), MR.paint(cleaned, order, keep))
            assert np.array_equal(p.stability.cpu().numpy(), hi[cand].astype(f32) / lo[cand].astype(f32)), "area_hi / area_lo stay the logits' own"
        if B == 1:      # off: the composition of the existing mask_* ops, and no `changed`
            off = generate_proposals(model, st, ProposalConfig(**{**pc.__dict__, "min_region_points": 0}))[0]
            want = MR.proposals(logits[0], scores[0], N, thr, 1.0, 1, 1.0001, ninf, ninf, 0.7)
            assert off.changed is None and np.array_equal(off.candidate.cpu().numpy(), want["candidate"])
            assert np.array_equal(_np_words(off.bits), SR.words(want["masks"][want["candidate"]])) and np.array_equal(off.labels.cpu().numpy(), want["labels"])


# ------------------------------------------------------------------------------------------------ 6. predictor
def _nearest(points, cloud):
    """Index of the nearest cloud point per prompt: ((dx * dx) + dy * dy) + dz * dz in fp32, ties to the lowest index (ops.knn's order)."""
    d = (np.asarray(points, dtype=f32)[:, None, :] - np.asarray(cloud, dtype=f32)[None]).astype(f32)
    d2 = ((d[..., 0] * d[..., 0]).astype(f32) + (d[..., 1] * d[..., 1]).astype(f32)).astype(f32)
    d2 = (d2 + (d[..., 2] * d[..., 2]).astype(f32)).astype(f32)
    return d2.argmin(1)


def test_predictor_clean_masks_on_a_demo_ply(ops, golden_ply):
    """keep_clicked on a demo PLY: the result equals the reference given the nearest-point seeds; after set_scene the scan-width result equals the
    working cloud's reference result indexed by scene.inv."""
    from conftest import ply_cases
    from point_sam_amd.config import get_config
    from point_sam_amd.model import PointCloudSAM
    from point_sam_amd.predictor import PointSAMPredictor
    from point_sam_amd.regions import RegionConfig
    from point_sam_amd.weights import random_state_dict
    meta, _ = golden_ply
    cfg = get_config(meta["cfg"], meta["G"], meta["K"])
    pred = PointSAMPredictor(PointCloudSAM(cfg, random_state_dict(cfg, seed=meta["seed"]), "cuda", precision="f16x3"))
    _, xyz, rgb, _ = next(iter(ply_cases(golden_ply)))
    xyz, rgb = xyz.cuda().contiguous(), rgb.cuda().contiguous()
    N = xyz.shape[1]
    rng = np.random.default_rng(6)
    clicks = rng.choice(N, (2, 2), replace=False)
    pts = xyz[0][torch.from_numpy(clicks).cuda()]                      # [2 prompt sets, 2 prompts, 3]
    labels = torch.tensor([[1, 0], [1, 1]], device="cuda")
    m, h = 8, 0.1
    rc = RegionConfig(min_island=m, min_hole=m, voxel_size=h, keep_clicked=True)

    def reference(cloud, logits, thr, click_pts):
        """cloud [n, 3], logits [2, C, n] -> cleaned [2 * C, n] bool; the seeds are the nearest cloud points of the positive prompts."""
        C = logits.shape[1]
        near = _nearest(click_pts.reshape(-1, 3), cloud).reshape(2, 2)
        seeds = np.where(labels.cpu().numpy() == 1, near, -1).astype(np.int32).repeat(C, axis=0)
        masks = logits.reshape(2 * C, -1) > f32(thr)
        out, area, changed, tr = R.clean(R.Graph(cloud, h), masks, m, m, seeds=seeds)
        return out, area, changed, tr

    # ---- set_pointcloud
    pred.set_pointcloud(xyz, rgb)
    logits, _, _ = pred.predict_masks(pts, labels, None, True)
    L = logits.cpu().numpy()
    thr = float(f32(np.median(L)))
    # the seeds of the clean-up: per prompt set the point with the highest logit of its first candidate (inside that mask) and one more click
    seed_pts = pts.clone()
    seed_pts[0, 0] = xyz[0][int(L[0, 0].argmax())]; seed_pts[1, 0] = xyz[0][int(L[1, 0].argmax())]
    bits, area, changed = pred.clean_masks(logits, rc, seed_pts, labels, threshold=thr)
    want, want_area, want_changed, tr = reference(xyz[0].cpu().numpy(), L, thr, seed_pts.cpu().numpy())
    print("ply", N, "points:", [{k: int(v) for k, v in t.items()} for t in tr])
    assert tr[0]["seeded"] and tr[3]["seeded"], "a click at the mask's highest logit is a member of it"
    assert tuple(bits.shape) == (6, (N + 63) // 64) and np.array_equal(_np_words(bits), SR.words(want))
    assert np.array_equal(area.cpu().numpy(), want_area) and np.array_equal(changed.cpu().numpy(), want_changed)
    graphs = pred._graphs
    pred.clean_masks(logits, rc, seed_pts, labels, threshold=thr)
    assert pred._graphs is graphs, "the graph is cached with the cloud"
    pred.clean_masks(logits, RegionConfig(min_island=m, voxel_size=0.2), threshold=thr)
    assert pred._graphs is not graphs, "other voxel settings: rebuilt"

    # ---- set_scene: the scan is the same PLY, the working cloud one point per voxel of 0.05
    pred.set_scene(xyz[0], rgb[0], voxel_size=0.05)
    sc = pred.scene
    assert not sc.identity and sc.num_working < N
    full, _, _ = pred.predict_masks(pts, labels, None, True)
    assert full.shape[-1] == N
    Lw = full.cpu().numpy()[..., sc.keep_idx.cpu().numpy()]
    thr = float(f32(np.median(Lw)))
    work = xyz[0][sc.keep_idx]
    seed_pts[0, 0] = work[int(Lw[0, 0].argmax())]; seed_pts[1, 0] = work[int(Lw[1, 0].argmax())]
    want_w, _, want_changed, tr = reference(work.cpu().numpy(), Lw, thr, seed_pts.cpu().numpy())
    assert tr[0]["seeded"] and tr[3]["seeded"]
    want_full = want_w[:, sc.inv.cpu().numpy()]
    bits, area, changed = pred.clean_masks(full, rc, seed_pts, labels, threshold=thr)
    assert tuple(bits.shape) == (6, (N + 63) // 64) and np.array_equal(_np_words(bits), SR.words(want_full))
    assert np.array_equal(area.cpu().numpy(), want_full.sum(1)) and np.array_equal(changed.cpu().numpy(), want_changed)
    # logits of the working cloud's width are cleaned and returned at that width
    bits_w, area_w, _ = pred.clean_masks(torch.from_numpy(Lw).cuda(), rc, seed_pts, labels, threshold=thr)
    assert np.array_equal(_np_words(bits_w), SR.words(want_w)) and np.array_equal(area_w.cpu().numpy(), want_w.sum(1))
