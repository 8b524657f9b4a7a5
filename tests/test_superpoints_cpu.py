"""Normals and superpoints, host side (no GPU needed): the numpy reference on hand-built cases, the configuration's validation, the chunking of
snap_bits, and the C entry points -- declared, bound, exported, built with the flags the contract needs, and refusing bad arguments before a launch."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import normal_cases as NC
import region_reference as R
import superpoint_reference as SP
from point_sam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("psam_normals_voxel_workspace_bytes", "psam_normals_voxel", "psam_superpoints_workspace_bytes", "psam_superpoints",
                "psam_superpoint_snap_workspace_bytes", "psam_superpoint_snap")
f32 = np.float32


# ------------------------------------------------------------------------------------------------ the reference on hand-built cases
def _lattice_plane():
    """65 x 65 points on z = 0.25, spacing 1 / 64: every coordinate is a multiple of 2^-6, so q is exact and every q_z is the same integer."""
    g = np.arange(-32, 33) / 64.0
    x, y = np.meshgrid(g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.full(x.size, 0.25)], 1).astype(f32)


def _two_planes():
    """A floor z = -0.5 and a wall x = -0.5, 33 x 33 lattice points each (spacing 1 / 32), meeting at a right angle along the line x = z = -0.5."""
    g = np.arange(-16, 17) / 32.0
    a, b = np.meshgrid(g, g, indexing="ij")
    floor = np.stack([a.ravel(), b.ravel(), np.full(a.size, -0.5)], 1)
    wall = np.stack([np.full(a.size, -0.5), b.ravel(), a.ravel()], 1)
    return np.concatenate([floor, wall]).astype(f32)


def test_fixed_point_is_exact_and_drops_points_outside_the_cube():
    q, ok = SP.fixed(np.array([[-1, 0, 1], [0.5, -0.25, 2.0 ** -20], [-(2.0 ** -21), 0, 0], [1.5, 0, 0], [np.nan, 0, 0], [0, -np.inf, 0]], dtype=f32))
    assert ok.tolist() == [True, True, True, False, False, False]
    assert q[:3].tolist() == [[0, 1 << 20, 1 << 21], [(1 << 20) + (1 << 19), (1 << 20) - (1 << 18), (1 << 20) + 1], [(1 << 20) - 1, 1 << 20, 1 << 20]]


def test_scatter_is_exact_invariant_under_translation_and_order():
    rng = np.random.default_rng(5)
    xyz = (np.round(rng.uniform(-0.4, 0.4, (300, 3)) * 2.0 ** 20) / 2.0 ** 20).astype(f32)      # 20 fractional bits: sums with 1 and 1 / 4 are exact in fp32
    g = R.Graph(xyz, 0.25)
    count, s, S = SP.scatter(xyz, g.inv, g.nbr)
    # a brute-force neighbourhood by cells, in Python integers
    q, _ = SP.fixed(xyz)
    for v in (0, len(S) // 2, len(S) - 1):
        near = np.flatnonzero((np.abs(g.cells[g.inv] - g.cells[v]) <= 1).all(1))
        pts = [tuple(int(c) for c in q[i]) for i in near]
        n = len(pts)
        assert count[v] == n
        want = [n * sum(p[a] * p[b] for p in pts) - sum(p[a] for p in pts) * sum(p[b] for p in pts) for a, b in SP.PAIRS]
        assert S[v] == want
    # a shift by one whole cell (2^18 fixed-point steps) moves every point to the next cell and leaves S as it is; so does another order of the points
    shifted = (xyz.astype(np.float64) + 0.25).astype(f32)
    assert np.array_equal(shifted.astype(np.float64), xyz.astype(np.float64) + 0.25), "the shift is exact in fp32 here"
    q2, _ = SP.fixed(shifted)
    assert np.array_equal(q2 - q, np.full_like(q, 1 << 18))
    g1 = R.Graph(shifted, 0.25)
    assert np.array_equal(g1.inv, g.inv) and np.array_equal(g1.cells, g.cells + 1)
    assert SP.scatter(shifted, g1.inv, g1.nbr)[2] == S
    perm = rng.permutation(len(xyz))
    g2 = R.Graph(xyz[perm], 0.25)
    _, _, S2 = SP.scatter(xyz[perm], g2.inv, g2.nbr)
    assert [S2[g2.inv[np.flatnonzero(perm == g.keep_idx[v])[0]]] for v in range(len(S))] == S


def test_a_lattice_plane_has_normal_z_and_curvature_exactly_zero():
    xyz = _lattice_plane()
    g = R.Graph(xyz, 0.125)
    count, s, S = SP.scatter(xyz, g.inv, g.nbr)
    assert all(row[2] == 0 and row[4] == 0 and row[5] == 0 for row in S), "no spread along z: the xz, yz and zz entries are exact zeros"
    normal, curv, lam, _ = SP.normals(count, s, S)
    assert count.min() >= 5
    assert np.array_equal(normal, np.tile(np.array([0, 0, 1], dtype=f32), (len(S), 1)))
    assert np.array_equal(curv, np.zeros(len(S), dtype=f32))
    # below min_points: no normal
    normal, curv, _, _ = SP.normals(count, s, S, min_points=int(count.max()) + 1)
    assert not normal.any() and not curv.any()
    # a viewpoint below the plane turns every normal towards it
    normal, _, _, facing = SP.normals(count, s, S, viewpoint=(0.0, 0.0, -1.0))
    assert np.array_equal(normal, np.tile(np.array([0, 0, -1], dtype=f32), (len(S), 1))) and (facing > 0.5).all()


def test_two_planes_at_a_right_angle_give_two_superpoints_and_one_at_91_degrees():
    xyz = _two_planes()
    g = R.Graph(xyz, 0.125)
    count, s, S = SP.scatter(xyz, g.inv, g.nbr)
    normal, curv, _, _ = SP.normals(count, s, S)
    vl, pl, size, num = SP.superpoints(g.inv, g.nbr, count, normal, curv, SP.cos_of(15.0), 0.08, 5, 50, 2)
    assert num == 2 and int(size.sum()) == len(xyz) and (pl >= 0).all()
    assert np.array_equal(pl, vl[g.inv]) and np.array_equal(np.bincount(pl), size)
    # away from the shared edge the floor is one superpoint and the wall the other
    floor, wall = np.arange(len(xyz)) < len(xyz) // 2, np.arange(len(xyz)) >= len(xyz) // 2
    far = (xyz[:, 0] > -0.2) | (xyz[:, 2] > -0.2)
    assert len(set(pl[floor & far])) == 1 and len(set(pl[wall & far])) == 1 and pl[floor & far][0] != pl[wall & far][0]
    # before the absorb rounds the voxels along the edge (mixed neighbourhoods: high curvature) stand alone
    _, _, size0, num0 = SP.superpoints(g.inv, g.nbr, count, normal, curv, SP.cos_of(15.0), 0.08, 5, 0, 0)
    assert num0 > 2 and sorted(size0.tolist())[-2:] == [825, 825]
    # 91 degrees: cos < 0, every pair of normals passes; with the curvature test open too (the edge voxels lie between the planes) all is one
    _, pl1, size1, num1 = SP.superpoints(g.inv, g.nbr, count, normal, curv, SP.cos_of(91.0), 1.0, 5, 50, 2)
    assert num1 == 1 and size1.tolist() == [len(xyz)] and not pl1.any()


def test_absorb_ties_go_to_the_lower_label_and_labels_are_compacted_in_order():
    """Five voxels in a row along x (cells 0 .. 4), ranks in point order 3 1 4 0 2 for the cells 0 .. 4 -- hand-made normals: cells 0, 1 join, cells
    3, 4 join, cell 2 (rank 4) stands alone between them with a normal equally far from both."""
    cell_of_rank = [3, 1, 4, 0, 2]
    xyz = np.array([[-1 + (c + 0.5) * 0.25, -0.9, -0.9] for c in cell_of_rank for _ in range(3)], dtype=f32)
    g = R.Graph(xyz, 0.25)
    assert g.inv.tolist() == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3 + [4] * 3
    count = np.full(5, 9)
    z, xdir, diag = [0, 0, 1], [1, 0, 0], [np.sqrt(0.5), 0, np.sqrt(0.5)]
    normal = np.array([xdir, z, xdir, z, diag], dtype=f32)       # ranks 3, 1 (cells 0, 1): z; ranks 0, 2 (cells 3, 4): x; rank 4 (cell 2): between
    curv = np.zeros(5, dtype=f32)
    vl, pl, size, num = SP.superpoints(g.inv, g.nbr, count, normal, curv, SP.cos_of(15.0), 0.08, 5, 0, 0)
    # union only: components {1, 3} (label 1), {0, 2} (label 0), {4}; compacted in increasing order of the label: 0 -> 0, 1 -> 1, 4 -> 2
    assert num == 3 and vl.tolist() == [0, 1, 0, 1, 2] and size.tolist() == [6, 6, 3]
    # one round, min_size 4: rank 4 is small, both neighbours score |cos 45| -- bit for bit the same product -- and the lower label (0) wins
    assert float(SP.dots(normal, 4, 0)) == float(SP.dots(normal, 4, 1))
    vl, pl, size, num = SP.superpoints(g.inv, g.nbr, count, normal, curv, SP.cos_of(15.0), 0.08, 5, 4, 1)
    assert num == 2 and vl.tolist() == [0, 1, 0, 1, 0] and size.tolist() == [9, 6]
    # min_size above every size: nobody is large enough to absorb anybody
    vl, _, size, num = SP.superpoints(g.inv, g.nbr, count, normal, curv, SP.cos_of(15.0), 0.08, 5, 100, 2)
    assert num == 3 and size.tolist() == [6, 6, 3]


def test_snap_reference_thresholds():
    label = np.array([0, 0, 0, 0, 1, 1, 1, -1, 2, 2], dtype=np.int32)
    size = np.array([4, 3, 2], dtype=np.int32)
    m = np.zeros((3, 10), dtype=bool)
    m[0, [0, 1, 4, 7]] = True        # half of superpoint 0, a third of 1, the unlabelled point
    m[1, [2, 3, 5, 6, 8]] = True     # the other half of 0, two thirds of 1, half of 2: disjoint from row 0
    out, area, changed = SP.snap(m, label, size, 0)
    assert out[0].tolist() == [1, 1, 1, 1, 1, 1, 1, 0, 0, 0] and out[1].tolist() == [1, 1, 1, 1, 1, 1, 1, 0, 1, 1] and not out[2].any()
    out, area, changed = SP.snap(m, label, size, 32768)                # a strict majority: exactly half is not enough
    assert out[0].sum() == 0 and out[1].tolist() == [0, 0, 0, 0, 1, 1, 1, 0, 0, 0] and not (out[0] & out[1]).any()
    assert area.tolist() == [0, 3, 0] and changed.tolist() == [1, 1, 0]
    out, _, _ = SP.snap(np.ones((1, 10), dtype=bool), label, size, 65535)      # a full row keeps every labelled point even at the highest threshold
    assert out[0].tolist() == [1, 1, 1, 1, 1, 1, 1, 0, 1, 1]


# ------------------------------------------------------------------------------------------------ the cases of tests/normal_cases.py
def test_committed_triples_have_their_pattern_and_the_search_finds_them():
    for table, m_bits in ((NC.HIGH, (12, 14)), (NC.LOW, (7, 10))):
        assert NC.search(m_bits) == {name: triple for name, triple, _ in table}
        for name, (m, dx, dy), bits in table:
            x = m * m * dx * dy
            assert x.bit_length() == bits and (bits > 64) == (table is NC.HIGH) and 2 * m <= 1 << 15
            assert NC.pattern(x) == NC.pattern(-x) == name
            # the pattern, spelled out once more on the binary digits: 53 kept, then the half bit, ten more to the end of the top 64, the rest
            digits = bin(x)[2:]
            kept, half, mid, rest = digits[:53], digits[53], digits[54:64], digits[64:]
            if name.startswith("tie"):
                assert half == "1" and "1" not in mid + rest and kept[-1] == ("1" if name == "tie_odd" else "0")
                assert float(x) == float((int(kept, 2) + (name == "tie_odd")) << (bits - 53))
            elif name == "half_sticky":
                assert half == "1" and "1" not in mid and "1" in rest and float(x) == float((int(kept, 2) + 1) << (bits - 53)), "up"
            else:
                assert half == "0" and "0" not in mid and "1" in rest and float(x) == float(int(kept, 2) << (bits - 53)), "down"
                if name == "below_half_odd":
                    assert kept[-1] == "1" and rest[0] == "1"
    assert [n for n, _, _ in NC.HIGH] == ["tie_even", "tie_odd", "below_half", "below_half_odd", "half_sticky"]
    assert [n for n, _, _ in NC.LOW] == ["tie_even", "tie_odd"]


def test_two_cluster_puts_the_product_into_the_scatter_matrix():
    cases = NC.rounding_cases()
    assert len(cases) == 2 * (len(NC.HIGH) + len(NC.LOW))
    for name, (m, d) in cases.items():
        xyz, inv, nbr = NC.two_cluster(m, d)
        assert xyz.shape == (2 * m, 3) and xyz.dtype == f32 and len(np.unique(xyz, axis=0)) == 2
        assert not np.array_equal(xyz[:m], np.tile(xyz[0], (m, 1))), "shuffled"
        count, s, S = SP.scatter(xyz, inv, nbr)
        assert count.tolist() == [2 * m] and S == [NC.two_cluster_scatter(m, d)] == [[m * m * d[a] * d[b] for a, b in SP.PAIRS]]
        assert (S[0][1] < 0) == name.endswith("_neg") and NC.pattern(S[0][1]) == name.split("_", 1)[1].replace("_neg", "")


def test_wrong_conversions_are_told_apart_by_the_committed_cases():
    """Stands in for running a mutated kernel: each wrong int -> fp64 conversion differs from float(exact) on the xy entry of a committed case, for
    both signs, and in both branches of the conversion where its mistake can show (up to 64 bits only the ties exist, and the two conversions that
    go through 64 bits are exact there)."""
    xy = {name: NC.two_cluster_scatter(m, d)[1] for name, (m, d) in NC.rounding_cases().items()}
    for x in xy.values():                                  # none of them is wrong about a value fp64 holds
        r = abs(x).bit_length() - 53
        assert all(f(x >> r << r) == float(x >> r << r) == (x >> r << r) for f in NC.WRONG.values())
    caught = {n: {name for name, x in xy.items() if f(x) != float(x)} for n, f in NC.WRONG.items()}
    assert caught["truncating"] >= {"high_tie_odd", "high_tie_odd_neg", "high_half_sticky", "low_tie_odd", "low_tie_odd_neg"}
    assert caught["half_up"] == {"high_tie_even", "high_tie_even_neg", "low_tie_even", "low_tie_even_neg"}
    assert caught["twice"] >= {"high_below_half_odd", "high_below_half_odd_neg"} and not any(n.startswith("low") for n in caught["twice"])
    assert caught["without_sticky"] == {"high_half_sticky", "high_half_sticky_neg"}
    for x in xy.values():                                  # and a conversion of the magnitude is what the reference does to a negative value
        assert float(-x) == -float(x)


def _exact_scatter(name):
    xyz, h = NC.cloud_points(name)
    xyz = np.ascontiguousarray(xyz, dtype=f32)
    g = R.Graph(xyz, h)
    return g, SP.scatter(xyz, g.inv, g.nbr)


@pytest.mark.parametrize("name", ["wide", "wide18"])
def test_wide_clouds_need_more_than_64_bits_and_round(name):
    g, (count, s, S) = _exact_scatter(name)
    assert len(S) == 8 and count.tolist() == [NC.WIDE[name]] * 8, "every neighbourhood is the whole cloud"
    largest, above, rounded = NC.scatter_stats(S)
    assert above > 0 and rounded > 0
    assert (largest, above, rounded) == NC.WIDE_COUNTS[name]
    if name == "wide18":
        assert sorted(abs(x).bit_length() for x in S[0])[0] == 64, "one entry fills the low word exactly: the last value of the branch without a shift"


def test_the_older_clouds_never_round():
    """Every scatter entry of the clouds test_count_and_scatter_equal_the_exact_integers runs is an integer fp64 holds: that test sees no rounding
    at all, which is why the rounding cases above exist.  Should this change, that test's equality still holds -- this only keeps the record."""
    for name in ("box", "sphere", "uniform6000", "grid", "edge", "duplicates", "heavy", "small63", "small65", "small4"):
        _, (count, s, S) = _exact_scatter(name)
        largest, above, rounded = NC.scatter_stats(S)
        assert largest <= 53 and above == 0 and rounded == 0, name


@pytest.mark.parametrize("name", sorted(NC.degenerate_fixed()))
def test_degenerate_neighbourhoods_have_the_stated_spectrum(name):
    """eigvalsh of float(S).  "Zero" and "equal" mean to 1e-14 l2: LAPACK's eigenvalues carry an error of a small multiple of 2^-53 |M|."""
    q, spectrum = NC.degenerate_fixed()[name]
    xyz, inv, nbr = NC.degenerate(name)
    count, s, S = SP.scatter(xyz, inv, nbr)
    assert count.tolist() == [len(q)] and len(q) >= 5
    pts = [tuple(int(c) for c in p) for p in q]            # S once more, from the integers the case was built of
    assert S[0] == [len(pts) * sum(p[a] * p[b] for p in pts) - sum(p[a] for p in pts) * sum(p[b] for p in pts) for a, b in SP.PAIRS]
    assert all(float(x) == x for x in S[0]), "small cases: the eigen solve's input is exact"
    lam = SP.eigen(count, S)[2][0]
    top, tol = lam[2], 1e-14 * lam[2]
    for i, tok in enumerate(spectrum):
        if tok == "0":
            assert abs(lam[i]) <= tol
        elif tok == "e":
            assert tol < lam[i] <= 1e-9 * top
        else:
            assert lam[i] > 0.1 * top
        for j in range(i):
            if spectrum[j][0] != tok[0]:
                assert lam[i] - lam[j] > 0.1 * top
            elif tok[0] not in "0e":
                assert tol < lam[i] - lam[j] <= 0.01 * lam[i] if "~" in tok + spectrum[j] else abs(lam[i] - lam[j]) <= tol
    if name == "coincident":
        assert S[0] == [0] * 6
    if name == "cubic":
        assert S[0][1] == S[0][2] == S[0][4] == 0 and S[0][0] == S[0][3] == S[0][5] > 0


# ------------------------------------------------------------------------------------------------ configuration and chunking
def test_superpoint_config_validation_and_defaults():
    from point_sam_amd.superpoints import SuperpointConfig
    d = SuperpointConfig().validate()
    assert (d.angle_deg, d.max_curvature, d.min_points, d.min_size, d.absorb_rounds, d.voxel_size, d.points_per_voxel) == (15.0, 0.08, 5, 50, 2, None, 4)
    assert d.cos_angle == SP.cos_of(15.0)
    assert "NOT been tuned" in SuperpointConfig.__doc__
    SuperpointConfig(angle_deg=91, max_curvature=1.0, min_points=1, min_size=0, absorb_rounds=0, voxel_size=0.05, points_per_voxel=1).validate()
    for bad in (dict(angle_deg=-1.0), dict(angle_deg=181.0), dict(angle_deg=float("nan")), dict(angle_deg="15"), dict(angle_deg=True),
                dict(max_curvature=-0.1), dict(max_curvature=1.5), dict(max_curvature=float("nan")), dict(min_points=0), dict(min_points=2.5),
                dict(min_points=True), dict(min_size=-1), dict(min_size=1.5), dict(absorb_rounds=-1), dict(absorb_rounds=65), dict(absorb_rounds=1.0),
                dict(voxel_size=0.0), dict(voxel_size=-0.1), dict(voxel_size=float("inf")), dict(voxel_size="0.1"), dict(points_per_voxel=0)):
        with pytest.raises(ValueError):
            SuperpointConfig(**bad).validate()
    assert SuperpointConfig().key() != SuperpointConfig(min_size=51).key()


def test_proposal_config_snap_field():
    from point_sam_amd.proposals import ProposalConfig
    from point_sam_amd.superpoints import SuperpointConfig
    assert ProposalConfig().validate().snap is None, "off by default"
    assert ProposalConfig.from_overrides({"snap": {"min_size": 20}}).snap == SuperpointConfig(min_size=20)
    assert ProposalConfig(snap=SuperpointConfig()).validate().snap == SuperpointConfig()
    for bad in ({"snap": 1}, {"snap": {"min_size": -1}}, {"snap": {"nonsense": 1}}, {"snap": "on"}):
        with pytest.raises(ValueError):
            ProposalConfig.from_overrides(bad)


def test_snap_bits_chunks_rows_so_that_the_count_table_stays_under_the_limit():
    from point_sam_amd import regions, superpoints as M
    assert M.q16_of(0.0) == 0 and M.q16_of(0.5) == 32768 and M.q16_of(1.0) == 65535 and M.q16_of(0.25) == 16384
    for bad in (-0.1, 1.1, float("nan"), "0.5", True):
        with pytest.raises(ValueError):
            M.q16_of(bad)
    for num in (1, 7, 1000, 1 << 20, 1 << 27):
        rows = M.rows_per_call(num)
        assert 1 <= rows <= regions.MAX_ROWS
        assert rows == 1 or rows * (4 * num + 16) <= regions.WORKSPACE_LIMIT      # the table [rows, num] int32, rounded up to 16 bytes
        assert rows == regions.MAX_ROWS or (rows + 1) * (4 * num + 16) > regions.WORKSPACE_LIMIT, "and no fewer rows than fit"
    assert M.rows_per_call(1000) == regions.MAX_ROWS and M.rows_per_call(1 << 20) == 63 and M.rows_per_call(1 << 27) == 1

    # the calls snap_bits makes, against a stand-in for the op: K = 7 rows in chunks of 3 -> 3 + 3 + 1, results in row order
    calls = []

    def fake(bits, labels, size, q16):
        calls.append((bits.shape[0], q16))
        return bits + 1, torch.full((bits.shape[0],), len(calls), dtype=torch.int32), torch.ones(bits.shape[0], dtype=torch.uint8)

    sp = M.Superpoints(torch.zeros(130, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), torch.tensor([130], dtype=torch.int32), 1, None)
    bits = torch.arange(7 * 3, dtype=torch.int64).reshape(7, 3)
    real, M.ops.superpoint_snap = M.ops.superpoint_snap, fake
    try:
        out, area, changed = M.snap_bits(sp, bits, 0.25, chunk=3)
        assert calls == [(3, 16384), (3, 16384), (1, 16384)] and torch.equal(out, bits + 1) and area.tolist() == [1, 1, 1, 2, 2, 2, 3]
        calls.clear()
        M.snap_bits(sp, bits)
        assert calls == [(7, 32768)]
        with pytest.raises(ValueError):
            M.snap_bits(sp, bits[:, :2])
        with pytest.raises(ValueError):
            M.snap_bits(sp, bits, chunk=0)
    finally:
        M.ops.superpoint_snap = real


def test_superpoint_bindings_refuse_cpu_tensors():
    from point_sam_amd import ops
    inv, nbr = torch.zeros(64, dtype=torch.int64), torch.full((4, 26), -1, dtype=torch.int32)
    with pytest.raises(_lib.PointSamHipError):
        ops.voxel_normals(torch.zeros(64, 3), inv, nbr)
    with pytest.raises(_lib.PointSamHipError):
        ops.superpoint_labels(inv, nbr, torch.zeros(4, dtype=torch.int32), torch.zeros(4, 3), torch.zeros(4), 0.9, 0.08)
    with pytest.raises(_lib.PointSamHipError):
        ops.superpoint_snap(torch.zeros(2, 1, dtype=torch.int64), torch.zeros(64, dtype=torch.int32), torch.ones(3, dtype=torch.int32), 0)


class _NoModel:
    def __getattr__(self, name):
        raise AssertionError("the model must not be reached")


def test_predictor_methods_need_a_cloud():
    from point_sam_amd.predictor import PointSAMPredictor
    pred = PointSAMPredictor(_NoModel())
    for call in (lambda: pred.point_normals(), lambda: pred.superpoints(), lambda: pred.snap_masks(torch.zeros(1, 1, dtype=torch.int64))):
        with pytest.raises(RuntimeError, match="set_pointcloud"):
            call()
    pred._state = object()
    with pytest.raises(TypeError, match="SuperpointConfig"):
        pred.superpoints(cfg={"min_size": 3})


# ------------------------------------------------------------------------------------------------ the C entry points
def test_entry_points_are_declared_bound_and_exported(tmp_path):
    from point_sam_amd.build import SOURCES, build_library
    build_library()                                        # the library cross-builds with the two new translation units
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pointsam_hip.h")).read()
    assert "normals and superpoints */" in hdr
    declared = set(re.findall(r"\b(psam_normals_[a-z0-9_]+|psam_superpoints?_[a-z0-9_]+|psam_superpoints)\s*\(", hdr))
    assert declared == set(ENTRY_POINTS) == {n for n in _lib.SIGNATURES if n.startswith(("psam_normals_", "psam_superpoint"))}
    kinds = {"int32_t": _lib.i32, "float": _lib.f32, "double": _lib.f64, "size_t": _lib.size_t}
    for n in ENTRY_POINTS:
        assert hasattr(lib, n), n
        ret, args = re.search(r"(\w+) %s\(([^)]*)\)" % n, hdr).groups()
        want = [_lib.ptr if "*" in a or "psam_stream_t" in a else kinds[a.split()[0]] for a in args.split(",")]
        assert _lib.SIGNATURES[n] == (kinds[ret], want) and ret == ("size_t" if n.endswith("_bytes") else "int32_t"), n
    flags = dict(SOURCES)
    for f in ("normals.hip", "superpoints.hip"):
        assert "-ffp-contract=off" in flags[f] and "-fno-slp-vectorize" in flags[f] and flags[f] == flags["geometry.hip"], f
    csrc = os.path.join(ROOT, "point_sam_amd", "csrc")
    # one union-find: regions.hip and superpoints.hip share region_union.h and keep no copy of the hook
    for f in ("regions.hip", "superpoints.hip"):
        src = open(os.path.join(csrc, f)).read()
        assert '#include "region_union.h"' in src and "atomicCAS" not in src, f
    assert open(os.path.join(csrc, "region_union.h")).read().count("atomicCAS(&par[a], a, b)") == 1
    # the scatter matrix is integer: no floating-point atomic, no fp accumulation before the one conversion
    normals_src = open(os.path.join(csrc, "normals.hip")).read()
    assert "__int128" in normals_src and "atomicAdd(&row[" in normals_src and "atomicAdd(float" not in normals_src and "atomicAdd(double" not in normals_src
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("needs a C compiler")
    prog = ['#include "pointsam_hip.h"', "#include <stdio.h>", "int main(void) {",
            "    size_t a = psam_normals_voxel_workspace_bytes(5000, 1000), b = psam_superpoints_workspace_bytes(5000, 1000),",
            "           c = psam_superpoint_snap_workspace_bytes(7, 5000, 33);",
            '    printf("%lu %lu %lu\\n", (unsigned long)a, (unsigned long)b, (unsigned long)c);']
    prog += [f"    void* p{i} = (void*){n};" for i, n in enumerate(ENTRY_POINTS)]
    prog += ["    return " + " && ".join(f"p{i} != 0" for i in range(len(ENTRY_POINTS))) + " ? 0 : 1;", "}"]
    c = tmp_path / "superpoint_symbols.c"
    c.write_text("\n".join(prog))
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-Wno-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", str(c), "-o",
                    str(tmp_path / "superpoint_symbols.o")], check=True)


def test_entry_points_reject_bad_arguments_on_the_host():
    """Null pointers, bad shapes and parameters return -1 with a message, a short workspace -3, a misaligned one -2, all before any launch."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15               # a non-null, aligned pointer; never dereferenced by the device: every call below is refused
    q = p + 256
    big = 1 << 40

    def rejected(status, word, code=-1):
        assert status == code, status
        msg = lib.psam_last_error_string()
        assert word in msg, msg

    N, V, K, S = 5000, 1000, 7, 33
    # ---- workspace sizes for one stated shape
    assert lib.psam_normals_voxel_workspace_bytes(N, V) == V * 16 * 8        # sixteen 64-bit sums per voxel
    # six [V] int32 arrays; the scan's ballots (one 64-bit word per wave of the one block of 1024 ranks: 16) and its block counts (1 + 1, padded to 16)
    assert lib.psam_superpoints_workspace_bytes(N, V) == 6 * V * 4 + 16 * 8 + 16
    assert lib.psam_superpoint_snap_workspace_bytes(K, N, S) == (K * S * 4 + 15) // 16 * 16
    for bad in (0, -3):
        assert lib.psam_normals_voxel_workspace_bytes(bad, V) == 0 and lib.psam_normals_voxel_workspace_bytes(N, bad) == 0
        assert lib.psam_superpoints_workspace_bytes(bad, V) == 0 and lib.psam_superpoints_workspace_bytes(N, bad) == 0
        assert lib.psam_superpoint_snap_workspace_bytes(bad, N, S) == 0 and lib.psam_superpoint_snap_workspace_bytes(K, bad, S) == 0
        assert lib.psam_superpoint_snap_workspace_bytes(K, N, bad) == 0
    assert lib.psam_normals_voxel_workspace_bytes(V, V + 1) == 0 and lib.psam_normals_voxel_workspace_bytes((1 << 28) + 1, V) == 0      # V <= N <= 2^28
    assert lib.psam_superpoint_snap_workspace_bytes(65536, N, S) == 0 and lib.psam_superpoint_snap_workspace_bytes(K, N, N + 1) == 0

    # ---- normals: (xyz, inv, nbr, N, V, min_points, viewpoint, count, scatter, normal, curvature, ws, ws_bytes, stream)
    nv = lambda *a: lib.psam_normals_voxel(*a, None)
    base = [p, p, p, N, V, 5, None, p, None, p, p, p, big]
    for i in (0, 1, 2, 7, 9, 10, 11):
        a = list(base); a[i] = None
        rejected(nv(*a), b"null")
    for i, bad in ((3, 0), (3, -1), (4, 0), (4, N + 1), (3, (1 << 28) + 1)):
        a = list(base); a[i] = bad
        rejected(nv(*a), b"N <= 2^28")
    a = list(base); a[5] = 0
    rejected(nv(*a), b"min_points")
    view = (ctypes.c_float * 3)(0.0, float("inf"), 0.0)
    a = list(base); a[6] = ctypes.addressof(view)
    rejected(nv(*a), b"viewpoint")
    a = list(base); a[12] = V * 128 - 1
    rejected(nv(*a), b"workspace", -3)
    a = list(base); a[11] = p + 8
    rejected(nv(*a), b"aligned", -2)
    a = list(base); a[8] = p + 4
    rejected(nv(*a), b"aligned", -2)

    # ---- superpoints: (inv, nbr, count, normal, curvature, N, V, min_points, max_curvature, cos_angle, min_size, absorb_rounds, voxel_label,
    #                    point_label, size, num, ws, ws_bytes, stream)
    su = lambda *a: lib.psam_superpoints(*a, None)
    base = [p, p, p, p, p, N, V, 5, 0.08, 0.96, 50, 2, p, p, p, p, p, big]
    for i in (0, 1, 2, 3, 4, 12, 13, 14, 15, 16):
        a = list(base); a[i] = None
        rejected(su(*a), b"null")
    for i, bad in ((5, 0), (6, 0), (6, N + 1)):
        a = list(base); a[i] = bad
        rejected(su(*a), b"N <= 2^28")
    for i, bad in ((7, 0), (10, -1)):
        a = list(base); a[i] = bad
        rejected(su(*a), b"min_points >= 1")
    for bad in (-1, 65):
        a = list(base); a[11] = bad
        rejected(su(*a), b"absorb_rounds")
    for i, bad in ((8, -0.5), (8, float("nan")), (9, 1.5), (9, -1.5), (9, float("nan"))):
        a = list(base); a[i] = bad
        rejected(su(*a), b"cos_angle")
    a = list(base); a[17] = 6 * V * 4 + 128 + 16 - 1
    rejected(su(*a), b"workspace", -3)
    a = list(base); a[16] = p + 4
    rejected(su(*a), b"aligned", -2)

    # ---- snap: (bits, point_label, size, K, N, S, q16, bits_out, area_out, changed, ws, ws_bytes, stream)
    sn = lambda *a: lib.psam_superpoint_snap(*a, None)
    base = [p, p, p, K, N, S, 32768, q, p, p, p, big]
    for i in (0, 1, 2, 7, 8, 9, 10):
        a = list(base); a[i] = None
        rejected(sn(*a), b"null")
    for i, bad in ((3, 0), (3, 65536), (4, 0), (5, 0), (5, N + 1)):
        a = list(base); a[i] = bad
        rejected(sn(*a), b"K <= 65535")
    for bad in (-1, 65536):
        a = list(base); a[6] = bad
        rejected(sn(*a), b"q16")
    a = list(base); a[7] = p
    rejected(sn(*a), b"alias")
    a = list(base); a[11] = K * S * 4 - 1
    rejected(sn(*a), b"workspace", -3)
    a = list(base); a[10] = p + 8
    rejected(sn(*a), b"aligned", -2)
