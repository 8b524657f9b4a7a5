"""Connected-component clean-up, host side: header / binding sync of the new entry points, their argument checks (no GPU needed: every call is refused
before a launch), the numpy / scipy reference on a hand-worked case, the configs' validation, and the demo's /segment with clean_min_points against a
stand-in predictor."""
import ctypes
import http.client
import json
import os
import re
import threading

import numpy as np
import pytest
import torch

import region_reference as R
import scene_reference as SR
from point_sam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGION_ENTRY_POINTS = ("psam_region_neighbors_workspace_bytes", "psam_region_neighbors", "psam_region_labels_workspace_bytes", "psam_region_labels",
                       "psam_region_clean_workspace_bytes", "psam_region_clean")


# ------------------------------------------------------------------------------------------------ header and binding
def test_region_entry_points_are_declared_bound_and_exported():
    from point_sam_amd.build import SOURCES, build_library
    build_library()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pointsam_hip.h")).read()
    declared = set(re.findall(r"\b(psam_region_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(REGION_ENTRY_POINTS)
    assert declared == {n for n in _lib.SIGNATURES if n.startswith("psam_region_")}
    for n in REGION_ENTRY_POINTS:
        assert hasattr(lib, n) and not re.match(r"psam_(mask|voxel|scene)_", n), n
    assert ("regions.hip", ["-ffp-contract=off"]) in SOURCES
    assert "connected components of masks */" in hdr
    assert lib.psam_version() == 100


def test_region_entry_points_reject_bad_arguments_on_the_host():
    """Null pointers, bad shapes and aliasing return -1 with a message, a short workspace -3, all before any launch."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15               # a non-null, aligned pointer; never dereferenced by the device: every call below is refused
    q = p + 256
    org_buf = (ctypes.c_float * 3)(-1.0, -1.0, -1.0)      # read by the host checks: kept alive for the whole test
    org = ctypes.addressof(org_buf)
    keep = [org_buf]
    big = 1 << 40

    def rejected(status, word, code=-1):
        assert status == code, status
        msg = lib.psam_last_error_string()
        assert word in msg, msg

    # ---- workspace sizes for one stated shape: V = 1000 voxels, K = 7 rows, N = 5000 points
    V, K, N = 1000, 7, 5000
    # the table: 2048 slots (the power of two at or above 2 V) of an 8-byte key and a 4-byte rank
    assert lib.psam_region_neighbors_workspace_bytes(V) == 2048 * 12
    # labels: member counts and parents, [K, V] int32 each
    assert lib.psam_region_labels_workspace_bytes(K, N, V) == 2 * K * V * 4
    # clean: counts, parents, sizes (and seed flags with S > 0), [K, V] int32 each; per row an int32 `active`, an int32 `any seed` (each padded
    # to 16 bytes: 32) and a 64-bit `largest` (56 -> 64)
    assert lib.psam_region_clean_workspace_bytes(K, N, V, 0) == 3 * K * V * 4 + 32 + 32 + 64
    assert lib.psam_region_clean_workspace_bytes(K, N, V, 3) == 4 * K * V * 4 + 32 + 32 + 64
    for bad in (0, -3):
        assert lib.psam_region_neighbors_workspace_bytes(bad) == 0
        assert lib.psam_region_labels_workspace_bytes(bad, N, V) == 0 and lib.psam_region_labels_workspace_bytes(K, bad, V) == 0
        assert lib.psam_region_labels_workspace_bytes(K, N, bad) == 0
        assert lib.psam_region_clean_workspace_bytes(bad, N, V, 0) == 0 and lib.psam_region_clean_workspace_bytes(K, bad, V, 0) == 0
        assert lib.psam_region_clean_workspace_bytes(K, N, bad, 0) == 0
    assert lib.psam_region_clean_workspace_bytes(K, N, V, -1) == 0
    assert lib.psam_region_labels_workspace_bytes(65536, N, V) == 0      # rows are a grid dimension

    # ---- neighbours: (xyz, keep_idx, V, origin, inv_h, nbr, ws, ws_bytes, stream)
    nb = lambda *a: lib.psam_region_neighbors(*a, None)
    for i in (0, 1, 3, 5, 6):
        a = [p, p, V, org, 4.0, p, p, big]
        a[i] = None
        rejected(nb(*a), b"null")
    rejected(nb(p, p, 0, org, 4.0, p, p, big), b"V")
    rejected(nb(p, p, -2, org, 4.0, p, p, big), b"V")
    for bad in (0.0, -4.0, float("nan"), float("inf")):
        rejected(nb(p, p, V, org, bad, p, p, big), b"inv_h")
    nan_org = (ctypes.c_float * 3)(-1.0, float("nan"), -1.0); keep.append(nan_org)
    rejected(nb(p, p, V, ctypes.addressof(nan_org), 4.0, p, p, big), b"origin")
    rejected(nb(p, p, V, org, 4.0, p, p, 2048 * 12 - 1), b"workspace", -3)
    rejected(nb(p, p, V, org, 4.0, p, p + 4, big), b"aligned", -2)

    # ---- labels: (bits, inv, nbr, K, N, V, complement, labels, ws, ws_bytes, stream)
    lb = lambda *a: lib.psam_region_labels(*a, None)
    for i in (0, 1, 2, 7, 8):
        a = [p, p, p, K, N, V, 0, p, p, big]
        a[i] = None
        rejected(lb(*a), b"null")
    for i in (3, 4, 5):
        for bad in (0, -1):
            a = [p, p, p, K, N, V, 0, p, p, big]
            a[i] = bad
            rejected(lb(*a), b"K <= 65535")
    rejected(lb(p, p, p, 65536, N, V, 0, p, p, big), b"65535")
    rejected(lb(p, p, p, K, N, V, 1, p, p, 2 * K * V * 4 - 1), b"workspace", -3)

    # ---- clean: (bits, select, inv, nbr, seeds, K, N, V, S, min_island, min_hole, bits_out, area_out, changed, ws, ws_bytes, stream)
    cl = lambda *a: lib.psam_region_clean(*a, None)
    base = [p, None, p, p, None, K, N, V, 0, 5, 5, q, p, p, p, big]
    for i in (0, 2, 3, 11, 12, 13, 14):
        a = list(base)
        a[i] = None
        rejected(cl(*a), b"null")
    for i in (5, 6, 7):
        for bad in (0, -1):
            a = list(base)
            a[i] = bad
            rejected(cl(*a), b"K <= 65535")
    a = list(base); a[8] = -1
    rejected(cl(*a), b"S >= 0")
    a = list(base); a[8] = 2                               # S > 0 without seeds
    rejected(cl(*a), b"seeds")
    a = list(base); a[9] = -1
    rejected(cl(*a), b"negative")
    a = list(base); a[10] = -1
    rejected(cl(*a), b"negative")
    a = list(base); a[11] = p                              # bits_out == bits
    rejected(cl(*a), b"alias")
    a = list(base); a[15] = 3 * K * V * 4 + 128 - 1
    rejected(cl(*a), b"workspace", -3)
    a = list(base); a[4] = p; a[8] = 3; a[15] = 3 * K * V * 4 + 128      # enough without seeds, short with them
    rejected(cl(*a), b"workspace", -3)


# ------------------------------------------------------------------------------------------------ the reference on a hand-worked case
def _hand_case():
    """21 points on the cells of one row (y = z = 0) of a grid of h = 0.25; a point's cell is its x cell.  In point order:

        point  0  1  2  3  4  5  6  7  8  9 10 11 12 13 14 15 16 17 18 19 20
        cell   0  0  1  3  3  4  6  6  8  2  5  7  9 11 12 13 13 14 15 16 17

    Voxel ranks follow the first point of each cell: cells 0, 1, 3, 4, 6, 8 have ranks 0 .. 5, then cells 2, 5, 7, 9, 11, 12, 13, 14, 15, 16, 17 ranks
    6 .. 16.  Cells are adjacent when they differ by 1, so the cloud is the chain of cells 0 .. 9 (points 0 .. 12) and the chain 11 .. 17 (points
    13 .. 20), not joined (cell 10 is empty)."""
    cell = [0, 0, 1, 3, 3, 4, 6, 6, 8, 2, 5, 7, 9, 11, 12, 13, 13, 14, 15, 16, 17]
    xyz = np.array([[-1 + (c + 0.5) * 0.25, -0.9, -0.9] for c in cell], dtype=np.float32)
    return R.Graph(xyz, 0.25), cell


def test_reference_on_a_hand_worked_case():
    g, cell = _hand_case()
    assert g.keep_idx.tolist() == [0, 2, 3, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15, 17, 18, 19, 20]
    assert g.inv.tolist() == [0, 0, 1, 2, 2, 3, 4, 4, 5, 6, 7, 8, 9, 10, 11, 12, 12, 13, 14, 15, 16]
    # rank 1 is cell 1: its neighbours along x are cell 0 (rank 0) at offset (0, 0, -1) = index 12 and cell 2 (rank 6) at (0, 0, +1) = index 13
    assert R.OFFSETS[12] == (0, 0, -1) and R.OFFSETS[13] == (0, 0, 1)
    assert g.nbr[1].tolist() == [-1] * 12 + [0, 6] + [-1] * 12
    assert g.nbr[0].tolist() == [-1] * 13 + [1] + [-1] * 12      # cell 0: nothing below (out of range), cell 1 above

    # the mask: points 0 1 2 | 3 4 5 | 6 7 | 13 14  (point 9, cell 2, and point 10, cell 5, are missing: they split the first chain)
    mask = np.zeros(21, dtype=bool)
    mask[[0, 1, 2, 3, 4, 5, 6, 7, 13, 14]] = True
    lab, sizes = R.components(g, mask)
    #   cells 0 1 (ranks 0 1): id 0, 3 points;  cells 3 4 (ranks 2 3): id 2, 3 points;  cell 6 (rank 4): id 4, 2 points;  cells 11 12 (ranks 10 11): id 10
    assert sizes == {0: 3, 2: 3, 4: 2, 10: 2}
    assert lab.tolist() == [0, 0, 0, 2, 2, 2, 4, 4, -1, -1, -1, -1, -1, 10, 10, -1, -1, -1, -1, -1, -1]
    # the complement: point 9 (cell 2, rank 6) alone; point 10 (cell 5, rank 7) alone; cells 7 8 9 (points 11, 8, 12: ranks 8, 5, 9): id 5, 3 points;
    # cells 13 .. 17 (points 15 .. 20, ranks 12 .. 16): id 12, 6 points
    clab, csizes = R.components(g, ~mask)
    assert csizes == {6: 1, 7: 1, 5: 3, 12: 6}
    assert clab[[9, 10, 11, 8, 12]].tolist() == [6, 7, 5, 5, 5] and (clab[15:] == 12).all()

    # islands, every component small (min_island = 4): the largest stays; sizes 3 and 3 tie, the lower id (0) wins
    out, tr = R.clean_row(g, mask, min_island=4)
    assert np.flatnonzero(out).tolist() == [0, 1, 2] and tr["tie"] and tr["kept_small_largest"] and tr["removed"] == 3
    # islands at the threshold: min_island = 3 keeps both components of exactly 3 points, removes the two of 2
    out, tr = R.clean_row(g, mask, min_island=3)
    assert np.flatnonzero(out).tolist() == [0, 1, 2, 3, 4, 5] and tr["removed"] == 2 and not tr["kept_small_largest"]
    # holes exactly at the threshold: min_hole = 3 fills the two single-point holes, not the hole of exactly 3 points; min_hole = 4 fills it too
    out, tr = R.clean_row(g, mask, min_hole=3)
    assert np.flatnonzero(out).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 13, 14] and tr["filled"] == 2
    out, tr = R.clean_row(g, mask, min_hole=4)
    assert np.flatnonzero(out).tolist() == list(range(15)) and tr["filled"] == 3
    # both: the filled holes join cells 0 .. 6 into one island of 10 points; the 2-point island on cells 11 12 then falls to min_island = 3
    out, tr = R.clean_row(g, mask, min_island=3, min_hole=3)
    assert np.flatnonzero(out).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 9, 10] and tr["filled"] == 2 and tr["removed"] == 1
    # seeds outside the mask (point 8), unused (-1) and out of range: the row is left as step 2 made it
    out, tr = R.clean_row(g, mask, min_island=3, seeds=[8, -1, 99])
    assert np.flatnonzero(out).tolist() == [0, 1, 2, 3, 4, 5] and not tr["seeded"]
    # a seed in a component that step 2 removed (point 6) does not count; one in a surviving component (point 4) keeps that one alone
    out, tr = R.clean_row(g, mask, min_island=3, seeds=[6, -1])
    assert np.flatnonzero(out).tolist() == [0, 1, 2, 3, 4, 5] and not tr["seeded"]
    out, tr = R.clean_row(g, mask, min_island=3, seeds=[6, 4])
    assert np.flatnonzero(out).tolist() == [3, 4, 5] and tr["seeded"] and tr["seed_dropped"] == 1
    # an empty mask stays empty, whatever min_hole says
    out, _ = R.clean_row(g, np.zeros(21, dtype=bool), min_hole=100)
    assert not out.any()
    # rows: select, area, changed
    masks = np.stack([mask, mask, np.ones(21, dtype=bool)])
    out, area, changed, _ = R.clean(g, masks, min_island=3, select=[1, 0, 1])
    assert area.tolist() == [6, 10, 21] and changed.tolist() == [1, 0, 0] and np.array_equal(out[1], mask)


# ------------------------------------------------------------------------------------------------ configs and wrappers
def test_region_config_validation_and_defaults():
    from point_sam_amd.regions import RegionConfig
    d = RegionConfig().validate()
    assert (d.min_island, d.min_hole, d.voxel_size, d.points_per_voxel, d.keep_clicked) == (0, 0, None, 4, False)
    RegionConfig(min_island=30, min_hole=7, voxel_size=0.05, points_per_voxel=1, keep_clicked=True).validate()
    for bad in (dict(min_island=-1), dict(min_hole=-1), dict(min_island=2.5), dict(min_hole=True), dict(points_per_voxel=0), dict(points_per_voxel=1.5),
                dict(voxel_size=0.0), dict(voxel_size=-0.1), dict(voxel_size=float("inf")), dict(voxel_size=float("nan")), dict(voxel_size="0.1"),
                dict(keep_clicked=1)):
        with pytest.raises(ValueError):
            RegionConfig(**bad).validate()


def test_proposal_config_region_fields():
    from point_sam_amd.proposals import DeviceProposals, ProposalConfig, Proposals
    import dataclasses
    d = ProposalConfig().validate()
    assert (d.min_region_points, d.region_voxel_size, d.region_points_per_voxel) == (0, 0.0, 4), "the feature is off by default"
    ProposalConfig.from_overrides({"min_region_points": 25, "region_voxel_size": 0.04, "region_points_per_voxel": 2})
    for bad in ({"min_region_points": -1}, {"min_region_points": 2.5}, {"min_region_points": True}, {"region_voxel_size": -0.1},
                {"region_voxel_size": float("nan")}, {"region_voxel_size": float("inf")}, {"region_points_per_voxel": 0}, {"region_points_per_voxel": 1.5}):
        with pytest.raises(ValueError):
            ProposalConfig.from_overrides(bad)
    assert dataclasses.fields(DeviceProposals)[-1].name == "changed" and dataclasses.fields(Proposals)[-1].name == "changed"
    assert dataclasses.fields(Proposals)[-1].default is None


def test_region_bindings_refuse_cpu_tensors():
    from point_sam_amd import ops, regions
    inv, nbr = torch.zeros(64, dtype=torch.int64), torch.full((4, 26), -1, dtype=torch.int32)
    bits = torch.zeros(2, 1, dtype=torch.int64)
    with pytest.raises(_lib.PointSamHipError):
        ops.region_neighbors(torch.zeros(8, 3), torch.zeros(2, dtype=torch.int64), 0.5)
    with pytest.raises(_lib.PointSamHipError):
        ops.region_labels(bits, inv, nbr)
    with pytest.raises(_lib.PointSamHipError):
        ops.region_clean(bits, inv, nbr, 3, 3)
    with pytest.raises(_lib.PointSamHipError):
        regions.build_graph(torch.zeros(8, 3), voxel_size=0.5)
    with pytest.raises(ValueError):
        regions.build_graph(torch.zeros(2, 8, 3), voxel_size=0.5)


class _NoModel:
    def __getattr__(self, name):
        raise AssertionError("the model must not be reached")


def test_clean_masks_without_a_cloud_raises():
    from point_sam_amd.predictor import PointSAMPredictor
    from point_sam_amd.regions import RegionConfig
    pred = PointSAMPredictor(_NoModel())
    with pytest.raises(RuntimeError, match="set_pointcloud"):
        pred.clean_masks(torch.zeros(1, 3, 64), RegionConfig(min_island=3))


def test_propose_on_device_needs_graphs_when_the_cleanup_is_on():
    from types import SimpleNamespace
    from point_sam_amd.proposals import ProposalConfig, build_region_graphs, propose_on_device
    state = SimpleNamespace(coords=torch.zeros(2, 128, 3))
    with pytest.raises(ValueError, match="region graph"):
        propose_on_device(_NoModel(), state, ProposalConfig(num_prompts=4, min_region_points=5))
    with pytest.raises(ValueError, match="region graph"):
        propose_on_device(_NoModel(), state, ProposalConfig(num_prompts=4, min_region_points=5), graphs=[object()])      # one graph, two clouds
    assert build_region_graphs(state, ProposalConfig()) is None, "off by default: no graph is built"


# ------------------------------------------------------------------------------------------------ /segment with clean_min_points
class CleaningPredictor:
    """Three candidates, the best (index 1) positive on the first 30 points.  clean_masks records its call and answers with the first 10 points."""

    def __init__(self):
        self.cleaned = []

    def set_pointcloud(self, xyz, rgb):
        self.n = xyz.shape[1]

    def predict_masks(self, pts, labels, prompt_mask, multimask):
        C = 3 if multimask else 1
        logit = torch.where(torch.arange(self.n) < 30, 1.0, -1.0)
        logits = torch.stack([logit + 0.01 * i for i in range(C)])[None]
        return logits, torch.tensor([[0.1, 0.9, 0.3][:C]]), logits

    def clean_masks(self, logits, cfg, prompt_points=None, prompt_labels=None, threshold=0.0):
        self.cleaned.append((logits.clone(), cfg, prompt_points.clone(), prompt_labels.clone(), threshold))
        m = torch.zeros(1, self.n, dtype=torch.bool)
        m[0, :10] = True
        return torch.from_numpy(SR.words(m.numpy()).view(np.int64)), torch.tensor([10], dtype=torch.int32), torch.tensor([1], dtype=torch.uint8)


def _post(port, path, body):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=10)
    c.request("POST", path, json.dumps(body), {"Content-Type": "application/json"})
    r = c.getresponse()
    return r.status, json.loads(r.read())


@pytest.mark.parametrize("clean", [None, 7])
def test_segment_answers_with_the_cleaned_mask_when_asked(clean):
    from point_sam_amd.demo_server import DemoSession, serve
    from point_sam_amd.regions import RegionConfig
    pred = CleaningPredictor()
    sess = DemoSession(pred, device="cpu", clean_min_points=clean)
    srv = serve(sess, "127.0.0.1", 0)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    try:
        port = srv.server_address[1]
        n = 70
        xyz = np.random.RandomState(0).rand(n, 3)
        st, _ = _post(port, "/sampled_pointcloud", {"points": {str(i): float(v) for i, v in enumerate(xyz.flatten())},
                                                    "colors": {str(i): 0.5 for i in range(3 * n)}})
        assert st == 200
        st, out = _post(port, "/segment", {"prompt_point": [0.1, 0.2, 0.3], "prompt_label": 1})
        assert st == 200 and len(out["seg"]) == n
        if clean is None:
            assert out["seg"] == [i < 30 for i in range(n)] and pred.cleaned == [], "unset, /segment behaves as before"
        else:
            assert out["seg"] == [i < 10 for i in range(n)]
            (logits, cfg, pts, lab, thr), = pred.cleaned
            assert tuple(logits.shape) == (1, 1, n) and torch.equal(logits[0, 0], torch.where(torch.arange(n) < 30, 1.0, -1.0) + 0.01)      # the best candidate
            assert cfg == RegionConfig(min_island=7, min_hole=7, keep_clicked=True) and thr == 0.0
            assert pts.shape == (1, 1, 3) and lab.tolist() == [[1]]
            assert sess.segment_mask.dtype == torch.bool and int(sess.segment_mask.sum()) == 10
            # the dense prompt of the next click is still the raw logits of the best candidate
            assert torch.equal(sess.prompt_mask[0], logits[0, 0])
    finally:
        srv.shutdown()
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            DemoSession(pred, device="cpu", clean_min_points=bad)
