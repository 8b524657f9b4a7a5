"""Automatic mask proposals, host side: the numpy reference on a case worked out by hand, ProposalConfig validation, the C entry points'
argument checks, header / binding sync, and the demo's /segment_all route against a stand-in predictor."""
import ctypes
import http.client
import json
import os
import re
import threading

import numpy as np
import pytest
import torch

import mask_reference as R
from point_sam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK_ENTRY_POINTS = ("psam_mask_pack", "psam_mask_valid", "psam_mask_intersections", "psam_mask_nms_workspace_bytes", "psam_mask_nms",
                     "psam_mask_paint_workspace_bytes", "psam_mask_paint")


def _six_masks():
    N = 20
    spans = [(0, 10), (0, 8), (10, 16), (8, 14), (16, 18), (0, 10)]
    logits = -np.ones((6, N), dtype=np.float32)
    for k, (a, b) in enumerate(spans):
        logits[k, a:b] = 1.0
    score = np.array([0.9, 0.8, 0.7, 0.95, 0.99, 0.9], dtype=np.float32)
    return N, logits, score


def test_reference_on_a_hand_worked_case():
    """Six masks on 20 points, IoU threshold 0.5, at least 3 points:

        mask  points   area  score        order by score (ties: lower index): 4, 3, 0, 5, 1, 2
        0     0..9     10    0.90         4: 2 points < 3 -> invalid, never kept, suppresses nothing
        1     0..7      8    0.80         3: first valid -> kept (rank 0)
        2     10..15    6    0.70         0: with 3: inter 2 (points 8, 9), union 14 -> 2 > 7 is false -> kept (rank 1)
        3     8..13     6    0.95         5: the same points as 0, same score, higher index: inter 10, union 10 -> 10 > 5 -> dropped
        4     16..17    2    0.99         1: with 3: inter 0; with 0: inter 8, union 10 -> 8 > 5 -> dropped
        5     0..9     10    0.90         2: with 3: inter 4 (points 10..13), union 8 -> 4 > 4 is FALSE (strict) -> kept (rank 2)

    keep = [1, 0, 1, 1, 0, 0]; labels: points 0..7 -> mask 0 (rank 1); 8..13 -> mask 3 (rank 0, better than masks 0 and 2 there);
    14, 15 -> mask 2 (rank 2); 16..19 -> -1 (mask 4 covers 16, 17 but is not kept)."""
    N, logits, score = _six_masks()
    out = R.proposals(logits, score, N, 0.0, 0.5, 3, 0.9, 0.0, 0.0, 0.5)
    assert out["area"].tolist() == [10, 8, 6, 6, 2, 10] and out["area_hi"].tolist() == out["area_lo"].tolist() == out["area"].tolist()
    assert out["order"].tolist() == [4, 3, 0, 5, 1, 2]
    assert out["valid"].tolist() == [True, True, True, True, False, True]
    assert out["inter"][0].tolist() == [10, 8, 0, 2, 0, 10] and out["inter"][2].tolist() == [0, 0, 6, 4, 0, 0]
    assert out["keep"].tolist() == [True, False, True, True, False, False]
    assert out["candidate"].tolist() == [3, 0, 2]
    assert out["labels"].tolist() == [1] * 8 + [0] * 6 + [2] * 2 + [-1] * 4
    # a hair under 0.5 and mask 2 goes as well: the decision is the strict fp64 comparison against the fp32 threshold
    below = np.nextafter(np.float32(0.5), np.float32(0))
    assert R.proposals(logits, score, N, 0.0, 0.5, 3, 0.9, 0.0, 0.0, below)["keep"].tolist() == [True, False, False, True, False, False]
    # the filter: "under 90 % of the cloud" is strict, the score cut is >=, NaN scores fail it
    area = np.array([18, 17, 5, 5]); sc = np.array([0.5, 0.5, np.nan, 0.25], dtype=np.float32)
    assert R.validity(area, area, area, sc, 20, 3, 0.9, 0.25, 1.0).tolist() == [False, True, False, True]
    assert R.validity(area, area - 1, area, sc, 20, 3, 0.9, 0.25, 1.0).tolist() == [False] * 4      # stability area_hi / area_lo < 1
    assert R.validity(area, area * 0, area * 0, sc, 20, 3, 0.9, 0.25, 0.0).tolist() == [False] * 4  # area_lo == 0


def test_reference_word_layout_and_fp32_matmul_shortcut():
    rng = np.random.default_rng(5)
    m = rng.random((7, 64 * 3 + 37)) < 0.4
    w = R.words(m)
    assert w.shape == (7, 4) and w.dtype == np.dtype("<u8")
    for k, n in ((0, 0), (3, 63), (4, 64), (6, 228)):
        assert bool((int(w[k, n // 64]) >> (n % 64)) & 1) == bool(m[k, n])
    assert (w[:, 3] >> np.uint64(37)).max() == 0                       # bits past N are zero
    assert np.array_equal(R.unwords(w, m.shape[1]), m)
    assert np.array_equal(R.intersections(m, m, exact_int=False), R.intersections(m, m))
    assert np.array_equal(R.intersections(m, m), np.array([[sum(bin(int(x & y)).count("1") for x, y in zip(w[i], w[j])) for j in range(7)] for i in range(7)]))


def test_proposal_config_validation():
    from point_sam_amd.proposals import ProposalConfig
    cfg = ProposalConfig().validate()
    assert (cfg.num_prompts, cfg.prompt_chunk, cfg.min_points, cfg.max_area_frac, cfg.nms_thresh) == (1024, 64, 25, 0.9, 0.7)
    for bad in (dict(num_prompts=0), dict(prompt_chunk=0), dict(num_prompts=1.5), dict(nms_thresh=1.5), dict(nms_thresh=-0.1), dict(min_points=-1),
                dict(stability_offset=-1.0), dict(max_area_frac=0.0), dict(mask_threshold=float("nan")), dict(pred_iou_thresh="high"), dict(num_prompts=True)):
        with pytest.raises(ValueError):
            ProposalConfig(**bad).validate()
    assert ProposalConfig.from_overrides({"num_prompts": 16, "nms_thresh": 0.5}).num_prompts == 16
    with pytest.raises(ValueError, match="unknown"):
        ProposalConfig.from_overrides({"nms_threshold": 0.5})


def test_mask_entry_points_are_declared_bound_and_exported():
    from point_sam_amd.build import build_library
    build_library()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pointsam_hip.h")).read()
    declared = set(re.findall(r"\b(psam_mask_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(MASK_ENTRY_POINTS)
    assert declared == {n for n in _lib.SIGNATURES if n.startswith("psam_mask_")}
    for n in MASK_ENTRY_POINTS:
        assert hasattr(lib, n), n
    assert "mask proposals */" in hdr
    assert lib.psam_version() == 100


def test_mask_entry_points_reject_bad_arguments_on_the_host():
    """Null pointers and empty shapes return -1 with a message before any launch (this runs without a GPU)."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)                     # a non-null pointer; never dereferenced: every call below is rejected on the host

    def rejected(status, word):
        assert status == -1
        msg = lib.psam_last_error_string()
        assert word in msg, msg

    rejected(lib.psam_mask_pack(None, 64, 1, 64, 0.0, 1.0, 0, None, None, None, None, None), b"null")
    rejected(lib.psam_mask_pack(p, 64, 1, 64, 0.0, 1.0, 0, p, p, p, None, None), b"null")
    rejected(lib.psam_mask_pack(p, 64, 0, 64, 0.0, 1.0, 0, p, p, p, p, None), b"K > 0")
    rejected(lib.psam_mask_pack(p, 64, 1, 0, 0.0, 1.0, 0, p, p, p, p, None), b"N > 0")
    rejected(lib.psam_mask_pack(p, 32, 1, 64, 0.0, 1.0, 0, p, p, p, p, None), b"ld >= N")
    rejected(lib.psam_mask_pack(p, 64, 1, 64, 0.0, 1.0, -1, p, p, p, p, None), b"dst_row")
    rejected(lib.psam_mask_valid(None, None, None, None, 4, 64, 1, 0.9, 0.0, 0.0, None, None), b"null")
    rejected(lib.psam_mask_valid(p, p, p, p, 0, 64, 1, 0.9, 0.0, 0.0, p, None), b"K > 0")
    rejected(lib.psam_mask_valid(p, p, p, p, 4, -5, 1, 0.9, 0.0, 0.0, p, None), b"N > 0")
    rejected(lib.psam_mask_intersections(None, None, 1, 1, 1, None, None), b"null")
    rejected(lib.psam_mask_intersections(p, p, 0, 1, 1, p, None), b"Ka > 0")
    rejected(lib.psam_mask_intersections(p, p, 1, 1, 0, p, None), b"W > 0")
    rejected(lib.psam_mask_nms(None, None, None, None, 4, 0.5, None, None, 0, None), b"null")
    rejected(lib.psam_mask_nms(p, p, p, p, 0, 0.5, p, p, 4096, None), b"K")
    rejected(lib.psam_mask_nms(p, p, p, p, 1 << 20, 0.5, p, p, 4096, None), b"K")
    assert lib.psam_mask_nms(p, p, p, p, 256, 0.5, p, p, 8, None) == -3 and b"workspace" in lib.psam_last_error_string()
    rejected(lib.psam_mask_paint(None, None, None, 4, 64, None, None, 0, None), b"null")
    rejected(lib.psam_mask_paint(p, p, p, 0, 64, p, p, 4096, None), b"K > 0")
    rejected(lib.psam_mask_paint(p, p, p, 4, 0, p, p, 4096, None), b"N > 0")
    assert lib.psam_mask_paint(p, p, p, 4096, 64, p, p, 8, None) == -3
    # workspaces: (K + 1) rows of ceil(K / 64) words for the suppression matrix and the start row; the count and the K ranked candidates
    assert lib.psam_mask_nms_workspace_bytes(3072) == 3073 * 48 * 8 and lib.psam_mask_nms_workspace_bytes(0) == 0
    assert lib.psam_mask_paint_workspace_bytes(3072) == 3073 * 4 and lib.psam_mask_paint_workspace_bytes(-1) == 0


def test_mask_bindings_refuse_cpu_tensors():
    from point_sam_amd import ops
    with pytest.raises(_lib.PointSamHipError):
        ops.mask_pack(torch.zeros(2, 64))
    with pytest.raises(_lib.PointSamHipError):
        ops.mask_intersections(torch.zeros(2, 1, dtype=torch.int64))
    assert ops.mask_words(64) == 1 and ops.mask_words(65) == 2 and ops.mask_words(2048 + 37) == 33
    bits = torch.from_numpy(R.words(np.array([[1, 0, 1] + [0] * 62 + [1]], dtype=bool)).view(np.int64))
    assert ops.mask_unpack(bits, 66).nonzero()[:, 1].tolist() == [0, 2, 65]


def test_predictor_generate_masks_needs_a_cloud():
    from point_sam_amd.predictor import PointSAMPredictor
    with pytest.raises(RuntimeError, match="set_pointcloud"):
        PointSAMPredictor(model=None).generate_masks()


# ------------------------------------------------------------------------------------------------ /segment_all against a stand-in predictor
class FakeProposals:
    def __init__(self, labels, score):
        self.labels, self.score = labels, score

    def __len__(self):
        return self.score.numel()


class FakePredictor:
    """Labels = index of the nearest of `num_prompts` anchor points (every point labelled), scores descending."""

    def __init__(self):
        self.cfgs = []

    def set_pointcloud(self, xyz, rgb):
        self.xyz = xyz

    def generate_masks(self, cfg):
        self.cfgs.append(cfg)
        k = cfg.num_prompts
        d = (self.xyz[0][:, None] - self.xyz[0][None, :k]).norm(dim=-1)
        return [FakeProposals(d.argmin(1).to(torch.int32), torch.linspace(0.9, 0.5, k))]


@pytest.fixture()
def server(tmp_path):
    from point_sam_amd.demo_server import DemoSession, serve
    pred = FakePredictor()
    sess = DemoSession(pred, models_dir=str(tmp_path), output_dir=str(tmp_path / "results"), device="cpu")
    srv = serve(sess, "127.0.0.1", 0)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    yield srv.server_address[1], sess, pred
    srv.shutdown()


def _req(port, method, path, body=None):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=10)
    c.request(method, path, None if body is None else json.dumps(body), {"Content-Type": "application/json"})
    r = c.getresponse()
    return r.status, json.loads(r.read())


def test_segment_all_route(server):
    port, sess, pred = server
    st, out = _req(port, "POST", "/segment_all", {})
    assert st == 400 and "point cloud" in out["error"]
    pts = np.random.RandomState(1).rand(40, 3)
    st, _ = _req(port, "POST", "/sampled_pointcloud", {"points": {str(i): float(v) for i, v in enumerate(pts.flatten())},
                                                      "colors": {str(i): 0.5 for i in range(120)}})
    assert st == 200
    st, out = _req(port, "POST", "/segment_all", {"num_prompts": 5, "nms_thresh": 0.5})
    assert st == 200 and out["num_masks"] == 5 and len(out["labels"]) == 40 and len(out["scores"]) == 5
    assert all(isinstance(v, int) and -1 <= v < 5 for v in out["labels"]) and out["labels"][:5] == [0, 1, 2, 3, 4]
    assert out["scores"] == sorted(out["scores"], reverse=True)
    assert pred.cfgs[-1].num_prompts == 5 and pred.cfgs[-1].nms_thresh == 0.5 and pred.cfgs[-1].min_points == 25
    st, out = _req(port, "POST", "/segment_all", {"num_prompts": 3, "iou": 0.5})          # unknown key -> 400 through _run
    assert st == 400 and "unknown" in out["error"] and "iou" in out["error"] and len(pred.cfgs) == 1
    st, out = _req(port, "POST", "/segment_all", {"nms_thresh": 7})                        # known key, bad value
    assert st == 400 and "nms_thresh" in out["error"]
    st, out = _req(port, "POST", "/segment_all", [1, 2])                                   # not an object
    assert st == 400
    # the click route and its state are untouched by a proposal pass
    assert sess.prompts == [] and sess.prompt_mask is None and sess.segment_mask is None


# ------------------------------------------------------------------------------------------------ the interval reference and the tested sizes
import kernel_sizes as KS


def _with_ties(K, seed):
    N, s, e, score, valid = R.interval_family(K, seed)
    if K >= 8:
        rng = np.random.default_rng(seed + 1)
        a, b = rng.choice(K, K // 8, replace=False), rng.choice(K, K // 8, replace=False)
        score[a] = score[b]                               # equal scores: the lower index goes first
        s[a[:K // 16]], e[a[:K // 16]] = s[b[:K // 16]], e[b[:K // 16]]      # and outright twins (IoU exactly 1) among them
    return N, s, e, score, valid


@pytest.mark.parametrize("K", [1, 65, 300])
@pytest.mark.parametrize("thr", [0.3, 0.5, 1.0])
def test_interval_reference_equals_the_mask_reference(K, thr):
    """nms_intervals / paint_intervals against nms() / paint() on the explicit boolean masks and the intersections() matrix, with score ties and
    duplicated masks; the closed-form areas and intersections against the counted ones; the reported suppressor really is the first one."""
    N, s, e, score, valid = _with_ties(K, 7 * K)
    assert N == 2 * K + 37 and (e - s).min() >= 4 and (e - s).max() <= 96 and s.min() >= 0 and e.max() <= N and score.dtype == np.float32
    masks = R.interval_masks(s, e, N)
    inter = R.intersections(masks, masks)
    assert np.array_equal(masks.sum(1), e - s)
    assert np.array_equal(inter, np.maximum(np.minimum(e[:, None], e[None]) - np.maximum(s[:, None], s[None]), 0))
    assert np.array_equal(R.interval_masks(s, e, N, slice(K // 2, K)), masks[K // 2:])
    order = R.order_of(score)
    if K >= 8:
        assert len(np.unique(score)) < K
    want = R.nms(order, valid, e - s, inter, thr)
    keep, sup = R.nms_intervals(s, e, order, valid, thr)
    assert np.array_equal(keep, want)
    assert np.array_equal(R.paint_intervals(s, e, order, keep, N), R.paint(masks, order, want))
    t = float(np.float32(thr))
    for p, i in enumerate(order):
        if sup[p] < 0:
            assert keep[i] or not valid[i]
            continue
        hits = [q for q in range(p) if keep[order[q]] and float(inter[i, order[q]]) > t * float(e[i] - s[i] + e[order[q]] - s[order[q]] - inter[i, order[q]])]
        assert not keep[i] and valid[i] and sup[p] == hits[0]
    if thr == 1.0:
        assert np.array_equal(keep, valid)                # nothing overlaps more than completely
    # out-of-range entries of `order` are no candidates: the result is that of the order without them
    if K >= 65:
        bad = order.copy()
        bad[[3, K // 2, K - 1]] = (-1, K, 2 ** 31 - 1)
        k2, s2 = R.nms_intervals(s, e, bad, valid, thr)
        short = np.delete(order, [3, K // 2, K - 1])
        k3, _ = R.nms_intervals(s, e, short, valid, thr)
        assert np.array_equal(k2, k3) and (s2[[3, K // 2, K - 1]] == -1).all()
        assert np.array_equal(R.paint_intervals(s, e, bad, k2, N), R.paint_intervals(s, e, short, k3, N))


def test_tested_sizes_follow_from_the_kernel_sources():
    """The size lists of tests/kernel_sizes.py (what the GPU tests run) equal what the constants and launches parsed from masks.hip and voxel_table.h
    (the scan of scene.hip and crops.hip) give.  A new nms_walk_kernel instance, another KW bound or a changed NMS_MAX_K / NMS_PF / RANK_THREADS /
    SCAN_THREADS fails here until the lists cover it."""
    c = KS.mask_constants()
    assert c["walks"] == [(1, 64), (2, 128), (4, 256)] and c["NMS_MAX_K"] == 16384 and c["NMS_PF"] == 8 and c["RANK_THREADS"] == 1024
    from point_sam_amd.proposals import MAX_CANDIDATES
    assert MAX_CANDIDATES == c["NMS_MAX_K"]
    assert KS.nms_sizes(c) == KS.NMS_SIZES == (4096, 4097, 4300, 8192, 8193, 8400, 12500, 16384)
    assert KS.NMS_SEGMENT == 64 * 64
    launched = {KS.walk_of(c, K) for K in KS.NMS_SIZES}
    assert launched == {nw for nw, _ in c["walks"]}                                  # every instance runs
    for nw, kw in c["walks"]:
        mine = [K for K in KS.NMS_SIZES if KS.walk_of(c, K) == nw]
        assert min(kw * 64, c["NMS_MAX_K"]) in mine                                  # at its last K: every word of the set full
        if nw > 1:
            assert any(K % 64 == 1 for K in mine)                                    # at its first: one live bit in the last word
            assert any(K % c["NMS_PF"] for K in mine)                                # a ragged prefetch group in a later word
    for s in range(1, max(launched)):                                                # every register s >= 1 of the set ends a walk part-way
        assert any(s * KS.NMS_SEGMENT + 64 < K < (s + 1) * KS.NMS_SEGMENT for K in KS.NMS_SIZES)
    assert set(KS.NMS_SEGMENT_SIZES) <= set(KS.NMS_SIZES) and {(K - 1) // KS.NMS_SEGMENT for K in KS.NMS_SEGMENT_SIZES} == set(range(1, max(launched)))
    first_r3 = min(K for K in KS.NMS_SIZES if (K + 63) // 64 > 192)
    assert first_r3 == 12500
    assert KS.paint_sizes(c) == KS.PAINT_SIZES
    assert [-(-K // c["RANK_THREADS"]) for K in KS.PAINT_SIZES] == [1, 1, 2, 3, 5]
    assert KS.valid_sizes(c) == KS.VALID_SIZES
    sc = KS.scan_constants()
    assert sc["SCAN_THREADS"] == sc["CROP_SCAN_THREADS"]      # one constant in voxel_table.h: scan_constants refuses a second definition in either file
    T = sc["SCAN_THREADS"]
    assert KS.scan_sizes(T) == KS.SCAN_SIZES
    assert [-(-(-(-M // T)) // T) for M in KS.SCAN_SIZES] == [1, 2, 3] and (-(-KS.SCAN_SIZES[2] // T)) % 3 != 0


@pytest.mark.parametrize("K", KS.NMS_SIZES)
def test_interval_family_exercises_every_segment_of_the_walk(K):
    """Conditions on the inputs of the GPU test (tests/test_gpu_mask_instances.py), asserted on the reference alone: equality on an all-kept or
    all-dropped case, or on one whose suppressions never cross a register of the walk's `removed` set, would prove nothing.  Positions are cut
    into segments of 4096 (64 words of the set: one register per lane)."""
    N, s, e, score, valid = R.interval_family(K, seed=K)
    order = R.order_of(score)
    keep, sup = R.nms_intervals(s, e, order, valid, 0.5)
    kept, dropped = keep[order], sup >= 0
    seg = np.arange(K) // KS.NMS_SEGMENT
    nseg = int(seg[-1]) + 1
    per_kept, per_drop = np.bincount(seg[kept], minlength=nseg), np.bincount(seg[dropped], minlength=nseg)
    print(f"K={K}: kept {int(kept.sum())} ({' / '.join(map(str, per_kept))}), suppressed {int(dropped.sum())} ({' / '.join(map(str, per_drop))}), "
          f"invalid {int((~valid).sum())}")
    assert kept.sum() >= K / 8 and dropped.sum() >= K / 8
    from_seg = np.where(dropped, sup // KS.NMS_SEGMENT, -1)
    for g in range(nseg):
        here = seg == g
        if K in KS.NMS_SEGMENT_SIZES:
            assert per_kept[g] >= 16 and per_drop[g] >= 64, (g, per_kept, per_drop)
            if g >= 1:
                assert (from_seg[here] == 0).any(), f"segment {g}: no position whose first suppressor lies in segment 0"
        if here.sum() >= 1024 and g >= 1:
            assert (from_seg[here] >= 1).any(), f"segment {g}: no position whose first suppressor lies in a segment >= 1"
