"""Full-resolution scenes, host side: header / binding sync of the new entry points, their argument checks (no GPU needed: every call is refused before a
launch), the voxel-size bisection against a fake counter, set_scene's argument validation, the numpy reference's own properties, and the demo session's
choice between set_scene and set_pointcloud against a stand-in predictor."""
import ctypes
import http.client
import json
import os
import re
import threading

import numpy as np
import pytest
import torch

import scene_reference as R
from point_sam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE_ENTRY_POINTS = ("psam_voxel_downsample_workspace_bytes", "psam_voxel_downsample", "psam_scene_expand_rows", "psam_scene_expand_bits")


def test_scene_entry_points_are_declared_bound_and_exported():
    from point_sam_amd.build import SOURCES, build_library
    build_library()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pointsam_hip.h")).read()
    declared = set(re.findall(r"\b(psam_(?:voxel|scene)_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(SCENE_ENTRY_POINTS)
    assert declared == {n for n in _lib.SIGNATURES if n.startswith(("psam_voxel_", "psam_scene_"))}
    for n in SCENE_ENTRY_POINTS:
        assert hasattr(lib, n) and not n.startswith("psam_mask_"), n
    assert ("scene.hip", ["-ffp-contract=off"]) in SOURCES
    assert "full-resolution scenes */" in hdr
    assert lib.psam_version() == 100


def test_the_voxel_table_and_the_row_popcount_live_in_one_file_each():
    """The table's format, its probe and the scan are csrc/voxel_table.h's: scene.hip, crops.hip and regions.hip include it and keep no copy.  The
    claiming compare-and-swap and the row popcount each occur in exactly one file of csrc/ (experiments/ aside)."""
    csrc = os.path.join(ROOT, "point_sam_amd", "csrc")
    table = open(os.path.join(csrc, "voxel_table.h")).read()
    for word in ("int voxel_claim(", "int voxel_find(", "int voxel_claim_run(", "void scan_block_offsets(", "constexpr int SCAN_THREADS", "struct VoxelWs"):
        assert table.count(word) == 1, word
    for f in ("scene.hip", "crops.hip", "regions.hip"):
        src = open(os.path.join(csrc, f)).read()
        assert '#include "voxel_table.h"' in src, f
        assert "atomicCAS(&keys" not in src and "VOXEL_EMPTY, key)" not in src and "__shfl_up" not in src and "make_uint4" not in src, f
    sources = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h", ".cpp"))}
    assert [f for f, src in sources.items() if "atomicCAS(&keys" in src] == ["voxel_table.h"]
    assert [f for f, src in sources.items() if "__popcll(row[w])" in src] == ["row_popcount.h"]
    assert sources["voxel_table.h"].count("atomicCAS(&keys") == 1 and sources["row_popcount.h"].count("__popcll(row[w])") == 1


def test_scene_entry_points_reject_bad_arguments_on_the_host():
    """Null pointers, empty shapes, a bad inv_h and a short workspace return -1 with a message before any launch."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15               # a non-null, aligned pointer; never dereferenced by the device: every call below is refused
    org = ctypes.addressof((ctypes.c_float * 3)(-1.0, -1.0, -1.0))
    keep = []

    def rejected(status, word):
        assert status == -1
        msg = lib.psam_last_error_string()
        assert word in msg, msg

    M = 1000
    need = lib.psam_voxel_downsample_workspace_bytes(M)
    # the table: 2048 slots (the power of two at or above 2 M) of an 8-byte key and a 4-byte index; one int32 per point; one per 1024 points + the total
    assert need == 2048 * 12 + 4000 + 16 and need >= 2 * M * 12
    assert lib.psam_voxel_downsample_workspace_bytes(0) == 0 and lib.psam_voxel_downsample_workspace_bytes(-3) == 0
    big = 1 << 30
    rejected(lib.psam_voxel_downsample(None, M, org, 4.0, p, p, p, p, p, big, None), b"null")
    rejected(lib.psam_voxel_downsample(p, M, None, 4.0, p, p, p, p, p, big, None), b"null")
    rejected(lib.psam_voxel_downsample(p, M, org, 4.0, p, p, None, p, p, big, None), b"null")
    rejected(lib.psam_voxel_downsample(p, M, org, 4.0, p, p, p, None, p, big, None), b"null")
    rejected(lib.psam_voxel_downsample(p, M, org, 4.0, p, p, p, p, None, big, None), b"null")
    rejected(lib.psam_voxel_downsample(p, M, org, 4.0, p, None, p, p, p, big, None), b"together")      # count-only means both null
    rejected(lib.psam_voxel_downsample(p, 0, org, 4.0, p, p, p, p, p, big, None), b"M")
    rejected(lib.psam_voxel_downsample(p, -7, org, 4.0, p, p, p, p, p, big, None), b"M")
    for bad in (0.0, -4.0, float("nan"), float("inf")):
        rejected(lib.psam_voxel_downsample(p, M, org, bad, p, p, p, p, p, big, None), b"inv_h")
    rejected(lib.psam_voxel_downsample(p, M, org, 4.0, p, p, p, p, p, need - 1, None), b"workspace")
    rejected(lib.psam_voxel_downsample(p, M, org, 4.0, None, None, p, p, p, need - 1, None), b"workspace")
    nan_org = (ctypes.c_float * 3)(-1.0, float("nan"), -1.0); keep.append(nan_org)
    rejected(lib.psam_voxel_downsample(p, M, ctypes.addressof(nan_org), 4.0, p, p, p, p, p, big, None), b"origin")

    rejected(lib.psam_scene_expand_rows(None, 8, p, 1, 8, 8, p, 8, None), b"null")
    rejected(lib.psam_scene_expand_rows(p, 8, None, 1, 8, 8, p, 8, None), b"null")
    rejected(lib.psam_scene_expand_rows(p, 8, p, 1, 8, 8, None, 8, None), b"null")
    rejected(lib.psam_scene_expand_rows(p, 8, p, 0, 8, 8, p, 8, None), b"R > 0")
    rejected(lib.psam_scene_expand_rows(p, 8, p, 1, 0, 8, p, 8, None), b"Nw > 0")
    rejected(lib.psam_scene_expand_rows(p, 8, p, 1, 8, 0, p, 8, None), b"M > 0")
    rejected(lib.psam_scene_expand_rows(p, 7, p, 1, 8, 8, p, 8, None), b"src_ld")
    rejected(lib.psam_scene_expand_rows(p, 8, p, 1, 8, 8, p, 7, None), b"dst_ld")

    rejected(lib.psam_scene_expand_bits(None, p, 1, 64, 64, p, p, None), b"null")
    rejected(lib.psam_scene_expand_bits(p, None, 1, 64, 64, p, p, None), b"null")
    rejected(lib.psam_scene_expand_bits(p, p, 1, 64, 64, None, None, None), b"null")
    rejected(lib.psam_scene_expand_bits(p, p, 0, 64, 64, p, None, None), b"K > 0")
    rejected(lib.psam_scene_expand_bits(p, p, 1, 0, 64, p, None, None), b"Nw > 0")
    rejected(lib.psam_scene_expand_bits(p, p, 1, 64, -1, p, None, None), b"M > 0")


def test_scene_bindings_refuse_cpu_tensors_and_bad_sizes():
    from point_sam_amd import ops
    with pytest.raises(_lib.PointSamHipError):
        ops.voxel_downsample(torch.zeros(8, 3), 0.5)
    with pytest.raises(_lib.PointSamHipError):
        ops.voxel_count(torch.zeros(8, 3), 0.5)
    with pytest.raises(_lib.PointSamHipError):
        ops.scene_expand_rows(torch.zeros(2, 8), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(_lib.PointSamHipError):
        ops.scene_expand_bits(torch.zeros(2, 1, dtype=torch.int64), torch.zeros(4, dtype=torch.int64), 64)


def test_choose_voxel_size_replays_the_bisection():
    from point_sam_amd.scene import choose_voxel_size
    for threshold_k in (0, 1, 17, 40, 79, 80):
        asked = []

        def count(k):                                      # monotone: sizes up to threshold_k fit
            asked.append(k)
            return 100 if k <= threshold_k else 101

        h = choose_voxel_size(None, 100, count)
        lo, hi, want = 0, 80, [0]
        while hi - lo > 1:
            mid = (lo + hi) // 2
            want.append(mid)
            if mid <= threshold_k:
                lo = mid
            else:
                hi = mid
        assert asked == want and 7 <= len(asked) <= 8
        assert h == 2.0 ** (1 - lo / 4) and lo == min(threshold_k, 79)      # k = 80 itself is never the answer of this bisection
    with pytest.raises(ValueError, match="max_points"):
        choose_voxel_size(None, 100, lambda k: 101)
    for bad in (0, -1, 2.5, True, None):
        with pytest.raises(ValueError):
            choose_voxel_size(None, bad, lambda k: 1)


class _NoModel:
    """set_scene validates before it touches the model."""
    def __getattr__(self, name):
        raise AssertionError("the model must not be reached")


def test_set_scene_argument_validation():
    from point_sam_amd.predictor import PointSAMPredictor
    pred = PointSAMPredictor(_NoModel())
    xyz, rgb = torch.zeros(10, 3), torch.zeros(10, 3)
    for kw in (dict(), dict(voxel_size=0.1, max_points=5), dict(voxel_size=0.0), dict(voxel_size=-1.0), dict(voxel_size=float("nan")),
               dict(voxel_size=float("inf")), dict(max_points=0), dict(max_points=2.5), dict(max_points=True)):
        with pytest.raises(ValueError):
            pred.set_scene(xyz, rgb, **kw)
    with pytest.raises(ValueError, match="B = 1"):
        pred.set_scene(torch.zeros(2, 10, 3), torch.zeros(2, 10, 3), max_points=5)
    with pytest.raises(ValueError):
        pred.set_scene(xyz, torch.zeros(9, 3), max_points=5)
    with pytest.raises(ValueError):
        pred.set_scene(torch.zeros(10, 2), torch.zeros(10, 2), max_points=5)
    assert pred.scene is None
    with pytest.raises(RuntimeError):
        pred.predict_masks(torch.zeros(1, 1, 3), torch.ones(1, 1, dtype=torch.int64))


def test_reference_properties():
    rng = np.random.default_rng(0)
    xyz = rng.uniform(-1, 1, (5000, 3)).astype(np.float32)
    xyz[100:200] = xyz[0]                                  # a crowded voxel
    for h in (0.5, 0.2, 0.0625):
        keep_idx, inv = R.downsample(xyz, h)
        k = R.keys(xyz, h)
        assert np.array_equal(inv[keep_idx], np.arange(len(keep_idx)))
        assert (np.diff(keep_idx) > 0).all()
        assert (keep_idx[inv] <= np.arange(len(xyz))).all()
        assert np.array_equal(k[keep_idx[inv]], k) and len(keep_idx) == len(np.unique(k))
    # a hand-worked case, h = 1: cells along x of -1, -0.0, 0.5, 1.0, -0.5 are 0, 1, 1, 2, 0
    pts = np.array([[-1, -1, -1], [-0.0, -1, -1], [0.5, -1, -1], [1.0, -1, -1], [-0.5, -1, -1]], dtype=np.float32)
    keep_idx, inv = R.downsample(pts, 1.0)
    assert keep_idx.tolist() == [0, 1, 3] and inv.tolist() == [0, 1, 1, 2, 0]
    for bad in (np.nan, np.inf, -np.inf, -1.5):
        q = pts.copy(); q[2, 1] = bad
        with pytest.raises(ValueError):
            R.downsample(q, 1.0)
    with pytest.raises(ValueError):                        # x = 1 at h = 2^-20: cell 2^21, one past the last
        R.downsample(pts, 2.0 ** -20)
    assert len(R.downsample(np.where(pts == 1.0, np.float32(1 - 2.0 ** -20), pts), 2.0 ** -20)[0]) == 5
    m = rng.random((3, 130)) < 0.5
    w = R.words(m)
    assert w.shape == (3, 3) and (w[:, 2] >> np.uint64(2)).max() == 0 and np.array_equal(R.unwords(w, 130), m)
    inv = rng.integers(0, 130, 1000)
    wf, area = R.expand_bits(w, inv, 130)
    assert np.array_equal(R.unwords(wf, 1000), m[:, inv]) and np.array_equal(area, m[:, inv].sum(1))


# ------------------------------------------------------------------------------------------------ the demo session against a stand-in predictor
class FakePredictor:
    def __init__(self):
        self.calls = []

    def set_pointcloud(self, xyz, rgb):
        self.calls.append(("set_pointcloud", tuple(xyz.shape)))
        self.n = xyz.shape[1]

    def set_scene(self, xyz, rgb, voxel_size=None, max_points=None):
        self.calls.append(("set_scene", tuple(xyz.shape), voxel_size, max_points))
        self.n = xyz.shape[1]

    def predict_masks(self, pts, lab, prompt_mask, multimask):
        assert prompt_mask is None or tuple(prompt_mask.shape) == (1, self.n)
        logits = torch.linspace(-1, 1, self.n).repeat(1, 3 if multimask else 1, 1)
        return logits, torch.tensor([[0.1, 0.9, 0.5][:logits.shape[1]]]), logits


@pytest.mark.parametrize("working_points", [None, 16])
def test_demo_session_uses_set_scene_only_when_asked(tmp_path, working_points):
    from point_sam_amd.demo_server import DemoSession, serve
    pred = FakePredictor()
    kw = {} if working_points is None else {"working_points": working_points}
    sess = DemoSession(pred, models_dir=str(tmp_path), output_dir=str(tmp_path / "results"), device="cpu", **kw)
    srv = serve(sess, "127.0.0.1", 0)
    threading.Thread(target=srv.serve_forever, daemon=True).start()

    def req(path, body):
        c = http.client.HTTPConnection("127.0.0.1", srv.server_address[1], timeout=10)
        c.request("POST", path, json.dumps(body), {"Content-Type": "application/json"})
        r = c.getresponse()
        return r.status, json.loads(r.read())

    try:
        pts = np.random.RandomState(1).rand(40, 3)
        st, _ = req("/sampled_pointcloud", {"points": {str(i): float(v) for i, v in enumerate(pts.flatten())}, "colors": {str(i): 0.5 for i in range(120)}})
        assert st == 200
        for click in range(2):
            st, out = req("/segment", {"prompt_point": [0.1, 0.2, 0.3], "prompt_label": 1})
            assert st == 200 and len(out["seg"]) == 40 and all(isinstance(v, bool) for v in out["seg"])
        want = ("set_pointcloud", (1, 40, 3)) if working_points is None else ("set_scene", (1, 40, 3), None, 16)
        assert pred.calls == [want, want]
    finally:
        srv.shutdown()


def test_demo_main_has_the_working_points_option():
    src = open(os.path.join(ROOT, "point_sam_amd", "demo_server.py")).read()
    assert '"--working-points"' in src and "working_points=args.working_points" in src
