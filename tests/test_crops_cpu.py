"""Scene crops, host side: the numpy reference's own invariants, header / binding sync and host-side argument checks of the new entry points (every call
is refused before a launch), build_crop's arguments and its voxel-size bisection against a fake counter, CropLayerConfig, the multi-crop merge with the
kernels stubbed, the predictor's crop state machine against a stub model, and the demo's /crop routes against a stand-in predictor."""
import ctypes
import http.client
import json
import os
import re
import shutil
import subprocess
import threading
import types

import numpy as np
import pytest
import torch

import crop_reference as C
import scene_reference as R
from point_sam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CROP_ENTRY_POINTS = ("psam_crop_downsample_workspace_bytes", "psam_crop_downsample", "psam_crop_expand_rows", "psam_crop_expand_bits")
f32 = np.float32


# ------------------------------------------------------------------------------------------------ the reference
def test_reference_invariants():
    rng = np.random.default_rng(0)
    xyz = rng.uniform(-1, 1, (6000, 3)).astype(f32)
    xyz[100:200] = xyz[0] = (0.2, -0.1, 0.0)              # a crowded voxel inside the ball
    xyz[300] = np.nan
    rgb = rng.uniform(-1, 1, (6000, 3)).astype(f32)
    center, r = (0.1, -0.2, 0.05), 0.6
    _, q, member = C.ball(xyz, center, r)
    assert 0 < member.sum() < 6000 and not member[300]
    for h in (None, 0.5, 0.2, 0.0625):
        keep_idx, inv, wxyz, wrgb, members = C.crop_downsample(xyz, rgb, center, r, h)
        assert members == member.sum()
        assert np.array_equal(inv[keep_idx], np.arange(len(keep_idx)))
        assert (np.diff(keep_idx) > 0).all()
        assert np.array_equal(inv == -1, ~member)                                       # -1 exactly off the ball
        assert member[keep_idx].all() and (keep_idx[inv[member]] <= np.nonzero(member)[0]).all()      # a representative is a member of no higher index
        assert np.abs(wxyz).max() <= 1 and np.array_equal(wrgb, rgb[keep_idx])
        assert len(keep_idx) == members if h is None else len(keep_idx) < members
    assert C.crop_downsample(xyz, rgb, (5.0, 0, 0), 0.1, 0.2)[0].size == 0
    # expand: rows take the fill, bits zero, off the ball
    inv = np.array([2, -1, 0, 0, -1], dtype=np.int64)
    assert C.expand_rows(np.array([[1.0, 2.0, 3.0]], dtype=f32), inv, f32(-np.inf)).tolist() == [[3.0, -np.inf, 1.0, 1.0, -np.inf]]
    bits, area = C.expand_bits(R.words(np.array([[True, False, True], [False, True, False]])), inv, 3)
    assert R.unwords(bits, 5).tolist() == [[True, False, True, True, False], [False] * 5] and area.tolist() == [3, 0]
    # prompts: the kernel's arithmetic; a point off the ball is refused
    p = C.crop_prompts(xyz[member][:7], center, r)
    assert np.array_equal(p, C.crop_downsample(xyz, rgb, center, r, None)[2][:7])
    with pytest.raises(ValueError):
        C.crop_prompts(xyz[~member & np.isfinite(xyz).all(1)][:1], center, r)


def test_the_reciprocal_of_a_radius_never_pushes_a_member_past_one():
    """r * fl32(1 / r) <= 1 for every fp32 mantissa (scaling by a power of two is exact): with inv_r the quotient, a member (|d| <= r per axis) never
    has |d * inv_r| > 1.  The kernel clamps all the same: inv_r is the C caller's to compute (tests/test_gpu_crops.py drives that case)."""
    m = (np.arange(1 << 23, dtype=np.uint32) | np.uint32(0x3F800000)).view(f32)
    assert (m * (f32(1) / m) <= f32(1)).all()


# ------------------------------------------------------------------------------------------------ the C entry points
def test_crop_entry_points_are_declared_bound_and_exported(tmp_path):
    from point_sam_amd.build import SOURCES, build_library
    build_library()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pointsam_hip.h")).read()
    declared = set(re.findall(r"\b(psam_crop_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(CROP_ENTRY_POINTS)
    assert declared == {n for n in _lib.SIGNATURES if n.startswith("psam_crop_")}
    for n in CROP_ENTRY_POINTS:
        assert hasattr(lib, n), n
    assert ("crops.hip", ["-ffp-contract=off"]) in SOURCES
    assert "scene crops */" in hdr
    # the header is plain C and part of every translation unit (csrc/common.h): a C99 program that names the new entry points compiles
    common = open(os.path.join(ROOT, "point_sam_amd", "csrc", "common.h")).read()
    assert "pointsam_hip.h" in common
    if shutil.which("gcc") is None:
        pytest.skip("needs gcc")
    src = ['#include "pointsam_hip.h"', "int main(void) {"]
    src += [f"    void* p{i} = (void*){n};" for i, n in enumerate(CROP_ENTRY_POINTS)]
    src += ["    return " + " && ".join(f"p{i} != 0" for i in range(len(CROP_ENTRY_POINTS))) + " ? 0 : 1;", "}"]
    c = tmp_path / "crop_symbols.c"
    c.write_text("\n".join(src))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-Wno-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "crop_symbols.o")],
                   check=True)


def test_crop_entry_points_reject_bad_arguments_on_the_host():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15               # a non-null, aligned pointer; never dereferenced by the device: every call below is refused
    ctr = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    c = ctypes.addressof(ctr)

    def rejected(status, word, code=-1):
        assert status == code
        msg = lib.psam_last_error_string()
        assert word in msg, msg

    M = 1000
    need = lib.psam_crop_downsample_workspace_bytes(M)
    # the scene's table (2048 slots of an 8-byte key and a 4-byte index), one int32 per point, two int32 per 1024 points + the total
    assert need == 2048 * 12 + 4000 + 16 + 16
    assert lib.psam_crop_downsample_workspace_bytes(0) == 0 and lib.psam_crop_downsample_workspace_bytes(-3) == 0
    assert lib.psam_crop_downsample_workspace_bytes(1 << 28) > 0 and lib.psam_crop_downsample_workspace_bytes((1 << 28) + 1) == 0
    big = 1 << 30
    down = lib.psam_crop_downsample
    rejected(down(None, p, M, c, 1.0, 1.0, 4.0, p, p, p, p, p, p, big, None), b"null")
    rejected(down(p, p, M, None, 1.0, 1.0, 4.0, p, p, p, p, p, p, big, None), b"null")
    rejected(down(p, p, M, c, 1.0, 1.0, 4.0, p, p, p, p, None, p, big, None), b"null")
    rejected(down(p, p, M, c, 1.0, 1.0, 4.0, p, p, p, p, p, None, big, None), b"null")
    rejected(down(p, p, M, c, 1.0, 1.0, 4.0, p, None, p, p, p, p, big, None), b"together")
    rejected(down(p, p, M, c, 1.0, 1.0, 4.0, p, p, p, None, p, p, big, None), b"together")
    rejected(down(p, p, M, c, 1.0, 1.0, 4.0, None, None, p, None, p, p, big, None), b"together")
    rejected(down(p, None, M, c, 1.0, 1.0, 4.0, p, p, p, p, p, p, big, None), b"rgb")
    rejected(down(p, p, 0, c, 1.0, 1.0, 4.0, p, p, p, p, p, p, big, None), b"M")
    rejected(down(p, p, (1 << 28) + 1, c, 1.0, 1.0, 4.0, p, p, p, p, p, p, big, None), b"M")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        rejected(down(p, p, M, c, bad, 1.0, 4.0, p, p, p, p, p, p, big, None), b"r2")
        rejected(down(p, p, M, c, 1.0, bad, 4.0, p, p, p, p, p, p, big, None), b"inv_r")
    for bad in (-4.0, float("nan"), float("inf")):
        rejected(down(p, p, M, c, 1.0, 1.0, bad, p, p, p, p, p, p, big, None), b"inv_h")
    rejected(down(p, p, M, c, 1.0, 1.0, 0.0, p, p, p, p, p, p, need - 1, None), b"workspace")
    rejected(down(p, None, M, c, 1.0, 1.0, 4.0, None, None, None, None, p, p, need - 1, None), b"workspace")      # count only: the same workspace
    rejected(down(p, p, M, c, 1.0, 1.0, 4.0, p, p, p, p, p, p + 4, big, None), b"aligned", -2)
    bad_c = (ctypes.c_float * 3)(0.0, float("nan"), 0.0)
    rejected(down(p, p, M, ctypes.addressof(bad_c), 1.0, 1.0, 4.0, p, p, p, p, p, p, big, None), b"center")

    rows = lib.psam_crop_expand_rows
    rejected(rows(None, 8, p, 1, 8, 8, 0, p, 8, None), b"null")
    rejected(rows(p, 8, None, 1, 8, 8, 0, p, 8, None), b"null")
    rejected(rows(p, 8, p, 1, 8, 8, 0, None, 8, None), b"null")
    rejected(rows(p, 8, p, 0, 8, 8, 0, p, 8, None), b"R > 0")
    rejected(rows(p, 8, p, 1, 0, 8, 0, p, 8, None), b"Nw > 0")
    rejected(rows(p, 8, p, 1, 8, 0, 0, p, 8, None), b"M > 0")
    rejected(rows(p, 7, p, 1, 8, 8, 0, p, 8, None), b"src_ld")
    rejected(rows(p, 8, p, 1, 8, 8, 0, p, 7, None), b"dst_ld")
    rejected(rows(p + 2, 8, p, 1, 8, 8, 0, p, 8, None), b"aligned", -2)

    bits = lib.psam_crop_expand_bits
    rejected(bits(None, p, 1, 64, 64, p, p, None), b"null")
    rejected(bits(p, None, 1, 64, 64, p, p, None), b"null")
    rejected(bits(p, p, 1, 64, 64, None, None, None), b"null")
    rejected(bits(p, p, 0, 64, 64, p, None, None), b"K > 0")
    rejected(bits(p, p, 1, 0, 64, p, None, None), b"Nw > 0")
    rejected(bits(p, p, 1, 64, -1, p, None, None), b"M > 0")


def test_crop_bindings_refuse_cpu_tensors_and_bad_values():
    from point_sam_amd import ops
    z = torch.zeros(8, 3)
    with pytest.raises(_lib.PointSamHipError):
        ops.crop_downsample(z, z, (0.0, 0.0, 0.0), 0.5)
    with pytest.raises(_lib.PointSamHipError):
        ops.crop_count(z, (0.0, 0.0, 0.0), 0.5, 0.1)
    with pytest.raises(_lib.PointSamHipError):
        ops.crop_expand_rows(torch.zeros(2, 8), torch.zeros(4, dtype=torch.int64), -1.0)
    with pytest.raises(_lib.PointSamHipError):
        ops.crop_expand_bits(torch.zeros(2, 1, dtype=torch.int64), torch.zeros(4, dtype=torch.int64), 64)
    assert ops._fill_pattern(float("-inf"), torch.float32) == 0xFF800000 and ops._fill_pattern(-1, torch.int32) == 0xFFFFFFFF
    assert ops._fill_pattern(0.0, torch.float32) == 0 and ops._fill_pattern(7, torch.int32) == 7
    for bad in (1.5, True, 2 ** 31):
        with pytest.raises(ValueError):
            ops._fill_pattern(bad, torch.int32)


# ------------------------------------------------------------------------------------------------ ops stubbed by the reference
def _reference_ops(monkeypatch, log=None):
    """ops.crop_* served by tests/crop_reference.py on CPU tensors: the host logic above them runs without a GPU."""
    from point_sam_amd import ops
    log = [] if log is None else log

    def check(center, radius):
        if not np.isfinite(np.asarray(center, dtype=f32)).all() or not (np.isfinite(f32(radius)) and f32(radius) > 0):
            raise ValueError("crop_downsample: bad center or radius")

    def crop_downsample(xyz, rgb, center, radius, voxel_size=None):
        check(center, radius)
        log.append(("downsample", voxel_size))
        k, i, wx, wr, m = C.crop_downsample(xyz.numpy(), rgb.numpy(), center, radius, voxel_size)
        return torch.from_numpy(k), torch.from_numpy(i), torch.from_numpy(wx), torch.from_numpy(wr), m

    def crop_count(xyz, center, radius, voxel_size=None):
        check(center, radius)
        log.append(("count", voxel_size))
        k, _, _, _, m = C.crop_downsample(xyz.numpy(), np.zeros_like(xyz.numpy()), center, radius, voxel_size)
        return len(k), m

    def crop_expand_rows(src, inv, fill, out=None):
        lead = tuple(src.shape[:-1])
        rows = C.expand_rows(src.reshape(-1, src.shape[-1]).numpy(), inv.numpy(), np.asarray(fill, dtype=src.numpy().dtype))
        return torch.from_numpy(rows).reshape(lead + (inv.numel(),))

    def crop_expand_bits(bits, inv, Nw, area=True):
        b, a = C.expand_bits(bits.numpy().view(np.uint64), inv.numpy(), Nw)
        return torch.from_numpy(b.view(np.int64)), torch.from_numpy(a) if area else None

    for fn in (crop_downsample, crop_count, crop_expand_rows, crop_expand_bits):
        monkeypatch.setattr(ops, fn.__name__, fn)
    return log


def _scan(M=4000, seed=2):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.uniform(-1, 1, (M, 3)).astype(f32)), torch.from_numpy(rng.uniform(-1, 1, (M, 3)).astype(f32))


def test_build_crop_arguments_and_bisection(monkeypatch):
    from point_sam_amd import scene as S
    log = _reference_ops(monkeypatch)
    xyz, rgb = _scan()
    center, r = (0.1, -0.2, 0.05), 0.6
    for kw in (dict(voxel_size=0.1, max_points=5), dict(voxel_size=0.0), dict(voxel_size=-1.0), dict(voxel_size=float("nan")), dict(voxel_size=float("inf")),
               dict(voxel_size=True), dict(max_points=0), dict(max_points=2.5), dict(max_points=True)):
        with pytest.raises(ValueError):
            S.build_crop(xyz, rgb, center, r, **kw)
    for bad_center in ((0.0, 0.0), (float("nan"), 0.0, 0.0)):
        with pytest.raises(ValueError):
            S.build_crop(xyz, rgb, bad_center, r)
    for bad_radius in (0.0, -0.5, float("nan")):
        with pytest.raises(ValueError):
            S.build_crop(xyz, rgb, center, bad_radius)
    with pytest.raises(ValueError):
        S.build_crop(xyz, torch.zeros(3999, 3), center, r)
    with pytest.raises(ValueError, match="no point"):
        S.build_crop(xyz, rgb, (5.0, 0.0, 0.0), 0.1)
    assert log == [("downsample", None)]                   # everything above but the empty ball was refused before a kernel
    want = C.crop_downsample(xyz.numpy(), rgb.numpy(), center, r, None)
    members = want[4]
    # neither limit, and a max_points the ball fits into: every member, no reduction
    for kw in (dict(), dict(max_points=members), dict(max_points=members + 1)):
        crop, wxyz, wrgb = S.build_crop(xyz, rgb, center, r, **kw)
        assert crop.voxel_size is None and crop.num_working == crop.num_members == members and crop.num_points == 4000
        assert np.array_equal(crop.keep_idx.numpy(), want[0]) and np.array_equal(crop.inv.numpy(), want[1]) and np.array_equal(wxyz.numpy(), want[2])
        assert crop.center == tuple(float(f32(v)) for v in center) and crop.radius == float(f32(r)) and not crop.identity
    # one point too many: the ladder is searched by the same bisection as the scene's, counting the ball's voxels
    del log[:]
    crop, wxyz, _ = S.build_crop(xyz, rgb, center, r, max_points=members - 1)
    asked = [h for what, h in log if what == "count"]
    assert asked[0] is None and asked[1] == S.ladder(0) and 8 <= len(asked) <= 9 and log[-1] == ("downsample", crop.voxel_size)
    k = round(4 * (1 - np.log2(crop.voxel_size)))
    assert S.ladder(k) == crop.voxel_size and crop.num_working <= members - 1
    assert len(C.crop_downsample(xyz.numpy(), rgb.numpy(), center, r, S.ladder(k + 1))[0]) > members - 1
    assert crop.num_working == len(C.crop_downsample(xyz.numpy(), rgb.numpy(), center, r, crop.voxel_size)[0]) == wxyz.shape[0]
    crop, _, _ = S.build_crop(xyz, rgb, center, r, max_points=1)      # the coarsest size holds the whole ball in one cell: its first member
    assert crop.voxel_size == 2.0 and crop.keep_idx.tolist() == [int(want[0][0])] and set(crop.inv.tolist()) == {-1, 0}
    crop, _, _ = S.build_crop(xyz, rgb, center, r, voxel_size=0.25)
    assert crop.voxel_size == 0.25 and crop.num_working == len(C.crop_downsample(xyz.numpy(), rgb.numpy(), center, r, 0.25)[0])


def test_crop_prompts_and_prompt_mask():
    from point_sam_amd import scene as S
    xyz, rgb = _scan()
    center, r = (0.1, -0.2, 0.05), 0.6
    keep, inv, wxyz, _, members = C.crop_downsample(xyz.numpy(), rgb.numpy(), center, r, 0.2)
    crop = S.Crop(tuple(float(f32(v)) for v in center), float(f32(r)), 4000, members, len(keep), torch.from_numpy(keep), torch.from_numpy(inv), 0.2)
    pts = xyz[torch.from_numpy(keep[:10])].reshape(2, 5, 3)
    got = S.crop_prompts(crop, pts)
    assert tuple(got.shape) == (2, 5, 3) and np.array_equal(got.numpy().reshape(-1, 3), wxyz[:10])      # the kernel's arithmetic, bit for bit
    assert np.array_equal(got.numpy(), C.crop_prompts(pts.numpy(), center, r))
    off = xyz[torch.from_numpy(np.nonzero(inv < 0)[0][:1])]
    with pytest.raises(ValueError, match="outside the crop"):
        S.crop_prompts(crop, torch.cat([pts[0], off])[None])
    with pytest.raises(ValueError, match="outside the crop"):
        S.crop_prompts(crop, torch.full((1, 1, 3), float("nan")))
    mask = torch.arange(4000.0)[None]
    assert torch.equal(S.reduce_prompt_mask(crop, mask), torch.from_numpy(keep).float()[None])
    narrow = torch.zeros(1, len(keep))
    assert S.reduce_prompt_mask(crop, narrow) is narrow and S.reduce_prompt_mask(crop, None) is None
    with pytest.raises(ValueError, match="width"):
        S.reduce_prompt_mask(crop, torch.zeros(1, 3999))


# ------------------------------------------------------------------------------------------------ CropLayerConfig
def test_crop_layer_config_validation():
    from point_sam_amd.proposals import CropLayerConfig
    ok = CropLayerConfig(num_crops=4, radius=0.25).validate()
    assert (ok.max_points, ok.edge_frac, ok.nms_thresh) == (32768, 0.05, 0.7)
    assert CropLayerConfig.from_overrides({"num_crops": 2, "radius": 0.5, "edge_frac": 0.0}).edge_frac == 0.0
    for kw in (dict(num_crops=0), dict(num_crops=2.0), dict(num_crops=True), dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")),
               dict(radius=float("inf")), dict(radius="1"), dict(max_points=0), dict(max_points=1.5), dict(edge_frac=-0.1), dict(edge_frac=1.0),
               dict(edge_frac=float("nan")), dict(nms_thresh=1.5), dict(nms_thresh=-0.1)):
        with pytest.raises(ValueError):
            CropLayerConfig(**{"num_crops": 2, "radius": 0.5, **kw}).validate()
    with pytest.raises(ValueError, match="unknown"):
        CropLayerConfig.from_overrides({"num_crops": 2, "radius": 0.5, "crop_layers": 1})
    with pytest.raises(ValueError, match="needs"):
        CropLayerConfig.from_overrides({"num_crops": 2})


# ------------------------------------------------------------------------------------------------ the merge, kernels stubbed
def _stub_mask_ops(monkeypatch):
    """mask_intersections / mask_nms / mask_paint in plain numpy, from their definitions in ops.py."""
    from point_sam_amd import ops
    calls = {}

    def mask_intersections(a, b=None):
        b = a if b is None else b
        ua, ub = R.unwords(a.numpy().view(np.uint64), a.shape[1] * 64), R.unwords(b.numpy().view(np.uint64), b.shape[1] * 64)
        return torch.from_numpy((ua[:, None, :] & ub[None, :, :]).sum(-1).astype(np.int32))

    def mask_nms(order, valid, area, inter, iou_thr):
        calls["nms"] = (order.clone(), valid.clone(), float(iou_thr))
        keep = np.zeros(order.numel(), dtype=np.uint8)
        for i in order.tolist():
            if valid[i] and not any(keep[j] and int(inter[i, j]) > iou_thr * (int(area[i]) + int(area[j]) - int(inter[i, j])) for j in range(len(keep))):
                keep[i] = 1
        return torch.from_numpy(keep)

    def mask_paint(bits, order, keep, N):
        masks = R.unwords(bits.numpy().view(np.uint64), N)
        labels = np.full(N, -1, dtype=np.int32)
        rank = 0
        for i in order.tolist():
            if keep[i]:
                labels[(labels == -1) & masks[i]] = rank
                rank += 1
        return torch.from_numpy(labels)

    for fn in (mask_intersections, mask_nms, mask_paint):
        monkeypatch.setattr(ops, fn.__name__, fn)
    return calls


def _layer(masks, scores, first_candidate):
    from point_sam_amd.proposals import Proposals
    masks = np.asarray(masks, dtype=bool)
    k, N = masks.shape
    cand = torch.arange(first_candidate, first_candidate + k, dtype=torch.int64)
    return Proposals(N, torch.from_numpy(R.words(masks).view(np.int64)), cand, cand // 3, torch.tensor(scores, dtype=torch.float32),
                     torch.from_numpy(masks.sum(1).astype(np.int32)), torch.ones(k), torch.full((N,), -1, dtype=torch.int32))


def test_merge_order_and_crop_index(monkeypatch):
    from point_sam_amd import proposals as P
    calls = _stub_mask_ops(monkeypatch)
    N = 130
    m = np.zeros((6, N), dtype=bool)
    m[0, 0:40] = True            # base, 0.9
    m[1, 60:100] = True          # base, 0.5
    m[2, 0:38] = True            # crop 0, 0.95: overlaps base row 0 (IoU 0.95) and beats it
    m[3, 100:130] = True         # crop 0, 0.5: ties with base row 1 -> the base layer comes first
    m[4, 60:99] = True           # crop 1, 0.4: suppressed by base row 1
    m[5, 45:55] = True           # crop 1, 0.5: ties again, third
    base, c0, c1 = _layer(m[0:2], [0.9, 0.5], 10), _layer(m[2:4], [0.95, 0.5], 20), _layer(m[4:6], [0.4, 0.5], 30)
    out = P.merge_proposals([(-1, base), (0, c0), (1, c1)], N, 0.7)
    order, valid, thr = calls["nms"]
    assert order.tolist() == [2, 0, 1, 3, 5, 4] and order.dtype == torch.int32      # by score, stable: equal scores in the order base, crop 0, crop 1
    assert valid.tolist() == [1] * 6 and valid.dtype == torch.uint8 and thr == 0.7
    assert out.crop_index.tolist() == [0, -1, 0, 1] and out.crop_index.dtype == torch.int64
    assert out.candidate.tolist() == [20, 11, 21, 31] and out.prompt_index.tolist() == [6, 3, 7, 10]      # per-origin numbering
    assert out.score.tolist() == [0.949999988079071, 0.5, 0.5, 0.5] and out.area.tolist() == [38, 40, 30, 10]
    assert np.array_equal(R.unwords(out.bits.numpy().view(np.uint64), N), m[[2, 1, 3, 5]])
    lab = out.labels.numpy()
    assert out.n_points == N and (lab[0:38] == 0).all() and (lab[38:45] == -1).all() and (lab[60:100] == 1).all() and (lab[100:130] == 2).all() and (lab[45:55] == 3).all()
    assert out.changed is None
    # a single layer passes through the same steps; no row at all gives an empty result
    solo = P.merge_proposals([(-1, base)], N, 0.7)
    assert solo.crop_index.tolist() == [-1, -1] and solo.candidate.tolist() == [10, 11]
    empty = _layer(np.zeros((0, N), dtype=bool), [], 0)
    none = P.merge_proposals([(-1, empty), (0, empty)], N, 0.7)
    assert len(none) == 0 and none.crop_index.numel() == 0 and (none.labels == -1).all() and none.labels.numel() == N
    with pytest.raises(ValueError, match="layer"):
        P.merge_proposals([(-1, base), (0, _layer(np.zeros((1, 64), dtype=bool), [0.1], 0))], N, 0.7)
    monkeypatch.setattr(P, "MAX_CANDIDATES", 5)
    with pytest.raises(ValueError, match="exceed"):
        P.merge_proposals([(-1, base), (0, c0), (1, c1)], N, 0.7)


# ------------------------------------------------------------------------------------------------ the predictor's state machine
class StubModel:
    """encode: remembers the cloud; decode: logit = 1 - 2 |x - first prompt| per point, three shifted candidates."""

    def __init__(self):
        g = types.SimpleNamespace(num_groups=4, group_size=4)
        self.pc_encoder = types.SimpleNamespace(patch_embed=types.SimpleNamespace(grouper=g))
        self.encoded = []

    def encode(self, xyz, rgb):
        self.encoded.append(tuple(xyz.shape))
        return types.SimpleNamespace(coords=xyz)

    def decode(self, state, points, labels, prompt_mask, multimask):
        self.last = (state, points.clone(), None if prompt_mask is None else prompt_mask.clone())
        logit = 1 - 2 * (state.coords[0] - points[0, 0]).norm(dim=-1)
        if prompt_mask is not None:
            logit = logit + 0.125 * prompt_mask[0]
        Cn = 3 if multimask else 1
        return torch.stack([logit + 0.25 * i for i in range(Cn)])[None].contiguous(), torch.tensor([[0.1, 0.9, 0.5][:Cn]])

    def check_coordinate_range(self):
        pass


def test_predictor_crop_state_machine(monkeypatch):
    from point_sam_amd.predictor import PointSAMPredictor
    _reference_ops(monkeypatch)
    xyz, rgb = _scan(600, seed=4)
    center, r = (0.1, -0.2, 0.05), 0.7
    keep, inv, wxyz, wrgb, members = C.crop_downsample(xyz.numpy(), rgb.numpy(), center, r, 0.25)
    model = StubModel()
    pred = PointSAMPredictor(model)
    with pytest.raises(RuntimeError, match="set_scene"):
        pred.set_crop(center, r)
    pred.set_pointcloud(xyz[None], rgb[None])
    with pytest.raises(RuntimeError, match="set_scene"):      # a plain cloud is no scene
        pred.set_crop(center, r)
    pred.set_scene(xyz, rgb, max_points=600)
    assert model.encoded == [(1, 600, 3), (1, 600, 3)] and pred.crop is None
    scene_state = pred._state
    click = xyz[int(keep[3])][None, None]
    one = torch.ones(1, 1, dtype=torch.int64)
    before, _, _ = pred.predict_masks(click, one, None, True)
    # the crop: its own encoder pass on the reference's cloud; the scene's state stays
    pred.set_crop(center, r, voxel_size=0.25)
    assert model.encoded[2:] == [(1, len(keep), 3)] and pred._state is scene_state
    assert np.array_equal(pred._crop_state.coords[0].numpy(), wxyz)
    assert (pred.crop.num_points, pred.crop.num_members, pred.crop.num_working) == (600, members, len(keep))
    pred.set_crop(center, r, voxel_size=0.25)               # the cache hits
    assert len(model.encoded) == 3
    logits, scores, _ = pred.predict_masks(click, one, None, True)
    state, pts, pm = model.last
    assert state is pred._crop_state and pm is None
    assert np.array_equal(pts.numpy(), C.crop_prompts(click.numpy(), center, r))      # the model saw crop coordinates
    assert tuple(logits.shape) == (1, 3, 600)
    want = 1 - 2 * (torch.from_numpy(wxyz) - pts[0, 0]).norm(dim=-1)
    assert np.array_equal(logits[0, 0].numpy(), C.expand_rows(want[None].numpy(), inv, f32(-np.inf))[0])
    assert torch.isneginf(logits[0][:, torch.from_numpy(inv < 0)]).all()
    # a scan-width prompt mask is reduced to the crop's representatives: the -inf off the ball never reaches the model
    pred.predict_masks(click, one, logits[0][1][None], False)
    assert torch.equal(model.last[2], (want + 0.25)[None]) and torch.isfinite(model.last[2]).all()
    with pytest.raises(ValueError, match="outside the crop"):
        pred.predict_masks(xyz[int(np.nonzero(inv < 0)[0][0])][None, None], one, None, True)
    # another crop replaces it; clear_crop returns to the scene without encoding
    pred.set_crop(center, r, voxel_size=0.5)
    assert len(model.encoded) == 4 and pred.crop.voxel_size == 0.5
    pred.clear_crop()
    assert pred.crop is None and len(model.encoded) == 4
    after, _, _ = pred.predict_masks(click, one, None, True)
    assert model.last[0] is scene_state and torch.equal(after, before)
    pred.set_crop(center, r, voxel_size=0.5)                # the last crop is still cached
    assert len(model.encoded) == 4 and pred.crop is not None
    # set_scene drops the crop, also for the same scene; set_pointcloud too
    pred.set_scene(xyz, rgb, max_points=600)
    assert pred.crop is None and len(model.encoded) == 4 and pred._state is scene_state
    pred.set_crop(center, r, voxel_size=0.5)
    assert len(model.encoded) == 4
    pred.set_pointcloud(xyz[None], rgb[None])
    assert pred.crop is None and pred.scene is None and len(model.encoded) == 5
    with pytest.raises(RuntimeError, match="set_scene"):
        pred.set_crop(center, r, voxel_size=0.5)
    # another scene forgets the cached crop
    xyz2, rgb2 = _scan(600, seed=5)
    pred.set_scene(xyz2, rgb2, max_points=600)
    pred.set_crop(center, r, voxel_size=0.5)
    assert len(model.encoded) == 7
    with pytest.raises(ValueError, match="no point"):
        pred.set_crop((9.0, 0.0, 0.0), 0.1)
    assert pred.crop is not None and pred.crop.voxel_size == 0.5      # a refused crop leaves the active one
    with pytest.raises(RuntimeError, match="clear_crop"):
        from point_sam_amd.proposals import CropLayerConfig
        pred.generate_masks(None, crops=CropLayerConfig(num_crops=1, radius=0.5))
    with pytest.raises(TypeError):
        pred.generate_masks(None, crops={"num_crops": 1})


# ------------------------------------------------------------------------------------------------ the demo's routes
class FakePredictor:
    def __init__(self):
        self.calls = []
        self.crop = None

    def set_pointcloud(self, xyz, rgb):
        self.calls.append(("set_pointcloud", tuple(xyz.shape)))
        self.n, self.crop = xyz.shape[1], None

    def set_scene(self, xyz, rgb, voxel_size=None, max_points=None):
        self.calls.append(("set_scene", tuple(xyz.shape), voxel_size, max_points))
        self.n, self.xyz, self.crop = xyz.shape[1], xyz[0], None

    def set_crop(self, center, radius, voxel_size=None, max_points=None):
        self.calls.append(("set_crop", tuple(center), radius, voxel_size, max_points))
        inside = (self.xyz - torch.tensor(center, dtype=self.xyz.dtype)).norm(dim=-1) <= radius
        if not inside.any():
            raise ValueError("build_crop: no point of the scan lies in the ball")
        self.crop = types.SimpleNamespace(num_members=int(inside.sum()), num_working=min(int(inside.sum()), max_points or 10 ** 9), inside=inside)

    def clear_crop(self):
        self.calls.append(("clear_crop",))
        self.crop = None

    def predict_masks(self, pts, lab, prompt_mask, multimask):
        assert prompt_mask is None or tuple(prompt_mask.shape) == (1, self.n)
        logits = torch.linspace(-1, 1, self.n).repeat(1, 3 if multimask else 1, 1)
        if self.crop is not None:
            logits = torch.where(self.crop.inside, logits, torch.tensor(float("-inf")))
        return logits, torch.tensor([[0.1, 0.9, 0.5][:logits.shape[1]]]), logits

    def generate_masks(self, cfg):
        from point_sam_amd.proposals import Proposals
        labels = torch.zeros(self.n, dtype=torch.int32)
        if self.crop is not None:
            labels[~self.crop.inside] = -1
        e = torch.zeros(1)
        return [Proposals(self.n, torch.zeros(1, (self.n + 63) // 64, dtype=torch.int64), e.long(), e.long(), torch.tensor([0.5]), e.int(), e, labels)]


@pytest.mark.parametrize("working_points", [None, 16])
def test_demo_crop_routes(tmp_path, working_points):
    from point_sam_amd.demo_server import DemoSession, serve
    pred = FakePredictor()
    kw = {} if working_points is None else {"working_points": working_points}
    sess = DemoSession(pred, models_dir=str(tmp_path), output_dir=str(tmp_path / "results"), device="cpu", crop_points=8, **kw)
    srv = serve(sess, "127.0.0.1", 0)
    threading.Thread(target=srv.serve_forever, daemon=True).start()

    def req(path, body=None):
        c = http.client.HTTPConnection("127.0.0.1", srv.server_address[1], timeout=10)
        c.request("POST", path, None if body is None else json.dumps(body), {"Content-Type": "application/json"})
        r = c.getresponse()
        return r.status, json.loads(r.read())

    try:
        assert req("/crop", {"center": [0.5, 0.5, 0.5], "radius": 0.4})[0] == 400          # no cloud yet
        pts = np.random.RandomState(1).rand(40, 3)
        cloud = {"points": {str(i): float(v) for i, v in enumerate(pts.flatten())}, "colors": {str(i): 0.5 for i in range(120)}}
        assert req("/sampled_pointcloud", cloud)[0] == 200
        plain = ("set_pointcloud", (1, 40, 3)) if working_points is None else ("set_scene", (1, 40, 3), None, 16)
        st, out = req("/segment", {"prompt_point": [0.5, 0.5, 0.5], "prompt_label": 1})
        assert st == 200 and len(out["seg"]) == 40 and pred.calls == [plain]              # without a crop the routes do what they did
        # the crop: a scene (the loaded cloud itself without --working-points), then the ball with --crop-points
        st, out = req("/crop", {"center": [0.5, 0.5, 0.5], "radius": 0.4})
        inside = np.linalg.norm(pts - 0.5, axis=1) <= 0.4
        assert st == 200 and out == {"status": "cropped", "members": int(inside.sum()), "working_points": min(int(inside.sum()), 8)}, out
        scene = ("set_scene", (1, 40, 3), None, working_points or 40)
        crop = ("set_crop", (0.5, 0.5, 0.5), 0.4, None, 8)
        assert pred.calls[1:] == [scene, crop] and sess.prompts == [] and sess.prompt_mask is None
        for click in range(2):
            st, out = req("/segment", {"prompt_point": [0.5, 0.5, 0.5], "prompt_label": 1})
            assert st == 200 and len(out["seg"]) == 40 and not np.array(out["seg"])[~inside].any()
        assert pred.calls[3:] == [scene, crop, scene, crop]
        st, out = req("/segment_all", {})
        assert st == 200 and (np.array(out["labels"])[~inside] == -1).all() and (np.array(out["labels"])[inside] == 0).all()
        # bad requests leave the crop as it is
        for bad in ({"center": [0.5, 0.5], "radius": 0.4}, {"center": [0.5, 0.5, 0.5], "radius": 0}, {"center": [0.5, 0.5, 0.5], "radius": "1"},
                    {"center": [0.5, 0.5, None], "radius": 0.4}, {"center": [0.5, 0.5, 0.5]}, {"center": [0.5, 0.5, 0.5], "radius": 0.4, "voxel": 1},
                    {"center": [9.0, 9.0, 9.0], "radius": 0.1}):
            st, out = req("/crop", bad)
            assert st == 400 and "error" in out, bad
        assert sess.crop == ((0.5, 0.5, 0.5), 0.4)
        n = len(pred.calls)
        assert req("/crop/clear") == (200, {"status": "cleared"}) and sess.crop is None and pred.calls[n:] == [("clear_crop",)]
        st, out = req("/segment", {"prompt_point": [0.5, 0.5, 0.5], "prompt_label": 1})
        assert st == 200 and pred.calls[-1] == plain
        # loading another cloud drops the crop
        assert req("/crop", {"center": [0.5, 0.5, 0.5], "radius": 0.4})[0] == 200 and sess.crop is not None
        assert req("/sampled_pointcloud", cloud)[0] == 200 and sess.crop is None
    finally:
        srv.shutdown()


def test_demo_main_has_the_crop_points_option():
    src = open(os.path.join(ROOT, "point_sam_amd", "demo_server.py")).read()
    assert '"--crop-points"' in src and "crop_points=args.crop_points" in src
