"""The global pose search on the host (point_sam_amd/align.py: SearchConfig, rotation_grid, candidate_poses, search; ops.align_score's argument checks;
the C entry's refusals; predictor.align(search=); the /propagate route) against tests/align_search_reference.py.  No GPU: where the search itself runs,
the reference scores and steps through `score=` / `step=`."""
import ctypes
import dataclasses
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import align_reference as A
import align_search_reference as S
from point_sam_amd import _lib
from point_sam_amd import align as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


# ------------------------------------------------------------------------------------------------ the grid
def _rotations(Rs, n):
    assert Rs.shape == (n, 3, 3) and Rs.dtype == np.float64
    assert np.abs(Rs @ Rs.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-12 and np.abs(np.linalg.det(Rs) - 1).max() <= 1e-12


def test_yaw_grid():
    Rs = X.rotation_grid(X.SearchConfig(rotations="yaw", yaw_steps=72))
    _rotations(Rs, 72)
    assert np.array_equal(Rs[0], np.eye(3))                                            # yaw 0 is the identity, exactly
    assert np.abs(Rs - S.yaw_grid(72)).max() <= 1e-12
    assert np.abs(Rs[18] - np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])).max() <= 1e-12      # a quarter turn about +z, counter-clockwise
    up = (1.0, -2.0, 0.5)
    Rs = X.rotation_grid(X.SearchConfig(yaw_steps=7, up=up))
    _rotations(Rs, 7)
    assert np.abs(Rs - S.yaw_grid(7, up)).max() <= 1e-12 and np.abs(Rs @ (np.array(up) / np.linalg.norm(up)) - np.array(up) / np.linalg.norm(up)).max() <= 1e-12
    assert np.abs(np.linalg.matrix_power(Rs[1], 7) - np.eye(3)).max() <= 1e-12 and np.array_equal(Rs[0], np.eye(3))
    assert X.rotation_grid(X.SearchConfig(yaw_steps=1)).shape == (1, 3, 3)


def test_so3_grid():
    cfg = X.SearchConfig(rotations="so3", axes=96, rolls=24)
    Rs = X.rotation_grid(cfg)
    _rotations(Rs, 96 * 24)
    assert cfg.num_rotations == 96 * 24 and np.abs(Rs - S.so3_grid(96, 24)).max() <= 1e-12
    d = S.fibonacci(96)
    assert np.abs(d[:, 2] - (1 - (2 * np.arange(96) + 1) / 96)).max() <= 1e-15 and np.abs(np.linalg.norm(d, axis=1) - 1).max() <= 1e-15
    for k, j in ((0, 0), (0, 5), (47, 23), (95, 1)):
        Rm = Rs[k * 24 + j]                                                            # index = k * rolls + j
        assert np.abs(Rm @ [0, 0, 1.0] - d[k]).max() <= 1e-12                           # whatever the roll, +z goes to d_k
        assert np.abs(Rs[k * 24].T @ Rm - S.turn([0, 0, 1.0], 2 * math.pi * j / 24)).max() <= 1e-12      # and the roll is about +z, applied first
    # the tilt is the SHORTEST arc: its axis lies in the xy plane
    tilt = Rs[40 * 24]
    axis = np.array([tilt[2, 1] - tilt[1, 2], tilt[0, 2] - tilt[2, 0], tilt[1, 0] - tilt[0, 1]])
    assert abs(axis[2]) <= 1e-12 * np.linalg.norm(axis)
    small = X.rotation_grid(X.SearchConfig(rotations="so3", axes=1, rolls=3))           # one direction: z_0 = 0, the equator
    _rotations(small, 3)
    assert np.abs(small[0] @ [0, 0, 1.0] - [1.0, 0, 0]).max() <= 1e-12


def test_rotation_to_and_the_branch_at_minus_z():
    assert np.array_equal(X.rotation_to([0, 0, -1.0]), np.diag([1.0, -1.0, -1.0]))      # the half turn about x
    assert np.array_equal(X.rotation_to([0, 0, -3.5]), np.diag([1.0, -1.0, -1.0]))      # the direction is normalised first
    assert np.array_equal(X.rotation_to([0, 0, 2.0]), np.eye(3))
    g = np.random.default_rng(5)
    for d in list(g.normal(size=(20, 3))) + [np.array([1e-3, 0, -1.0]), np.array([0, -1e-5, -1.0])]:
        Rm = X.rotation_to(d)
        _rotations(Rm[None], 1)
        assert np.abs(Rm @ [0, 0, 1.0] - d / np.linalg.norm(d)).max() <= 1e-12 and np.abs(Rm - S.from_z(d)).max() <= 1e-9


def test_explicit_rotations_pass_through():
    Rs = np.stack([A.rotation([1, 2, 3], 10.0 * k) for k in range(5)])
    cfg = X.SearchConfig(rotations=Rs.tolist())
    assert cfg.num_rotations == 5 and np.array_equal(X.rotation_grid(cfg), Rs)
    with pytest.raises(TypeError):
        X.rotation_grid({"rotations": "yaw"})


# ------------------------------------------------------------------------------------------------ the candidates
def test_candidate_order_and_the_offset_lattice():
    anchors = np.array([[0.5, 0.25, -0.125], [-1.0, 0.0, 2.0]])
    cfg = X.SearchConfig(yaw_steps=5, offsets=1, offset_step=0.25, anchors=anchors)
    sc, qc = np.array([9.0, 9.0, 9.0]), np.array([0.3, -0.7, 0.2])                       # with anchors the source centroid is not used
    poses = X.candidate_poses(cfg, sc, qc)
    Rs = X.rotation_grid(cfg)
    assert poses.shape == (5 * 2 * 27, 3, 4) and poses.dtype == np.float64
    assert np.abs(poses - S.candidates(S.yaw_grid(5), anchors, qc, 1, 0.25)).max() <= 1e-12
    for r, a, (i, j, k) in ((0, 0, (-1, -1, -1)), (3, 1, (1, 0, -1)), (4, 1, (1, 1, 1)), (2, 0, (0, -1, 1))):
        p = poses[(r * 2 + a) * 27 + ((k + 1) * 3 + (j + 1)) * 3 + (i + 1)]            # x runs fastest
        assert np.array_equal(p[:, :3], Rs[r])
        assert np.abs(p[:, :3] @ qc + p[:, 3] - (anchors[a] + 0.25 * np.array([i, j, k]))).max() <= 1e-12      # the query centroid lands at c + o
    # offsets = 0 and no anchors: one pose per rotation, the centroid match
    plain = X.candidate_poses(X.SearchConfig(yaw_steps=4), sc, qc)
    assert plain.shape == (4, 3, 4) and np.abs(plain[:, :, :3] @ qc + plain[:, :, 3] - sc).max() <= 1e-12
    with pytest.raises(ValueError, match="finite"):
        X.candidate_poses(cfg, sc, [0.0, np.nan, 0.0])


# ------------------------------------------------------------------------------------------------ the configuration
def test_search_config_validation_and_from_overrides():
    cfg = X.SearchConfig()
    assert (cfg.rotations, cfg.sample, cfg.keep, cfg.offsets, cfg.radius, cfg.anchors) == ("yaw", 1024, 8, 0, None, None)
    with pytest.raises(dataclasses.FrozenInstanceError):
        cfg.keep = 3
    assert "NONE of the defaults has been tuned on real data" in X.SearchConfig.__doc__
    for bad in (dict(rotations="roll"), dict(rotations=np.eye(3)), dict(rotations=[np.eye(3) * 2]), dict(rotations=[np.diag([1.0, 1, -1])]),
                dict(rotations=np.full((2, 3, 3), np.nan)), dict(rotations=np.zeros((0, 3, 3))), dict(yaw_steps=0), dict(yaw_steps=2.0), dict(yaw_steps=True),
                dict(up=(0, 0, 0)), dict(up=(0, 1)), dict(up="z"), dict(up=(0, float("nan"), 1)), dict(axes=0), dict(rolls=-1), dict(offsets=-1),
                dict(offsets=1.5), dict(offsets=17), dict(offset_step=0), dict(offset_step=float("inf")), dict(offset_step="a"),
                dict(anchors=[[0, 0]]), dict(anchors=[0, 0, 0]), dict(anchors=[[0, 0, float("inf")]]), dict(anchors=[]), dict(sample=0), dict(sample=1.5),
                dict(radius=0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius="r"), dict(keep=0), dict(keep=1025),
                dict(rotations="so3", axes=1 << 10, rolls=1 << 10, offsets=1), dict(yaw_steps=1 << 20, anchors=[[0, 0, 0], [1, 1, 1]])):
        with pytest.raises(ValueError):
            X.SearchConfig(**bad)
    got = X.SearchConfig.from_overrides({"rotations": "so3", "axes": 12, "rolls": 4, "offsets": 1, "offset_step": 0.05, "anchors": [[0, 0, 0], [1, 2, 3]],
                                         "sample": 256, "radius": 0.05, "keep": 3, "up": [0, 1, 0]})
    assert (got.rotations, got.axes, got.rolls, got.offsets, got.offset_step, got.sample, got.radius, got.keep, got.up) == \
        ("so3", 12, 4, 1, 0.05, 256, 0.05, 3, (0.0, 1.0, 0.0))
    assert np.array_equal(got.anchors, [[0.0, 0, 0], [1, 2, 3]]) and got.num_rotations == 48
    assert X.SearchConfig.from_overrides({}).yaw_steps == 72
    for bad in ({"speed": 3}, {"keep": 0}, [], None, "yaw"):
        with pytest.raises(ValueError):
            X.SearchConfig.from_overrides(bad)


# ------------------------------------------------------------------------------------------------ the sampling rule
def _pack(take):
    pad = np.zeros(-(-len(take) // 64) * 64, dtype=bool)
    pad[:len(take)] = take
    return (pad.reshape(-1, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(1, dtype=np.uint64).view(np.int64)


class _Stop(Exception):
    pass


def _scored(xyz, cfg, bits=None, src=None):
    """The sample `search` hands to the score, and the poses: the stand-in records them and ends the search."""
    seen = {}

    def score(index, sample, poses, radius):
        seen.update(sample=np.array(sample), poses=np.array(poses), radius=radius)
        raise _Stop
    index = types.SimpleNamespace(src_xyz=np.zeros((4, 3), dtype=f32) if src is None else src)
    with pytest.raises(_Stop):
        X.search(index, xyz, cfg, X.AlignConfig(0.1), bits=bits, score=score)
    return seen


@pytest.mark.parametrize("n", [5, 63, 64, 65, 1000])
def test_sampling_rule(n):
    assert np.array_equal(X.sample_positions(n, 64), S.sample_positions(n, 64))
    g = np.random.default_rng(n)
    xyz = g.uniform(-1, 1, size=(n, 3)).astype(f32)
    src = g.uniform(-1, 1, size=(50, 3)).astype(f32)
    seen = _scored(xyz, X.SearchConfig(sample=64, yaw_steps=3), src=src)
    want = xyz[S.sample_positions(n, 64)]
    assert np.array_equal(seen["sample"], want) and len(want) == min(n, 64) and seen["radius"] == 0.1
    if n > 64:
        assert np.array_equal(seen["sample"][:3], xyz[[0, n // 64, 2 * n // 64]])
    # the centroids are the sources' and the SCORED queries', in fp64
    assert np.abs(seen["poses"] - S.candidates(S.yaw_grid(3), src.astype(np.float64).mean(0), want.astype(np.float64).mean(0))).max() <= 1e-12


def test_sampling_under_bits():
    g = np.random.default_rng(2)
    xyz = g.uniform(-1, 1, size=(1000, 3)).astype(f32)
    take = g.uniform(size=1000) < 0.3
    part = np.nonzero(take)[0]
    for sample in (64, len(part), 512):
        seen = _scored(xyz, X.SearchConfig(sample=sample), bits=_pack(take))
        assert np.array_equal(seen["sample"], xyz[part[S.sample_positions(len(part), sample)]])
    seen = _scored(torch.from_numpy(xyz), X.SearchConfig(sample=64), bits=torch.from_numpy(_pack(take)))     # tensors, as the predictor passes them
    assert np.array_equal(seen["sample"], xyz[part[S.sample_positions(len(part), 64)]])
    with pytest.raises(ValueError, match="no query"):
        X.search(types.SimpleNamespace(src_xyz=xyz), xyz, X.SearchConfig(), X.AlignConfig(0.1), bits=_pack(np.zeros(1000, dtype=bool)), score=lambda *a: 0)


# ------------------------------------------------------------------------------------------------ the ordering and the choice
def _sums(x, s):
    n = len(x)
    return A.sums_from(s.astype(f32), x.astype(f32), np.arange(n, dtype=np.int32), np.zeros(n, dtype=f32), np.ones(n, dtype=bool))[0]


def _hand_made(counts, outcome, keep):
    """27 poses (the identity x the 27 offsets); score answers `counts`; the step answers, for the candidate whose offset it recognises in the pose, the
    sums of outcome[candidate] = (pairs, noise): `pairs` exact pairs displaced by noise * a fixed pattern, so that more noise is a higher rms."""
    g = np.random.default_rng(1)
    xyz = g.uniform(-1, 1, size=(40, 3)).astype(f32)
    pattern = g.normal(size=(40, 3))
    cfg = X.SearchConfig(rotations=[np.eye(3)], offsets=1, offset_step=0.5, keep=keep)
    index = types.SimpleNamespace(src_xyz=xyz)
    poses = X.candidate_poses(cfg, xyz.astype(np.float64).mean(0), xyz.astype(np.float64).mean(0))
    calls = []

    def step(index_, xyz_, pose, radius, bits):
        p = int(np.argmin(np.abs(poses - np.asarray(pose)[None]).sum((1, 2))))
        calls.append(p)
        pairs, noise = outcome.get(p, (0, 0.0))
        x = xyz[:pairs].astype(np.float64)
        out = _sums(x, x + noise * pattern[:pairs]) if pairs else np.zeros(20)
        out[19] = 40
        return out
    got = X.search(index, xyz, cfg, X.AlignConfig(0.1, iterations=1, min_pairs=3), score=lambda i, x, p, r: np.asarray(counts), step=step)
    return got, calls


def test_ordering_by_count_then_index_and_the_choice_by_pairs_rms_then_order():
    counts = np.zeros(27, dtype=np.int32)
    counts[[20, 4, 11, 7, 25]] = [9, 9, 12, 9, 3]
    # the order: 11 (12), then 4, 7, 20 (9 each, by index), then 25; keep = 4 stops before it
    got, calls = _hand_made(counts, {11: (20, 1e-3), 4: (30, 2e-3), 7: (30, 1e-3), 20: (30, 1e-3)}, keep=4)
    rec = got.search
    assert calls == [11, 4, 7, 20] == [c["pose_index"] for c in rec.candidates] and [c["count"] for c in rec.candidates] == [12, 9, 9, 9]
    assert (rec.poses, rec.sample, rec.chosen) == (27, 40, 2)          # most pairs: 4, 7, 20; the lower rms: 7, 20; the earlier: 7
    assert got.pairs == 30 and rec.candidates[1]["rms"] > rec.candidates[2]["rms"] == rec.candidates[3]["rms"] == got.rms > 0
    assert [c["pairs"] for c in rec.candidates] == [20, 30, 30, 30] and got.iterations == 1
    # pairs beat rms
    got, _ = _hand_made(counts, {11: (20, 1e-4), 4: (21, 5e-2)}, keep=2)
    assert got.search.chosen == 1 and got.pairs == 21
    # keep beyond the poses: all 27 are refined, in order
    got, calls = _hand_made(counts, {25: (10, 1e-3)}, keep=40)
    assert calls[:5] == [11, 4, 7, 20, 25] and calls[5:] == [p for p in range(27) if p not in (11, 4, 7, 20, 25)] and got.search.chosen == 4
    # nobody has a pair: the first candidate's Alignment, not converged
    got, calls = _hand_made(counts, {}, keep=3)
    assert got.search.chosen == 0 and got.pairs == 0 and not got.converged and "min_pairs" in got.reason and calls == [11, 4, 7]
    assert X.icp("i", np.zeros((4, 3), dtype=f32), X.AlignConfig(0.1), step=lambda *a: np.zeros(20)).search is None


def test_search_refuses_bad_arguments():
    xyz = np.zeros((10, 3), dtype=f32)
    index = types.SimpleNamespace(src_xyz=xyz)
    with pytest.raises(TypeError, match="SearchConfig"):
        X.search(index, xyz, {"keep": 1}, X.AlignConfig(0.1))
    with pytest.raises(TypeError, match="AlignConfig"):
        X.search(index, xyz, X.SearchConfig(), 0.1)
    with pytest.raises(ValueError, match="exceeds"):
        X.search(index, xyz, X.SearchConfig(radius=0.2), X.AlignConfig(0.1))
    with pytest.raises(ValueError, match="one count per pose"):
        X.search(index, xyz, X.SearchConfig(), X.AlignConfig(0.1), score=lambda *a: np.zeros(5))
    with pytest.raises(ValueError, match="finite"):
        X.search(index, np.full((10, 3), np.nan, dtype=f32), X.SearchConfig(), X.AlignConfig(0.1), score=lambda *a: np.zeros(72))


# ------------------------------------------------------------------------------------------------ the search recovers the truth
def _reference_search(src, qry, cfg):
    index = types.SimpleNamespace(src_xyz=src)

    def score(index_, sample, poses, radius):
        return S.score(src, S.ICP["radius"], sample, poses, radius)

    def step(index_, xyz, pose, radius, bits):
        assert bits is None
        return A.step(src, S.ICP["radius"], xyz, np.asarray(pose, dtype=np.float64).astype(f32), radius)[1]
    return X.search(index, qry, cfg, X.AlignConfig(**S.ICP), score=score, step=step)


def _report(name, out, truth, good):
    rec = out.search
    rot, tr = A.pose_error(out.pose, truth)
    print(f"{name}: {rec.poses} poses on {rec.sample} queries; refined {[(c['pose_index'], c['count'], c['pairs']) for c in rec.candidates]}; chosen "
          f"{rec.chosen}: {out.pairs} pairs, rms {out.rms:.6f}, rotation error {rot:.4e} rad, translation error {tr:.4e}; reference ICP from the truth: "
          f"{good['pairs']} pairs, {A.pose_error(good['pose'], truth)}")
    return rot, tr


def test_search_recovers_the_yaw_partial_overlap_case():
    """(a): 132 degrees about z, the queries cut to x < 0.1; 72 yaw steps x 27 offsets on 512 queries at radius 0.06, ICP 0.1 -> 0.04.  The pose chosen
    is held to what plain reference ICP reaches from a good start -- the truth itself: S.YAW_REF_*, recomputed here.  The fixed point ICP stops at
    depends on where it started (the pairs are between two different samples of the surfaces), by an amount of the order of that error itself: refined
    from the grid poses of both cases the reference ends between 0.7 and 1.5 of it (align_search_reference.py).  The bound is twice the recorded
    error; the start is 132 degrees away.
    The count-best candidate alone would not do: one of the first eight refines into the false optimum, with fewer pairs."""
    src, qry = S.yaw_case()
    good = A.icp(src, qry, init=S.YAW_TRUTH, **S.ICP)
    ref_rot, ref_tr = A.pose_error(good["pose"], S.YAW_TRUTH)
    assert good["converged"] and good["pairs"] == len(qry) == 4405
    assert abs(ref_rot / S.YAW_REF_ROTATION_ERROR - 1) < 0.01 and abs(ref_tr / S.YAW_REF_TRANSLATION_ERROR - 1) < 0.01
    cfg = X.SearchConfig(rotations="yaw", yaw_steps=S.YAW_STEPS, offsets=S.YAW_OFFSETS, offset_step=S.YAW_OFFSET_STEP, sample=S.SAMPLE, radius=S.SCORE_RADIUS,
                         keep=S.KEEP)
    out = _reference_search(src, qry, cfg)
    rot, tr = _report("yaw", out, S.YAW_TRUTH, good)
    rec = out.search
    assert (rec.poses, rec.sample) == (1944, 512)
    assert [c["pose_index"] for c in rec.candidates] == S.YAW_ORDER and [c["count"] for c in rec.candidates] == S.YAW_COUNTS
    assert out.converged and out.pairs == good["pairs"] and rot <= 2 * S.YAW_REF_ROTATION_ERROR and tr <= 2 * S.YAW_REF_TRANSLATION_ERROR
    assert min(c["pairs"] for c in rec.candidates) < out.pairs              # the count alone is not sufficient
    identity = A.icp(src, qry, **S.ICP)                                     # and plain ICP from the identity is nowhere near
    assert A.pose_error(identity["pose"], S.YAW_TRUTH)[0] > 1.0


def test_search_recovers_the_so3_full_overlap_case():
    """(b): 130 degrees about a skew axis, full overlap; 96 directions x 24 rolls with the centroid match alone, 512 queries; the condition and its
    bound as for (a), against S.SO3_REF_*.  Here the four refined candidates all find every pair and the rms decides."""
    src, qry = S.so3_case()
    good = A.icp(src, qry, init=S.SO3_TRUTH, **S.ICP)
    ref_rot, ref_tr = A.pose_error(good["pose"], S.SO3_TRUTH)
    assert good["converged"] and good["pairs"] == len(qry) == 6100
    assert abs(ref_rot / S.SO3_REF_ROTATION_ERROR - 1) < 0.01 and abs(ref_tr / S.SO3_REF_TRANSLATION_ERROR - 1) < 0.01
    cfg = X.SearchConfig(rotations="so3", axes=S.SO3_AXES, rolls=S.SO3_ROLLS, sample=S.SAMPLE, radius=S.SCORE_RADIUS, keep=S.SO3_KEEP)
    out = _reference_search(src, qry, cfg)
    rot, tr = _report("so3", out, S.SO3_TRUTH, good)
    rec = out.search
    assert (rec.poses, rec.sample) == (2304, 512)
    assert [c["pose_index"] for c in rec.candidates] == S.SO3_ORDER and [c["count"] for c in rec.candidates] == S.SO3_COUNTS
    assert out.converged and out.pairs == good["pairs"] and rot <= 2 * S.SO3_REF_ROTATION_ERROR and tr <= 2 * S.SO3_REF_TRANSLATION_ERROR
    assert out.rms == min(c["rms"] for c in rec.candidates)


# ------------------------------------------------------------------------------------------------ ops and the C entry
def test_score_entry_is_declared_bound_exported_and_shares_the_walk():
    from point_sam_amd import ops
    from point_sam_amd.build import SOURCES, build_library
    build_library()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pointsam_hip.h")).read()
    assert re.search(r"\bint32_t psam_pose_score\s*\(", hdr) and "psam_pose_score" in _lib.SIGNATURES and hasattr(lib, "psam_pose_score")
    assert int(re.search(r"#define PSAM_ALIGN_SCORE_POSES (\d+)\b", hdr).group(1)) == ops.ALIGN_SCORE_POSES
    assert "AT LEAST ONE candidate" in hdr and "CANNOT validate" in hdr
    assert dict(SOURCES)["align_score.hip"] == dict(SOURCES)["align.hip"] == ["-ffp-contract=off", "-fno-slp-vectorize"]
    csrc = os.path.join(ROOT, "point_sam_amd", "csrc")
    shared = open(os.path.join(csrc, "transfer_index.h")).read()
    text = open(os.path.join(csrc, "align_score.hip")).read()
    assert "bool transfer_any_candidate(" in shared and "void transfer_candidates(" in shared
    assert "transfer_any_candidate(" in text and "bool transfer_any_candidate(" not in text and '#include "transfer_index.h"' in text
    assert "__ballot" in text and "hipMalloc" not in text and "Synchronize" not in text


def test_score_entry_rejects_bad_arguments_on_the_host():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 15) & ~15               # a non-null, aligned pointer; never dereferenced by the device: every call below is refused
    org = (ctypes.c_float * 3)(-1.0, -1.0, -1.0)
    bad_org = (ctypes.c_float * 3)(-1.0, float("nan"), -1.0)

    def refused(status, code, text):      # the whole text, as the entry worded it before its checks moved into the shared header
        assert status == code, (status, lib.psam_last_error_string())
        assert lib.psam_last_error_string() == b"psam_pose_score: " + text, lib.psam_last_error_string()
    aligned = b"index_ws must be 16-byte aligned, src, qry, poses and counts 4-byte aligned"
    N, M, P, big = 1000, 100, 7, 1 << 20
    good = dict(src=p, N=N, index_ws=p, index_ws_bytes=big, origin=ctypes.addressof(org), inv_h=4.0, r2=0.0625, qry=p, M=M, poses=p, P=P, counts=p)
    call = lambda **kw: lib.psam_pose_score(*{**good, **kw}.values(), None)
    for name in ("src", "index_ws", "origin", "qry", "poses", "counts"):
        refused(call(**{name: None}), -1, b"null pointer")
    for name, word, top in (("N", b"need 0 < N <= 2^28", 1 << 28), ("M", b"need 0 < M <= 2^28", 1 << 28), ("P", b"need 0 < P <= 2^20", 1 << 20)):
        for bad in (0, -5, top + 1):
            refused(call(**{name: bad}), -1, word)
    for name in ("inv_h", "r2"):
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            refused(call(**{name: bad}), -1, name.encode() + b" must be finite and positive")
    refused(call(origin=ctypes.addressof(bad_org)), -1, b"origin must be finite")
    refused(call(index_ws=p + 8), -2, aligned)
    for name in ("src", "qry", "poses", "counts"):
        refused(call(**{name: p + 2}), -2, aligned)
    refused(call(index_ws_bytes=lib.psam_transfer_index_workspace_bytes(N) - 1), -3, b"index workspace too small (psam_transfer_index_workspace_bytes)")


def test_align_score_refuses_bad_arguments_before_the_library_is_touched(monkeypatch):
    from point_sam_amd import ops

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_library)
    index = ops.TransferIndex(torch.zeros(8, dtype=torch.int64), torch.zeros(10, 3), f32(0.25), f32(4), f32(0.0625), (-1.0, -1.0, -1.0))
    xyz = torch.zeros(100, 3)
    poses = np.stack([np.eye(4)] * 3)
    with pytest.raises(TypeError, match="TransferIndex"):
        ops.align_score("index", xyz, poses)
    with pytest.raises(TypeError):
        ops.align_score(index, xyz.double(), poses)
    with pytest.raises(ValueError):
        ops.align_score(index, torch.zeros(100, 2), poses)
    for radius in (0.26, 1.0):
        with pytest.raises(ValueError, match=r"align_score: radius .* exceeds the index's .*: the search covers the 27 cells around a query only"):
            ops.align_score(index, xyz, poses, radius)
    for radius in (0, -0.1, float("nan"), "r", True):
        with pytest.raises(ValueError, match="radius"):
            ops.align_score(index, xyz, poses, radius)
    nan = poses.copy()
    nan[1, 2, 3] = np.nan
    row = poses.copy()
    row[2, 3] = [0, 0, 0, 2]
    for bad in (nan, row, nan[:, :3], np.eye(4), np.zeros((0, 3, 4)), np.zeros((2, 3, 3)), "poses", np.full((2, 3, 4), 1e39), torch.from_numpy(nan),
                torch.zeros(3, 12)):                    # twelve words per row are taken from the DEVICE only
        with pytest.raises(ValueError, match="pose"):
            ops.align_score(index, xyz, bad)
    words = ops.transfer_poses(poses[:, :3] * 0.1)
    assert words.shape == (3, 12) and words.dtype == np.float32 and np.array_equal(words[1], ops.transfer_pose(poses[1, :3] * 0.1))
    assert np.array_equal(ops.transfer_poses(torch.from_numpy(poses)), ops.transfer_poses(poses[:, :3]))
    # good arguments on the CPU get as far as the device check, still without the library
    with pytest.raises(_lib.PointSamHipError, match="GPU"):
        ops.align_score(index, xyz, poses, 0.25)


# ------------------------------------------------------------------------------------------------ the predictor and the demo route
def test_predictor_align_refuses_a_bad_search_before_it_looks_at_the_cloud():
    from point_sam_amd import transfer as T
    from point_sam_amd.predictor import PointSAMPredictor
    pred = PointSAMPredictor(None)
    snap = T.Snapshot(torch.zeros(5, 3), torch.zeros(2, 5), 2)
    cfg = X.AlignConfig(0.1)
    with pytest.raises(TypeError, match="SearchConfig"):
        pred.align(snap, cfg, search={"keep": 2})
    with pytest.raises(ValueError, match="init and search"):
        pred.align(snap, cfg, init=np.eye(4), search=X.SearchConfig())
    with pytest.raises(ValueError, match="exceeds"):
        pred.align(snap, cfg, search=X.SearchConfig(radius=0.11))
    with pytest.raises(RuntimeError, match="set_scene"):
        pred.align(snap, cfg, search=X.SearchConfig(radius=0.1))


class FakeSearcher:
    """tests/test_align_cpu.py's stand-in predictor with the `search` argument: it answers with a fixed Alignment and logs what it was given."""
    POSE = np.array([[0.0, -1.0, 0.0, 0.125], [1.0, 0.0, 0.0, -0.25], [0.0, 0.0, 1.0, 0.5]])

    def __init__(self):
        self.log = []

    def set_pointcloud(self, xyz, rgb):
        self.xyz = xyz

    def predict_masks(self, pts, labels, prompt_mask, multimask):
        logit = 0.5 - (self.xyz[0] - pts[0][-1]).norm(dim=-1)
        return logit[None, None], torch.tensor([[0.9]]), logit[None, None]

    def snapshot(self, logits):
        return ("snap", logits.clone())

    def align(self, snap, cfg, init=None, mask=None, **kw):
        self.log.append(("align", cfg, init, mask, kw))
        out = X.Alignment(self.POSE.copy(), 41, 0.82, 0.0125, 7, True, "fixed point", [(41, 0.0125, cfg.radius)] * 7)
        if "search" in kw:
            out.search = X.SearchRecord(216, 50, [dict(pose_index=9, count=40, pairs=12, rms=float("nan"), converged=False),
                                                  dict(pose_index=3, count=38, pairs=41, rms=0.0125, converged=True)], 1)
        return out

    def propagate(self, snap, radius, pose=None):
        from point_sam_amd.transfer import Propagated
        self.log.append(("propagate", radius, pose))
        K = snap[1].shape[0]
        return Propagated(snap[1].clone(), torch.full((K,), 0.75), torch.zeros(K, dtype=torch.bool), torch.ones(K, dtype=torch.int64), 1.0,
                          torch.zeros(K, 1, 3), torch.ones(K, 1, dtype=torch.bool))


def test_propagate_route_with_search(tmp_path):
    import http.client
    import json
    import threading
    from point_sam_amd.demo_server import DemoSession, serve
    pts = np.random.RandomState(0).rand(50, 3) * 4 + 1
    for name, cloud in (("scan0.ply", pts), ("scan1.ply", pts[::-1] + 0.25)):
        with open(tmp_path / name, "w") as f:
            f.write(f"ply\nformat ascii 1.0\nelement vertex {len(cloud)}\nproperty float x\nproperty float y\nproperty float z\n"
                    "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
            f.writelines(f"{p[0]} {p[1]} {p[2]} 255 0 128\n" for p in cloud)
    pred = FakeSearcher()
    sess = DemoSession(pred, models_dir=str(tmp_path), output_dir=str(tmp_path / "results"), device="cpu")
    srv = serve(sess, "127.0.0.1", 0)
    threading.Thread(target=srv.serve_forever, daemon=True).start()

    def req(method, path, body=None):
        c = http.client.HTTPConnection("127.0.0.1", srv.server_address[1], timeout=10)
        c.request(method, path, None if body is None else json.dumps(body), {"Content-Type": "application/json"})
        r = c.getresponse()
        return r.status, json.loads(r.read())

    def first_scan_with_a_mask():
        sess.masks.clear()
        _, out = req("GET", "/pointcloud/scan0.ply")
        assert req("POST", "/segment", {"prompt_point": out["xyz"][9:12], "prompt_label": 1})[0] == 200

    try:
        body = {"pointcloud": "scan1.ply", "radius": 0.1}
        align = {"radius": 0.2, "final_radius": 0.05, "shrink": 0.5}
        given = [[1, 0, 0, 0.01], [0, 1, 0, 0], [0, 0, 1, 0]]
        # "search" without "align", with "pose", or with a bad field: this request's 400, before anything is loaded
        first_scan_with_a_mask()
        for bad in (dict(body, search={}), dict(body, align=align, pose=given, search={}), dict(body, align=align, search={"keep": 0}),
                    dict(body, align=align, search={"speed": 1}), dict(body, align=align, search=3)):
            st, out = req("POST", "/propagate", bad)
            assert st == 400 and "error" in out and sess.obj_path == "scan0.ply" and pred.log == [], bad
        # with both: predictor.align gets the SearchConfig and no init; the response's "align" carries the record
        st, out = req("POST", "/propagate", dict(body, align=align, search={"rotations": "so3", "axes": 9, "rolls": 24, "sample": 50, "keep": 2}))
        assert st == 200, out
        kind, cfg, init, mask, kw = pred.log[0]
        assert kind == "align" and cfg == X.AlignConfig(0.2, 0.05, 0.5) and init is None and mask is None and set(kw) == {"search"}
        sc = kw["search"]
        assert isinstance(sc, X.SearchConfig) and (sc.rotations, sc.axes, sc.rolls, sc.sample, sc.keep) == ("so3", 9, 24, 50, 2)
        assert pred.log[1] == ("propagate", 0.1, FakeSearcher.POSE.tolist()) and out["pose"] == FakeSearcher.POSE.tolist()
        assert out["align"] == {"pairs": 41, "coverage": 0.82, "rms": 0.0125, "iterations": 7, "converged": True, "search": {
            "poses": 216, "sample": 50, "chosen": 1, "candidates": [{"pose_index": 9, "count": 40, "pairs": 12, "rms": None, "converged": False},
                                                                    {"pose_index": 3, "count": 38, "pairs": 41, "rms": 0.0125, "converged": True}]}}
        # without "search": the call and the answer of before -- no `search` argument reaches the predictor, no "search" in the response
        first_scan_with_a_mask()
        pred.log.clear()
        st, plain = req("POST", "/propagate", dict(body, align=align, pose=given))
        assert st == 200 and pred.log[0] == ("align", X.AlignConfig(0.2, 0.05, 0.5), given, None, {})
        assert plain["align"] == {"pairs": 41, "coverage": 0.82, "rms": 0.0125, "iterations": 7, "converged": True}
        assert set(plain) == set(out) and all(plain[k] == out[k] for k in plain if k != "align")
    finally:
        srv.shutdown()
