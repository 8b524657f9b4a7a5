"""Interpolated scene masks, host side: the numpy reference (tests/interp_reference.py) against a literal per-point transcription of the definition and
its own invariants, header / binding sync and host-side argument checks of the three entry points (every call is refused before a launch), the
bindings' refusal of CPU tensors, the predictor's smooth-edges state machine with the kernels served by the reference, and the demo's option."""
import ctypes
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import crop_reference as C
import interp_reference as I
import scene_reference as R
from point_sam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTERP_ENTRY_POINTS = ("psam_interp_scene_plan", "psam_interp_scene_rows", "psam_interp_scene_bits")
f32 = np.float32


# ------------------------------------------------------------------------------------------------ the reference
def _scene(xyz, h):
    keep_idx, inv = R.downsample(xyz, h)
    wxyz = xyz[keep_idx]
    return keep_idx, inv, wxyz, I.neighbors(wxyz, h)


def _literal_plan(p, inv, wxyz, nbr, eps=1e-8):
    """The definition, one scan point at a time, on np.float32 scalars (every operation rounds to fp32)."""
    M, Nw = len(p), len(wxyz)
    idx3, w3 = np.full((M, 3), -1, dtype=np.int32), np.zeros((M, 3), dtype=f32)
    for i in range(M):
        v = int(inv[i])
        if not 0 <= v < Nw:
            continue
        cands = []
        for r in [v] + [int(x) for x in nbr[v] if x >= 0]:
            dx, dy, dz = (f32(p[i, a]) - f32(wxyz[r, a]) for a in range(3))
            cands.append((f32(f32(dx * dx + dy * dy) + dz * dz), r))
        cands.sort(key=lambda c: (float(c[0]), c[1]))
        best = cands[:3]
        if best[0][0] == 0 or len(best) == 1:
            idx3[i, 0], w3[i, 0] = best[0][1], 1
            continue
        a = [f32(1) / max(q, f32(eps)) for q, _ in best]
        s = f32(a[0] + a[1])
        if len(best) == 3:
            s = f32(s + a[2])
        for j, (_, r) in enumerate(best):
            idx3[i, j], w3[i, j] = r, f32(a[j] / s)
    return idx3, w3


def _literal_rows(src, idx3, w3, fill):
    Rr, Nw = src.shape
    out = np.empty((Rr, len(idx3)), dtype=f32)
    for i, (idx, w) in enumerate(zip(idx3, w3)):
        ok = [0 <= int(j) < Nw for j in idx]
        for r in range(Rr):
            if not ok[0]:
                out[r, i] = fill
            elif not ok[1]:
                out[r:r + 1, i:i + 1].view(np.uint32)[:] = src[r:r + 1, idx[0]:idx[0] + 1].view(np.uint32)
            else:
                acc = f32(f32(w[0] * src[r, idx[0]]) + f32(w[1] * src[r, idx[1]]))
                if ok[2]:
                    acc = f32(acc + f32(w[2] * src[r, idx[2]]))
                out[r, i] = acc
    return out


def _lattice_cloud(seed, n=400, grid=32, cells=4):
    """Coordinates on a 1 / grid lattice inside the first `cells` cells of h = 0.25 per axis: distance ties and points on cell faces are frequent."""
    rng = np.random.default_rng(seed)
    return (-1 + rng.integers(0, cells * grid // 4, (n, 3)) / grid).astype(f32)


@pytest.mark.parametrize("seed", [0, 1])
def test_reference_equals_the_literal_definition(seed):
    xyz = _lattice_cloud(seed)
    xyz[5] = xyz[R.downsample(xyz, 0.25)[0][3]]            # an exact duplicate of a representative
    keep_idx, inv, wxyz, nbr = _scene(xyz, 0.25)
    idx3, w3 = I.plan(xyz, inv, wxyz, nbr)
    lit_idx, lit_w = _literal_plan(xyz, inv, wxyz, nbr)
    assert np.array_equal(idx3, lit_idx) and np.array_equal(w3.view(np.int32), lit_w.view(np.int32))
    ties = 0
    for i in range(len(xyz)):                              # the case is worth its name: ties between a point's candidates do occur
        c = [inv[i]] + [r for r in nbr[inv[i]] if r >= 0]
        q = ((xyz[i][None] - wxyz[c]).astype(np.float64) ** 2).sum(1)
        ties += len(np.unique(q)) < len(q)
    assert ties > 20
    assert (idx3[:, 2] >= 0).any() and (idx3[:, 1] < 0).any()
    # every weight row sums to about one, indices are distinct and ascending in (q, r)
    blend = idx3[:, 1] >= 0
    assert np.allclose(w3[blend].sum(1), 1, atol=1e-6) and (w3[~blend] == np.array([1, 0, 0], dtype=f32)).all()
    assert (idx3[blend, 0] != idx3[blend, 1]).all()
    rng = np.random.default_rng(seed)
    src = rng.normal(0, 1, (3, len(wxyz))).astype(f32)
    got = I.apply_rows(src, idx3, w3, -np.inf)
    assert np.array_equal(got.view(np.int32), _literal_rows(src, idx3, w3, f32(-np.inf)).view(np.int32))
    bits, area = I.apply_bits(src, idx3, w3, 0.37)
    assert np.array_equal(R.unwords(bits, len(xyz)), got > f32(0.37)) and np.array_equal(area, (got > f32(0.37)).sum(1))


def test_reference_on_a_crop_equals_the_literal_definition():
    rng = np.random.default_rng(3)
    xyz = rng.uniform(-1, 1, (900, 3)).astype(f32)
    xyz[17] = np.nan                                       # off the ball like every non-finite point
    center, radius, h = (0.1, -0.2, 0.05), 0.6, 0.25
    keep_idx, inv, wxyz, _, members = C.crop_downsample(xyz, np.zeros_like(xyz), center, radius, h)
    assert 0 < members < 900 and inv[17] == -1
    u = I.crop_coordinate(xyz, center, radius)
    assert np.array_equal(u[keep_idx], wxyz)               # the crop cloud's own points are exact hits
    nbr = I.neighbors(wxyz, h)
    idx3, w3 = I.plan(u, inv, wxyz, nbr)
    lit_idx, lit_w = _literal_plan(u, inv, wxyz, nbr)
    assert np.array_equal(idx3, lit_idx) and np.array_equal(w3.view(np.int32), lit_w.view(np.int32))
    off = inv < 0
    assert (idx3[off] == -1).all() and (w3[off] == 0).all() and (idx3[~off, 0] >= 0).all()
    src = rng.normal(0, 1, (2, len(wxyz))).astype(f32)
    out = I.apply_rows(src, idx3, w3, -np.inf)
    assert np.isneginf(out[:, off]).all() and np.isfinite(out[:, ~off]).all()
    assert np.array_equal(out[:, keep_idx].view(np.int32), src.view(np.int32))


def test_representatives_keep_their_values_bit_for_bit():
    rng = np.random.default_rng(5)
    xyz = rng.uniform(-1, 1, (3000, 3)).astype(f32)
    keep_idx, inv, wxyz, nbr = _scene(xyz, 0.2)
    idx3, w3 = I.plan(xyz, inv, wxyz, nbr)
    assert np.array_equal(idx3[keep_idx], np.stack([np.arange(len(keep_idx)), -np.ones(len(keep_idx)), -np.ones(len(keep_idx))], 1))
    src = rng.normal(0, 1, (2, len(wxyz))).astype(f32)
    special = np.array([0x7FC12345, 0xFFA00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001], dtype=np.uint32).view(f32)      # NaNs with payloads, infinities, -0, a denormal
    src[0, :6], src[1, 6:12] = special, special
    out = I.apply_rows(src, idx3, w3)
    assert np.array_equal(out[:, keep_idx].view(np.uint32), src.view(np.uint32))
    # the 27-cell candidates hold the nearest working point: the first index is the brute-force nearest in (q, rank)
    d = ((xyz[:500, None, :].astype(np.float64) - wxyz[None].astype(np.float64)) ** 2).sum(-1)
    assert (idx3[:500, 0] == d.argmin(1)).mean() > 0.99


def test_a_one_voxel_cloud_copies():
    rng = np.random.default_rng(6)
    xyz = (rng.uniform(0.01, 0.2, (50, 3))).astype(f32)
    keep_idx, inv, wxyz, nbr = _scene(xyz, 0.25)
    assert keep_idx.tolist() == [0] and (nbr == -1).all()
    idx3, w3 = I.plan(xyz, inv, wxyz, nbr)
    assert (idx3 == np.array([0, -1, -1])).all() and (w3 == np.array([1, 0, 0], dtype=f32)).all()
    src = np.array([[np.nan], [2.5]], dtype=f32)
    src.view(np.uint32)[0, 0] = 0x7FC00BAD
    out = I.apply_rows(src, idx3, w3)
    assert (out.view(np.uint32)[0] == 0x7FC00BAD).all() and (out[1] == 2.5).all()
    bits, area = I.apply_bits(src, idx3, w3)
    assert area.tolist() == [0, 50]
    # an index outside [0, Nw) is unused: the first makes the point off, the second turns a blend into a copy
    idx = np.array([[1, 0, 0], [0, 1, 0], [0, -7, 0]], dtype=np.int32)
    w = np.full((3, 3), 0.25, dtype=f32)
    assert I.apply_rows(src[1:], idx, w, fill=-1.0).tolist() == [[-1.0, 2.5, 2.5]]


# ------------------------------------------------------------------------------------------------ the C entry points
def _ctype(decl: str):
    decl = decl.strip()
    if "*" in decl or decl.startswith("psam_stream_t"):
        return _lib.ptr
    return {"float": _lib.f32, "int32_t": _lib.i32, "int64_t": _lib.i64, "uint32_t": ctypes.c_uint32, "size_t": _lib.size_t}[decl.split()[-2] if len(decl.split()) > 1 else decl]


def test_interp_entry_points_are_declared_bound_and_exported(tmp_path):
    from point_sam_amd.build import SOURCES, build_library
    build_library()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pointsam_hip.h")).read()
    declared = set(re.findall(r"\b(psam_interp_scene_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(INTERP_ENTRY_POINTS)
    assert declared == {n for n in _lib.SIGNATURES if n.startswith("psam_interp_scene_")}
    for n in INTERP_ENTRY_POINTS:
        assert hasattr(lib, n), n
        # the header's parameter list and the ctypes signature agree, type by type
        ret, params = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % n, hdr).groups()
        want = [_ctype(p) for p in params.split(",")]
        assert ret == "int32_t" and _lib.SIGNATURES[n] == (_lib.i32, want), n
    assert ("scene_interp.hip", ["-ffp-contract=off"]) in SOURCES
    assert "interpolated scene masks */" in hdr and hdr.count("common.py:238") >= 1 and "NOT a true 3-NN" in hdr
    # the shared coordinate header: one definition for crops.hip and scene_interp.hip
    csrc = os.path.join(ROOT, "point_sam_amd", "csrc")
    assert "crop_member(" in open(os.path.join(csrc, "crop_coord.h")).read()
    for f in ("crops.hip", "scene_interp.hip"):
        src = open(os.path.join(csrc, f)).read()
        assert '#include "crop_coord.h"' in src and "bool crop_member(" not in src, f
    if shutil.which("gcc") is not None:                    # the header stays plain C with the new declarations
        src = ['#include "pointsam_hip.h"', "int main(void) {"]
        src += [f"    void* p{i} = (void*){n};" for i, n in enumerate(INTERP_ENTRY_POINTS)]
        src += ["    return " + " && ".join(f"p{i} != 0" for i in range(len(INTERP_ENTRY_POINTS))) + " ? 0 : 1;", "}"]
        c = tmp_path / "interp_symbols.c"
        c.write_text("\n".join(src))
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-Wno-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", str(c), "-o",
                        str(tmp_path / "interp_symbols.o")], check=True)


def test_interp_entry_points_reject_bad_arguments_on_the_host():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15               # a non-null, aligned pointer; never dereferenced by the device: every call below is refused
    ctr = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    c = ctypes.addressof(ctr)

    def rejected(status, word, code=-1):
        assert status == code
        msg = lib.psam_last_error_string()
        assert word in msg, msg

    plan = lib.psam_interp_scene_plan
    M, Nw, big = 1000, 100, 1 << 28
    for k in (0, 2, 3, 4, 9, 10):                          # xyz, inv, wxyz, nbr, idx3, w3
        a = [p, M, p, p, p, Nw, None, 0.0, 1e-8, p, p, None]
        a[k] = None
        rejected(plan(*a), b"null")
    for bad in (0, -1, big + 1):
        rejected(plan(p, bad, p, p, p, Nw, None, 0.0, 1e-8, p, p, None), b"M")
        rejected(plan(p, M, p, p, p, bad, None, 0.0, 1e-8, p, p, None), b"Nw")
    for bad in (float("nan"), float("inf"), -1e-8):
        rejected(plan(p, M, p, p, p, Nw, None, 0.0, bad, p, p, None), b"eps")
    for bad in (float("nan"), float("inf"), 0.0, -1.0):
        rejected(plan(p, M, p, p, p, Nw, c, bad, 1e-8, p, p, None), b"inv_r")
    for bad in (float("nan"), float("inf"), float("-inf")):
        bad_c = (ctypes.c_float * 3)(0.0, bad, 0.0)
        rejected(plan(p, M, p, p, p, Nw, ctypes.addressof(bad_c), 1.0, 1e-8, p, p, None), b"center")
    rejected(plan(p, M, p, p, p + 4, Nw, None, 0.0, 1e-8, p, p, None), b"aligned", -2)
    rejected(plan(p, M, p + 4, p, p, Nw, None, 0.0, 1e-8, p, p, None), b"aligned", -2)

    rows = lib.psam_interp_scene_rows
    for k in (0, 2, 3, 8):
        a = [p, 8, p, p, 1, 8, 8, 0.0, p, 8, None]
        a[k] = None
        rejected(rows(*a), b"null")
    rejected(rows(p, 8, p, p, 0, 8, 8, 0.0, p, 8, None), b"R > 0")
    rejected(rows(p, 8, p, p, 1, 0, 8, 0.0, p, 8, None), b"Nw")
    rejected(rows(p, 1 << 30, p, p, 1, big + 1, 8, 0.0, p, 8, None), b"Nw")
    rejected(rows(p, 8, p, p, 1, 8, 0, 0.0, p, 8, None), b"M")
    rejected(rows(p, 8, p, p, 1, 8, big + 1, 0.0, p, 1 << 30, None), b"M")
    rejected(rows(p, 7, p, p, 1, 8, 8, 0.0, p, 8, None), b"src_ld")
    rejected(rows(p, 8, p, p, 1, 8, 8, 0.0, p, 7, None), b"dst_ld")
    rejected(rows(p + 2, 8, p, p, 1, 8, 8, 0.0, p, 8, None), b"aligned", -2)

    bits = lib.psam_interp_scene_bits
    for k in (0, 2, 3, 8):
        a = [p, 64, p, p, 1, 64, 64, 0.0, p, p, None]
        a[k] = None
        rejected(bits(*a), b"null")
    rejected(bits(p, 64, p, p, 0, 64, 64, 0.0, p, None, None), b"K > 0")
    rejected(bits(p, 64, p, p, 1, 0, 64, 0.0, p, None, None), b"Nw")
    rejected(bits(p, 64, p, p, 1, 64, -1, 0.0, p, None, None), b"M")
    rejected(bits(p, 63, p, p, 1, 64, 64, 0.0, p, None, None), b"src_ld")
    rejected(bits(p, 64, p, p, 1, 64, 64, 0.0, p + 4, None, None), b"aligned", -2)


def test_interp_bindings_refuse_cpu_tensors_and_bad_values():
    from point_sam_amd import ops
    xyz, inv, wxyz, nbr = torch.zeros(8, 3), torch.zeros(8, dtype=torch.int64), torch.zeros(2, 3), torch.full((2, 26), -1, dtype=torch.int32)
    idx3, w3 = torch.zeros(8, 3, dtype=torch.int32), torch.zeros(8, 3)
    with pytest.raises(_lib.PointSamHipError):
        ops.scene_interp_plan(xyz, inv, wxyz, nbr)
    with pytest.raises(_lib.PointSamHipError):
        ops.scene_interp_plan(xyz, inv, wxyz, nbr, center=(0.0, 0.0, 0.0), radius=0.5)
    with pytest.raises(_lib.PointSamHipError):
        ops.scene_interp_rows(torch.zeros(2, 2), idx3, w3)
    with pytest.raises(_lib.PointSamHipError):
        ops.scene_interp_bits(torch.zeros(2, 2), idx3, w3)


# ------------------------------------------------------------------------------------------------ the predictor, kernels served by the references
def _reference_ops(monkeypatch, log):
    from point_sam_amd import ops
    t = torch.from_numpy

    def voxel_downsample(xyz, voxel_size, origin=(-1.0, -1.0, -1.0)):
        k, i = R.downsample(xyz.numpy(), voxel_size, origin)
        return t(k), t(i)

    def voxel_count(xyz, voxel_size, origin=(-1.0, -1.0, -1.0)):
        return len(R.downsample(xyz.numpy(), voxel_size, origin)[0])

    def crop_downsample(xyz, rgb, center, radius, voxel_size=None):
        k, i, wx, wr, m = C.crop_downsample(xyz.numpy(), rgb.numpy(), center, radius, voxel_size)
        return t(k), t(i), t(wx), t(wr), m

    def crop_count(xyz, center, radius, voxel_size=None):
        k, _, _, _, m = C.crop_downsample(xyz.numpy(), np.zeros_like(xyz.numpy()), center, radius, voxel_size)
        return len(k), m

    def scene_expand_rows(src, inv, out=None):
        log.append("scene_expand_rows")
        return src[..., inv]

    def crop_expand_rows(src, inv, fill, out=None):
        log.append("crop_expand_rows")
        lead = tuple(src.shape[:-1])
        return t(C.expand_rows(src.reshape(-1, src.shape[-1]).numpy(), inv.numpy(), np.asarray(fill, dtype=f32))).reshape(lead + (inv.numel(),))

    def region_neighbors(xyz, keep_idx, voxel_size, origin=(-1.0, -1.0, -1.0)):
        log.append(("region_neighbors", tuple(xyz.shape), keep_idx.numel(), voxel_size))
        return t(I.neighbors(xyz.numpy()[keep_idx.numpy()], voxel_size, origin))

    def scene_interp_plan(xyz, inv, wxyz, nbr, center=None, radius=None, eps=1e-8):
        log.append(("scene_interp_plan", center, radius))
        p = xyz.numpy() if center is None else I.crop_coordinate(xyz.numpy(), center, radius)
        idx3, w3 = I.plan(p, inv.numpy(), wxyz.numpy(), nbr.numpy(), eps)
        return t(idx3), t(w3)

    def scene_interp_rows(src, idx3, w3, fill=None, out=None):
        log.append(("scene_interp_rows", fill))
        lead = tuple(src.shape[:-1])
        rows = I.apply_rows(src.reshape(-1, src.shape[-1]).numpy(), idx3.numpy(), w3.numpy(), 0.0 if fill is None else fill)
        return t(rows).reshape(lead + (idx3.shape[0],))

    def scene_interp_bits(src, idx3, w3, thr=0.0, area=True):
        log.append(("scene_interp_bits", thr))
        b, a = I.apply_bits(src.reshape(-1, src.shape[-1]).numpy(), idx3.numpy(), w3.numpy(), thr)
        return t(b.view(np.int64)), t(a)

    def mask_pack(logits, thr=0.0, off=1.0, out=None, row=0):
        log.append(("mask_pack", thr))
        m = logits.reshape(-1, logits.shape[-1]).numpy() > f32(thr)
        return t(R.words(m).view(np.int64)), t(m.sum(1).astype(np.int32)), None, None

    def scene_expand_bits(bits, inv, Nw, area=True):
        log.append("scene_expand_bits")
        b, a = R.expand_bits(bits.numpy().view(np.uint64), inv.numpy(), Nw)
        return t(b.view(np.int64)), t(a)

    def crop_expand_bits(bits, inv, Nw, area=True):
        log.append("crop_expand_bits")
        b, a = C.expand_bits(bits.numpy().view(np.uint64), inv.numpy(), Nw)
        return t(b.view(np.int64)), t(a)

    for fn in (voxel_downsample, voxel_count, crop_downsample, crop_count, scene_expand_rows, crop_expand_rows, region_neighbors, scene_interp_plan,
               scene_interp_rows, scene_interp_bits, mask_pack, scene_expand_bits, crop_expand_bits):
        monkeypatch.setattr(ops, fn.__name__, fn)


class StubModel:
    """encode: remembers the cloud; decode: logit = 1 - 2 |x - first prompt| per point (+ an eighth of the mask prompt), three shifted candidates."""

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


class _NoModel:
    def __getattr__(self, name):
        raise AssertionError("the model must not be reached")


def test_smooth_argument_validation():
    from point_sam_amd.predictor import PointSAMPredictor
    pred = PointSAMPredictor(_NoModel())
    xyz, rgb = torch.zeros(10, 3), torch.zeros(10, 3)
    for bad in (None, 1, 0, "yes", 1.0):
        with pytest.raises(ValueError, match="smooth"):
            pred.set_scene(xyz, rgb, max_points=5, smooth=bad)
    for bad in (1, 0, "no", 0.0):
        with pytest.raises(ValueError, match="smooth"):      # refused before the missing scene is noticed
            pred.set_crop((0.0, 0.0, 0.0), 0.5, smooth=bad)
    with pytest.raises(RuntimeError, match="set_scene"):
        pred.set_crop((0.0, 0.0, 0.0), 0.5, smooth=None)
    assert pred.scene is None


def test_predictor_smooth_state_machine(monkeypatch):
    from point_sam_amd.predictor import PointSAMPredictor
    log = []
    _reference_ops(monkeypatch, log)
    rng = np.random.default_rng(9)
    xyz, rgb = torch.from_numpy(rng.uniform(-1, 1, (700, 3)).astype(f32)), torch.from_numpy(rng.uniform(0, 1, (700, 3)).astype(f32))
    h = 0.25
    keep_idx, inv, wxyz, nbr = _scene(xyz.numpy(), h)
    idx3, w3 = I.plan(xyz.numpy(), inv, wxyz, nbr)
    model = StubModel()
    pred = PointSAMPredictor(model)
    click, one = xyz[int(keep_idx[3])][None, None], torch.ones(1, 1, dtype=torch.int64)

    def interp_calls():
        return [c for c in log if isinstance(c, tuple) and c[0] in ("region_neighbors", "scene_interp_plan")]

    # off by default: the voxel transfer, and no plan is ever built
    pred.set_scene(xyz, rgb, voxel_size=h)
    state = pred._state
    coarse, _, _ = pred.predict_masks(click, one, None, True)
    work = model.decode(state, click, one, None, True)[0]
    assert torch.equal(coarse, work[..., torch.from_numpy(inv)]) and log == ["scene_expand_rows"]
    # on: the same state (smooth is no part of the key), the plan built by the first prediction and kept
    pred.set_scene(xyz, rgb, voxel_size=h, smooth=True)
    assert pred._state is state and model.encoded == [(1, len(keep_idx), 3)] and interp_calls() == []
    smooth, scores, _ = pred.predict_masks(click, one, None, True)
    assert interp_calls() == [("region_neighbors", (700, 3), len(keep_idx), h), ("scene_interp_plan", None, None)]
    want = I.apply_rows(work[0].numpy(), idx3, w3)
    assert tuple(smooth.shape) == (1, 3, 700) and np.array_equal(smooth[0].numpy().view(np.int32), want.view(np.int32))
    assert torch.equal(smooth[..., torch.from_numpy(keep_idx)], work) and not torch.equal(smooth, coarse)
    again, _, _ = pred.predict_masks(click, one, None, True)
    assert torch.equal(again, smooth) and len(interp_calls()) == 2
    # the scan-width smooth logits as the next click's mask prompt: exactly the working-width logits
    pred.predict_masks(click, one, smooth[0][1][None], False)
    assert torch.equal(model.last[2], work[0][1][None])
    # the bits: the same decision without the floats; off again: mask_pack + the voxel expansion
    del log[:]
    bits, area, s2 = pred.predict_mask_bits(click, one, None, True, threshold=0.25)
    assert log == [("scene_interp_bits", 0.25)] and torch.equal(s2, scores)
    assert np.array_equal(R.unwords(bits.numpy().view(np.uint64), 700), smooth[0].numpy() > f32(0.25)) and area.tolist() == (smooth[0] > 0.25).sum(1).tolist()
    pred.set_scene(xyz, rgb, voxel_size=h)
    del log[:]
    bits, area, _ = pred.predict_mask_bits(click, one, None, True, threshold=0.25)
    assert log == [("mask_pack", 0.25), "scene_expand_bits"]
    assert np.array_equal(R.unwords(bits.numpy().view(np.uint64), 700), coarse[0].numpy() > f32(0.25))
    assert pred._state is state and len(model.encoded) == 1
    # a crop takes the scene's setting unless told otherwise; its plan lives with the cached crop and survives clear_crop()
    center, r, hc = (0.1, -0.2, 0.05), 0.7, 0.25
    ck, ci, cw, _, members = C.crop_downsample(xyz.numpy(), rgb.numpy(), center, r, hc)
    cidx, cwt = I.plan(I.crop_coordinate(xyz.numpy(), center, r), ci, cw, I.neighbors(cw, hc))
    cclick = xyz[int(ck[3])][None, None]                   # a click inside the ball
    pred.set_scene(xyz, rgb, voxel_size=h, smooth=True)
    pred.set_crop(center, r, voxel_size=hc)
    crop_state = pred._crop_state
    del log[:]
    got, _, _ = pred.predict_masks(cclick, one, None, True)
    assert interp_calls() == [("region_neighbors", (len(ck), 3), len(ck), hc), ("scene_interp_plan", pred.crop.center, pred.crop.radius)]
    assert ("scene_interp_rows", float("-inf")) in log and "crop_expand_rows" not in log
    cwork = model.decode(crop_state, model.last[1], one, None, True)[0]
    assert np.array_equal(got[0].numpy().view(np.int32), I.apply_rows(cwork[0].numpy(), cidx, cwt, -np.inf).view(np.int32))
    assert torch.isneginf(got[0][:, torch.from_numpy(ci < 0)]).all() and torch.equal(got[..., torch.from_numpy(ck)], cwork)
    pred.clear_crop()
    pred.set_crop(center, r, voxel_size=hc, smooth=False)      # the same crop, not smooth: the cache hits, the voxel transfer answers
    del log[:]
    hard, _, _ = pred.predict_masks(cclick, one, None, True)
    assert pred._crop_state is crop_state and log == ["crop_expand_rows"] and not torch.equal(hard, got)
    bits, _, _ = pred.predict_mask_bits(cclick, one, None, True)
    assert log[1:] == [("mask_pack", 0.0), "crop_expand_bits"] and np.array_equal(R.unwords(bits.numpy().view(np.uint64), 700), hard[0].numpy() > 0)
    pred.set_crop(center, r, voxel_size=hc, smooth=True)       # smooth again: the plan was kept
    del log[:]
    back, _, _ = pred.predict_masks(cclick, one, None, True)
    assert torch.equal(back, got) and interp_calls() == [] and len(model.encoded) == 2
    # a scene that is its own working cloud, a crop without a voxel size and a plain cloud have nothing to blend
    pred2 = PointSAMPredictor(StubModel())
    pred2.set_scene(xyz, rgb, max_points=700, smooth=True)
    del log[:]
    pred2.predict_masks(click, one, None, True)
    assert pred2._scene_plan is None and log == []
    pred2.set_crop(center, r)
    pred2.predict_masks(xyz[int(ck[3])][None, None], one, None, True)
    assert log == ["crop_expand_rows"] and pred2._crop_cache[3] is None
    pred2.set_pointcloud(xyz[None], rgb[None])
    del log[:]
    bits, area, _ = pred2.predict_mask_bits(click, one, None, False)
    assert log == [("mask_pack", 0.0)] and tuple(bits.shape) == (1, 11)


# ------------------------------------------------------------------------------------------------ the demo
class FakePredictor:
    def __init__(self):
        self.calls = []
        self.crop = None

    def set_pointcloud(self, xyz, rgb):
        self.calls.append(("set_pointcloud",))
        self.n = xyz.shape[1]

    def set_scene(self, xyz, rgb, voxel_size=None, max_points=None, smooth=False):
        self.calls.append(("set_scene", max_points, smooth))
        self.n = xyz.shape[1]

    def set_crop(self, center, radius, voxel_size=None, max_points=None, smooth=None):
        self.calls.append(("set_crop", max_points, smooth))
        self.crop = types.SimpleNamespace(num_members=5, num_working=5)

    def predict_masks(self, pts, lab, prompt_mask, multimask):
        logits = torch.linspace(-1, 1, self.n).repeat(1, 3 if multimask else 1, 1)
        return logits, torch.tensor([[0.1, 0.9, 0.5][:logits.shape[1]]]), logits


def test_demo_session_forwards_smooth_edges(tmp_path):
    from point_sam_amd.demo_server import DemoSession
    cloud = {"points": {str(i): 0.01 * i for i in range(120)}, "colors": {str(i): 0.5 for i in range(120)}}
    click = {"prompt_point": [0.1, 0.2, 0.3], "prompt_label": 1}
    pred = FakePredictor()
    sess = DemoSession(pred, models_dir=str(tmp_path), output_dir=str(tmp_path / "r"), device="cpu", working_points=16, crop_points=8, smooth_edges=True)
    sess.sampled_pointcloud(cloud)
    assert len(sess.segment(click)["seg"]) == 40
    sess.set_crop({"center": [0.5, 0.5, 0.5], "radius": 0.4})
    sess.segment(click)
    assert pred.calls == [("set_scene", 16, True), ("set_scene", 16, True), ("set_crop", 8, True), ("set_scene", 16, True), ("set_crop", 8, True)]
    # off (the default): the keyword is not passed at all, so a predictor without it keeps working
    pred = FakePredictor()
    sess = DemoSession(pred, models_dir=str(tmp_path), output_dir=str(tmp_path / "r"), device="cpu", working_points=16)
    assert sess.smooth_edges is False
    sess.sampled_pointcloud(cloud)
    sess.segment(click)
    sess.set_crop({"center": [0.5, 0.5, 0.5], "radius": 0.4})
    assert pred.calls == [("set_scene", 16, False), ("set_scene", 16, False), ("set_crop", None, None)]
    # without a working cloud or a crop there is nothing to smooth: the plain cloud path is unchanged
    pred = FakePredictor()
    sess = DemoSession(pred, models_dir=str(tmp_path), output_dir=str(tmp_path / "r"), device="cpu", smooth_edges=True)
    sess.sampled_pointcloud(cloud)
    sess.segment(click)
    assert pred.calls == [("set_pointcloud",)]
    for bad in (1, None, "yes"):
        with pytest.raises(ValueError, match="smooth_edges"):
            DemoSession(FakePredictor(), device="cpu", smooth_edges=bad)


def test_demo_parser_has_the_smooth_edges_option():
    from point_sam_amd.demo_server import build_parser
    assert build_parser().parse_args([]).smooth_edges is False
    args = build_parser().parse_args(["--smooth-edges", "--working-points", "4096"])
    assert args.smooth_edges is True and args.working_points == 4096
    src = open(os.path.join(ROOT, "point_sam_amd", "demo_server.py")).read()
    assert "smooth_edges=args.smooth_edges" in src
