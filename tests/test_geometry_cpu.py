"""Instance geometry, host side: the numpy reference (tests/geometry_reference.py) against a literal transcription, header / binding sync and
host-side argument checks of the C entry points (every call is refused before a launch), the bindings' argument validation, the host maths of
point_sam_amd/geometry.py with the two kernels served by the reference, the predictor's width checks and error types with a stub model, and the
demo's two new routes with a stub predictor."""
import ctypes
import http.client
import json
import math
import os
import re
import shutil
import subprocess
import threading
import types

import numpy as np
import pytest
import torch

import geometry_reference as G
from point_sam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRY_ENTRY_POINTS = ("psam_instance_moments_workspace_bytes", "psam_instance_moments", "psam_instance_extents_workspace_bytes", "psam_instance_extents")
f32 = np.float32


# ------------------------------------------------------------------------------------------------ the reference
def test_reference_equals_a_literal_transcription():
    """A check of the yardstick, not of the feature: it exercises tests/geometry_reference.py alone (and so would pass without the kernels)."""
    rng = np.random.default_rng(0)
    N = 203
    xyz, rgb = rng.uniform(-4, 4, (N, 3)).astype(f32), rng.uniform(-1, 1, (N, 3)).astype(f32)
    mask = np.stack([rng.random(N) < 0.3, np.zeros(N, dtype=bool), np.ones(N, dtype=bool)])
    bits = G.words(mask)
    assert bits.shape == (3, 4) and bits.dtype == np.int64
    dirty = bits.copy()
    dirty[:, -1] |= np.int64(-1) << np.int64(N % 64)      # bits past N are ignored
    for b in (bits, dirty):
        for k in range(3):
            assert np.array_equal(G.members(b[k], N), np.nonzero(mask[k])[0])
    count, sums, lo, hi, abs_sums = G.mask_moments(xyz, dirty, rgb)
    assert count.tolist() == mask.sum(1).tolist() and (sums[1] == 0).all() and np.isposinf(lo[1]).all() and np.isneginf(hi[1]).all()
    from fractions import Fraction
    idx = np.nonzero(mask[0])[0]
    exact = sum(Fraction(float(xyz[i, 0])) * Fraction(float(xyz[i, 1])) for i in idx)      # sum xy in rational arithmetic
    assert sums[0, 4] == float(exact)                      # fsum is the correctly rounded exact sum
    assert sums[0, 9] == float(sum(Fraction(float(rgb[i, 0])) for i in idx))
    assert np.array_equal(lo[0], xyz[idx].min(0)) and np.array_equal(hi[2], xyz.max(0))
    assert (abs_sums >= np.abs(sums)).all()
    # the extents, one point and one operation at a time on np.float32 scalars
    origin, axes = rng.uniform(-1, 1, (3, 3)).astype(f32), rng.uniform(-1.5, 1.5, (3, 3, 3)).astype(f32)
    elo, ehi, r2max = G.mask_extents(xyz, dirty, origin, axes)
    p_all, r_all = [], []
    for i in idx:
        d = [f32(xyz[i, a] - origin[0, a]) for a in range(3)]
        p_all.append([f32(f32(f32(d[0] * axes[0, c, 0]) + f32(d[1] * axes[0, c, 1])) + f32(d[2] * axes[0, c, 2])) for c in range(3)])
        r_all.append(f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2])))
    assert np.array_equal(elo[0], np.min(p_all, 0)) and np.array_equal(ehi[0], np.max(p_all, 0)) and r2max[0] == max(r_all)
    assert np.isposinf(elo[1]).all() and np.isneginf(ehi[1]).all() and np.isneginf(r2max[1])
    flat = G.mask_extents(xyz, bits, origin, None)
    assert np.array_equal(flat[0][2], (xyz - origin[2]).astype(f32).min(0))
    # -0 orders below +0
    z = np.array([0.0, -0.0, 0.0], dtype=f32)
    assert np.signbit(G.ordered_min(z)) and not np.signbit(G.ordered_max(z))


# ------------------------------------------------------------------------------------------------ the C entry points
def _ctype(decl: str):
    decl = decl.strip()
    if "*" in decl or decl.startswith("psam_stream_t"):
        return _lib.ptr
    return {"float": _lib.f32, "int32_t": _lib.i32, "int64_t": _lib.i64, "size_t": _lib.size_t}[decl.split()[-2] if len(decl.split()) > 1 else decl]


def test_geometry_entry_points_are_declared_bound_and_exported(tmp_path):
    from point_sam_amd import ops
    from point_sam_amd.build import SOURCES, build_library
    build_library()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pointsam_hip.h")).read()
    declared = set(re.findall(r"\b(psam_instance_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(GEOMETRY_ENTRY_POINTS)
    assert declared == {n for n in _lib.SIGNATURES if n.startswith("psam_instance_")}
    for n in GEOMETRY_ENTRY_POINTS:
        assert hasattr(lib, n), n
        ret, params = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % n, hdr).groups()
        want = [_ctype(p) for p in params.split(",")]
        assert _lib.SIGNATURES[n] == (_lib.size_t if n.endswith("_bytes") else _lib.i32, want) and ret == ("size_t" if n.endswith("_bytes") else "int32_t"), n
    flags = dict(SOURCES)["geometry.hip"]
    assert "-ffp-contract=off" in flags
    assert "instance geometry */" in hdr and "No float atomics" in hdr
    assert int(re.search(r"#define PSAM_INSTANCE_RANGE_WORDS (\d+)", hdr).group(1)) == ops.INSTANCE_RANGE_WORDS
    src = open(os.path.join(ROOT, "point_sam_amd", "csrc", "geometry.hip")).read()
    assert "atomic" not in src.split("#include")[1] and src.count("geom_walk(") == 3      # no atomics; one bit walk, used by both kernels
    if shutil.which("gcc") is not None:                    # the header stays plain C with the new declarations
        prog = ['#include "pointsam_hip.h"', "int main(void) {"]
        prog += [f"    void* p{i} = (void*){n};" for i, n in enumerate(GEOMETRY_ENTRY_POINTS)]
        prog += ["    return " + " && ".join(f"p{i} != 0" for i in range(len(GEOMETRY_ENTRY_POINTS))) + " && PSAM_INSTANCE_RANGE_WORDS > 0 ? 0 : 1;", "}"]
        c = tmp_path / "geometry_symbols.c"
        c.write_text("\n".join(prog))
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-Wno-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", str(c), "-o",
                        str(tmp_path / "geometry_symbols.o")], check=True)


def test_geometry_entry_points_reject_bad_arguments_on_the_host():
    from point_sam_amd import ops
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15               # a non-null, aligned pointer; never dereferenced by the device: every call below is refused

    def rejected(status, word, code=-1):
        assert status == code
        msg = lib.psam_last_error_string()
        assert word in msg, msg

    R = ops.INSTANCE_RANGE_WORDS * 64
    mw, ew = lib.psam_instance_moments_workspace_bytes, lib.psam_instance_extents_workspace_bytes
    # one partial per (row, range of 256 words): twelve fp64 sums, a count and six box keys; seven keys for the extents
    assert mw(1, 1) == mw(1, R) == 124 and mw(1, R + 1) == 248 and mw(3, 5 * R) == 3 * 5 * 124 and mw(256, 4000000) == 256 * 245 * 124
    assert ew(1, R) == 28 and ew(1, R + 1) == 56 and ew(65, 3 * R + 1) == 65 * 4 * 28
    for bad in ((0, 64), (-1, 64), (65536, 64), (1, 0), (1, -5), (1, (1 << 28) + 1)):
        assert mw(*bad) == 0 and ew(*bad) == 0
    big = 1 << 30
    mom, ext = lib.psam_instance_moments, lib.psam_instance_extents
    for k in (0, 2, 5, 6, 7, 8, 9):                       # xyz, bits, count, sums, lo, hi, ws; rgb may be null
        a = [p, None, p, 1, 64, p, p, p, p, p, big, None]
        a[k] = None
        rejected(mom(*a), b"null")
    for K, N in ((0, 64), (-1, 64), (65536, 64)):
        rejected(mom(p, p, p, K, N, p, p, p, p, p, big, None), b"K")
        rejected(ext(p, p, K, N, p, None, p, p, p, p, big, None), b"K")
    for N in (0, -64, (1 << 28) + 1):
        rejected(mom(p, p, p, 1, N, p, p, p, p, p, big, None), b"N")
        rejected(ext(p, p, 1, N, p, p, p, p, p, p, big, None), b"N")
    rejected(mom(p, p, p, 2, R + 1, p, p, p, p, p, mw(2, R + 1) - 1, None), b"workspace")
    rejected(ext(p, p, 2, R + 1, p, p, p, p, p, p, ew(2, R + 1) - 1, None), b"workspace")
    for k in (0, 1, 4, 6, 7, 8, 9):                       # xyz, bits, origin, lo, hi, r2max, ws; axes may be null
        a = [p, p, 1, 64, p, None, p, p, p, p, big, None]
        a[k] = None
        rejected(ext(*a), b"null")
    rejected(mom(p, p, p + 4, 1, 64, p, p, p, p, p, big, None), b"aligned", -2)
    rejected(mom(p, p, p, 1, 64, p, p + 4, p, p, p, big, None), b"aligned", -2)
    rejected(mom(p + 2, p, p, 1, 64, p, p, p, p, p, big, None), b"aligned", -2)
    rejected(ext(p, p + 4, 1, 64, p, p, p, p, p, p, big, None), b"aligned", -2)
    rejected(ext(p, p, 1, 64, p, p + 1, p, p, p, p, big, None), b"aligned", -2)


def test_geometry_bindings_validate_before_any_library_call(monkeypatch):
    from point_sam_amd import ops
    xyz, bits = torch.zeros(100, 3), torch.zeros(2, 2, dtype=torch.int64)
    with pytest.raises(_lib.PointSamHipError):             # no CPU fall-back
        ops.mask_moments(xyz, bits)
    with pytest.raises(_lib.PointSamHipError):
        ops.mask_extents(xyz, bits, torch.zeros(2, 3))

    def no_library():
        raise AssertionError("the library must not be reached")
    monkeypatch.setattr(_lib, "load", no_library)
    # Past the device check the REAL ops._chk (dtype, contiguity) and the wrappers' own shape checks are exercised: CPU tensors are made to
    # report is_cuda for the rest of this test, and the library is out of reach, so nothing can be launched on them.
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    org, axes = torch.zeros(2, 3), torch.zeros(2, 3, 3)
    bad_moments = [
        (TypeError, (xyz.double(), bits)), (TypeError, (xyz, bits.int())), (TypeError, (xyz, bits, xyz.half())),
        (ValueError, (torch.zeros(3, 100).t(), bits)), (ValueError, (xyz, torch.zeros(2, 4, dtype=torch.int64)[:, ::2])),
        (ValueError, (torch.zeros(100, 4), bits)), (ValueError, (torch.zeros(2, 100, 3), bits)), (ValueError, (torch.zeros(0, 3), bits[:, :0].contiguous())),
        (ValueError, (xyz, torch.zeros(2, 3, dtype=torch.int64))), (ValueError, (xyz, torch.zeros(2, 1, dtype=torch.int64))),
        (ValueError, (xyz, torch.zeros(4, dtype=torch.int64))), (ValueError, (xyz, torch.zeros(0, 2, dtype=torch.int64))),
        (ValueError, (xyz, bits, torch.zeros(99, 3))), (ValueError, (xyz, bits, torch.zeros(100, 3, 1))),
    ]
    for err, args in bad_moments:
        with pytest.raises(err):
            ops.mask_moments(*args)
    bad_extents = [
        (ValueError, (xyz, torch.zeros(2, 3, dtype=torch.int64), org)), (ValueError, (xyz, bits, torch.zeros(3, 3))), (ValueError, (xyz, bits, torch.zeros(2, 4))),
        (TypeError, (xyz, bits, org.double())), (ValueError, (xyz, bits, org, torch.zeros(2, 9))), (ValueError, (xyz, bits, org, torch.zeros(3, 3, 3))),
        (TypeError, (xyz, bits, org, axes.double())), (ValueError, (xyz, bits, org, torch.zeros(2, 3, 6)[:, :, ::2])),
    ]
    for err, args in bad_extents:
        with pytest.raises(err):
            ops.mask_extents(*args)
    with pytest.raises(AssertionError, match="library"):   # a good call passes every check and reaches the library; [1, N, 3] is one cloud
        ops.mask_moments(xyz[None], bits, xyz)
    with pytest.raises(AssertionError, match="library"):
        ops.mask_extents(xyz, bits, org, axes)


# ------------------------------------------------------------------------------------------------ host maths, kernels served by the reference
def _reference_geometry_ops(monkeypatch, log=None):
    from point_sam_amd import ops
    t = torch.from_numpy

    def mask_moments(xyz, bits, rgb=None):
        if log is not None:
            log.append(("mask_moments", tuple(xyz.shape), tuple(bits.shape), rgb is not None))
        x = xyz[0] if xyz.dim() == 3 else xyz
        count, sums, lo, hi, _ = G.mask_moments(x.numpy(), bits.numpy(), None if rgb is None else rgb.reshape(-1, 3).numpy())
        return t(count), t(sums), t(lo), t(hi)

    def mask_extents(xyz, bits, origin, axes=None):
        if log is not None:
            log.append(("mask_extents", tuple(xyz.shape), tuple(bits.shape), axes is not None))
        x = xyz[0] if xyz.dim() == 3 else xyz
        return tuple(t(a) for a in G.mask_extents(x.numpy(), bits.numpy(), origin.numpy(), None if axes is None else axes.numpy()))

    monkeypatch.setattr(ops, "mask_moments", mask_moments)
    monkeypatch.setattr(ops, "mask_extents", mask_extents)


def _blob(rng, n, scale, rot, shift):
    return ((rng.normal(0, 1, (n, 3)) * scale) @ rot + shift).astype(f32)


def _rotation(a, b, c):
    ca, sa, cb, sb, cc, sc = math.cos(a), math.sin(a), math.cos(b), math.sin(b), math.cos(c), math.sin(c)
    return (np.array([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1]]) @ np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]]) @ np.array([[1, 0, 0], [0, cc, -sc], [0, sc, cc]])).T


def test_mask_geometry_host_maths(monkeypatch):
    from point_sam_amd.geometry import InstanceGeometry, mask_geometry
    log = []
    _reference_geometry_ops(monkeypatch, log)
    rng = np.random.default_rng(4)
    rot = _rotation(0.5, -0.8, 0.3)                        # rows: the generating axes
    a = _blob(rng, 400, (0.5, 0.2, 0.05), rot, (0.3, -0.1, 0.2))
    b = _blob(rng, 300, (0.05, 0.4, 0.15), np.eye(3), (-0.5, 0.5, 0.0))
    xyz = np.concatenate([a, b, rng.uniform(-1, 1, (324, 3)).astype(f32)])
    rgb = rng.uniform(0, 1, (len(xyz), 3)).astype(f32)
    mask = np.zeros((4, len(xyz)), dtype=bool)
    mask[0, :400], mask[1, 400:700], mask[3, 5] = True, True, True      # row 2 is empty, row 3 a single point
    bits = torch.from_numpy(G.words(mask))
    geo = mask_geometry(torch.from_numpy(xyz), bits, torch.from_numpy(rgb))
    assert isinstance(geo, InstanceGeometry) and len(geo) == 4 and [c[0] for c in log] == ["mask_moments", "mask_extents"] and log[1][3] is True
    assert geo.count.tolist() == [400, 300, 0, 1] and geo.valid.tolist() == [True, True, False, True]
    assert (geo.count.dtype, geo.centroid.dtype, geo.aabb_lo.dtype, geo.covariance.dtype, geo.mean_rgb.dtype, geo.axes.dtype, geo.obb_center.dtype,
            geo.obb_half.dtype, geo.radius.dtype, geo.valid.dtype) == (torch.int32, torch.float64, torch.float32, torch.float64, torch.float64, torch.float32,
                                                                       torch.float64, torch.float64, torch.float32, torch.bool)
    for k, sel in ((0, slice(0, 400)), (1, slice(400, 700))):
        p = xyz[sel].astype(np.float64)
        assert np.allclose(geo.centroid[k].numpy(), p.mean(0), rtol=0, atol=1e-14)
        assert np.allclose(geo.covariance[k].numpy(), np.cov(p.T, bias=True), rtol=0, atol=1e-14)
        assert np.array_equal(geo.covariance[k].numpy(), geo.covariance[k].numpy().T)
        assert np.allclose(geo.mean_rgb[k].numpy(), rgb[sel].astype(np.float64).mean(0), rtol=0, atol=1e-14)
        assert np.array_equal(geo.aabb_lo[k].numpy(), xyz[sel].min(0)) and np.array_equal(geo.aabb_hi[k].numpy(), xyz[sel].max(0))
        ax = geo.axes[k].numpy().astype(np.float64)
        # descending eigenvalues: the variance along axis 0 >= axis 1 >= axis 2, and the axes are the covariance's eigenvectors
        var = np.array([ax[i] @ geo.covariance[k].numpy() @ ax[i] for i in range(3)])
        assert var[0] >= var[1] >= var[2] and np.allclose(var, np.linalg.eigvalsh(np.cov(p.T, bias=True))[::-1], rtol=1e-5)
        for i in (0, 1):                                   # sign convention: the largest component of axes 0 and 1 is positive
            assert ax[i, np.argmax(np.abs(ax[i]))] > 0
        assert np.allclose(np.cross(ax[0], ax[1]), ax[2], atol=1e-6) and abs(np.linalg.det(ax) - 1) < 1e-6      # right-handed
        assert np.allclose(ax @ ax.T, np.eye(3), atol=1e-6)
        # the box is tight in its frame and holds every member; the radius reaches the farthest one
        q = (p - geo.obb_center[k].numpy()) @ ax.T
        half = geo.obb_half[k].numpy()
        assert (np.abs(q) <= half + 1e-5).all() and np.allclose(np.abs(q).max(0), half, atol=1e-5)
        assert abs(float(geo.radius[k]) - np.linalg.norm(p - geo.centroid[k].numpy(), axis=1).max()) < 1e-5
    assert (np.abs(geo.axes[0].numpy() @ rot.T).max(1) > 0.99).all()       # the elongated blob's frame is the generating one, up to order and sign
    assert np.abs(geo.axes[0].numpy()[0] @ rot[0]) > 0.99
    # an empty row is NaN, not garbage
    for name in ("centroid", "aabb_lo", "aabb_hi", "covariance", "mean_rgb", "axes", "obb_center", "obb_half", "radius"):
        assert bool(torch.isnan(getattr(geo, name)[2]).all()), name
        assert bool(torch.isfinite(getattr(geo, name)[[0, 1, 3]]).all()), name
    # a single point: a degenerate but finite box of size zero around it
    assert np.allclose(geo.centroid[3].numpy(), xyz[5]) and (geo.obb_half[3] == 0).all() and float(geo.radius[3]) == 0.0
    assert abs(np.linalg.det(geo.axes[3].numpy().astype(np.float64)) - 1) < 1e-6

    log.clear()
    flat = mask_geometry(torch.from_numpy(xyz), bits, None, oriented=False)
    assert [c[0] for c in log] == ["mask_moments", "mask_extents"] and log[0][3] is False and log[1][3] is False      # no eigen step, no axes
    assert flat.mean_rgb is None
    for k in (0, 1, 3):
        assert np.array_equal(flat.axes[k].numpy(), np.eye(3, dtype=f32))
        lo, hi = flat.aabb_lo[k].numpy().astype(np.float64), flat.aabb_hi[k].numpy().astype(np.float64)
        assert np.array_equal(flat.obb_center[k].numpy(), (lo + hi) / 2) and np.array_equal(flat.obb_half[k].numpy(), (hi - lo) / 2)
        assert float(flat.radius[k]) == float(geo.radius[k])
    assert bool(torch.isnan(flat.axes[2]).all()) and bool(torch.isnan(flat.obb_half[2]).all()) and not bool(flat.valid[2])
    assert torch.equal(flat.centroid[[0, 1, 3]], geo.centroid[[0, 1, 3]])
    with pytest.raises(ValueError, match="oriented"):
        mask_geometry(torch.from_numpy(xyz), bits, None, oriented=1)
    none = mask_geometry(torch.from_numpy(xyz), bits[:0], None)
    assert len(none) == 0 and tuple(none.axes.shape) == (0, 3, 3)


def test_principal_axes_order_and_signs():
    from point_sam_amd.geometry import principal_axes
    rot = _rotation(1.0, 0.4, -0.7)
    cov = np.stack([rot.T @ np.diag(d) @ rot for d in ((3.0, 2.0, 1.0), (1.0, 3.0, 2.0), (0.5, 0.1, 4.0))])
    ax = principal_axes(cov)
    for k, order in enumerate(((0, 1, 2), (1, 2, 0), (2, 0, 1))):
        for i in range(3):
            assert abs(abs(ax[k, i] @ rot[order[i]]) - 1) < 1e-12
        for i in (0, 1):
            assert ax[k, i, np.argmax(np.abs(ax[k, i]))] > 0
        assert abs(np.linalg.det(ax[k]) - 1) < 1e-12 and np.allclose(np.cross(ax[k, 0], ax[k, 1]), ax[k, 2], atol=1e-15)


# ------------------------------------------------------------------------------------------------ the predictor with a stub model
def test_predictor_geometry_widths_and_error_types(monkeypatch):
    from test_scene_interp_cpu import StubModel, _reference_ops
    from point_sam_amd import ops
    from point_sam_amd.geometry import mask_geometry
    from point_sam_amd.predictor import PointSAMPredictor
    log = []
    _reference_ops(monkeypatch, log)
    _reference_geometry_ops(monkeypatch, log)
    rng = np.random.default_rng(11)
    M = 700
    xyz, rgb = torch.from_numpy(rng.uniform(-1, 1, (M, 3)).astype(f32)), torch.from_numpy(rng.uniform(0, 1, (M, 3)).astype(f32))
    pred = PointSAMPredictor(StubModel())
    row = torch.from_numpy(G.words((np.linalg.norm(xyz.numpy() - xyz.numpy()[3], axis=1) < 0.4)[None]))
    with pytest.raises(RuntimeError, match="set_pointcloud"):
        pred.mask_geometry(row)
    with pytest.raises(RuntimeError, match="set_scene"):
        pred.set_crop_to_mask(row[0])
    pred.set_scene(xyz, rgb, voxel_size=0.25)
    Nw = pred.scene.num_working
    assert Nw < M and ops.mask_words(Nw) != ops.mask_words(M)
    geo = pred.mask_geometry(row)
    want = mask_geometry(xyz, row, rgb)
    assert torch.equal(geo.centroid, want.centroid) and torch.equal(geo.axes, want.axes) and torch.equal(geo.mean_rgb, want.mean_rgb)
    assert torch.equal(pred.mask_geometry(types.SimpleNamespace(bits=row)).obb_half, want.obb_half)      # anything with .bits, a Proposals among them
    assert pred.mask_geometry(row, oriented=False).axes[0].tolist() == np.eye(3).tolist()
    with pytest.raises(ValueError, match=rf"{ops.mask_words(Nw)} words.*{M} points \({ops.mask_words(M)} words\)"):      # names both widths
        pred.mask_geometry(torch.zeros(2, ops.mask_words(Nw), dtype=torch.int64))
    for bad in (row[0], row.int(), "bits", None):
        with pytest.raises(ValueError, match="masks must be"):
            pred.mask_geometry(bad)
    # set_crop_to_mask: exactly set_crop(center, radius, ...) with the mask's centroid and its radius * (1 + margin)
    calls = []
    real = pred.set_crop
    monkeypatch.setattr(pred, "set_crop", lambda *a, **k: calls.append((a, k)) or real(*a, **k))
    flat = pred.mask_geometry(row, oriented=False)
    center, radius = pred.set_crop_to_mask(row[0], margin=0.25, max_points=200)
    assert calls == [((center, radius, None, 200, None), {})] and pred.crop is not None
    assert center == tuple(flat.centroid[0].float().tolist()) and abs(radius - 1.25 * float(flat.radius[0])) < 1e-6
    assert pred.crop.center == center and pred.crop.radius == radius
    members = G.members(row[0].numpy(), M)
    assert (pred.crop.inv.numpy()[members] >= 0).all()
    assert torch.equal(pred.mask_geometry(row).centroid, want.centroid)      # under the crop the scan still answers
    # an empty mask, a wrong width, several rows, a bad margin: ValueError, and the state stays
    before = (pred.crop, pred._crop_state, pred._crop_key)
    for bad, kw, word in ((torch.zeros_like(row[0]), {}, "empty"), (row[0][:-1], {}, "words"), (torch.cat([row, row]), {}, "one mask"),
                          (row[0], {"margin": -0.1}, "margin"), (row[0], {"margin": float("nan")}, "margin"), (row[0], {"smooth": 1}, "smooth")):
        with pytest.raises(ValueError, match=word):
            pred.set_crop_to_mask(bad, **kw)
        assert (pred.crop, pred._crop_state, pred._crop_key) == before and len(calls) == 1
    pred.clear_crop()
    # after set_pointcloud: the cloud's own width, cloud `cloud` of the batch
    bx, br = torch.stack([xyz[:300], xyz[300:600]]), torch.stack([rgb[:300], rgb[300:600]])
    pred.set_pointcloud(bx, br)
    rows = torch.from_numpy(G.words(rng.random((2, 300)) < 0.3))
    assert torch.equal(pred.mask_geometry(rows, cloud=1).centroid, mask_geometry(bx[1], rows, br[1]).centroid)
    assert torch.equal(pred.mask_geometry(rows).centroid, mask_geometry(bx[0], rows, br[0]).centroid)
    with pytest.raises(ValueError, match=rf"{ops.mask_words(M)} words.*300 points"):
        pred.mask_geometry(row)
    for bad in (2, -1, True, 1.0):
        with pytest.raises(ValueError, match="cloud"):
            pred.mask_geometry(rows, cloud=bad)
    with pytest.raises(RuntimeError, match="set_scene"):
        pred.set_crop_to_mask(rows[0])


# ------------------------------------------------------------------------------------------------ the demo's routes
class FakePredictor:
    """A scene predictor as far as the demo drives it: logits = 0.5 - distance to the first prompt; proposals = two fixed masks; the geometry calls
    are logged and answered by the reference through point_sam_amd.geometry."""

    def __init__(self):
        self.log = []
        self.crop = None
        self.scene = None

    def set_pointcloud(self, xyz, rgb):
        self.xyz, self.rgb, self.scene, self.crop = xyz[0], rgb[0], None, None

    def set_scene(self, xyz, rgb, voxel_size=None, max_points=None, **kw):
        self.log.append(("set_scene", max_points, kw))
        self.xyz, self.rgb, self.scene, self.crop = xyz[0], rgb[0], True, None

    def set_crop(self, center, radius, voxel_size=None, max_points=None, **kw):
        self.log.append(("set_crop", tuple(center), radius, max_points, kw))
        inside = int(((self.xyz - torch.tensor(center, dtype=torch.float32)).norm(dim=-1) <= radius).sum())
        if inside == 0:
            raise ValueError("no point of the scan inside the ball")
        self.crop = types.SimpleNamespace(center=tuple(center), radius=radius, num_members=inside, num_working=inside)

    def clear_crop(self):
        self.crop = None

    def set_crop_to_mask(self, bits_row, margin=0.1, voxel_size=None, max_points=None, **kw):
        from point_sam_amd.geometry import mask_geometry
        self.log.append(("set_crop_to_mask", margin, max_points, kw))
        geo = mask_geometry(self.xyz, bits_row[None], None, oriented=False)
        if not bool(geo.valid[0]):
            raise ValueError("set_crop_to_mask: the mask is empty")
        center, radius = tuple(geo.centroid[0].float().tolist()), float(geo.radius[0]) * (1 + margin)
        self.set_crop(center, radius, voxel_size, max_points, **kw)
        return center, radius

    def predict_masks(self, pts, labels, prompt_mask, multimask):
        logit = 0.5 - (self.xyz - pts[0, 0]).norm(dim=-1)
        if self.crop is not None:
            logit = torch.where((self.xyz - torch.tensor(self.crop.center)).norm(dim=-1) <= self.crop.radius, logit, torch.tensor(float("-inf")))
        return logit[None, None], torch.tensor([[0.9]]), logit[None, None]

    def generate_masks(self, cfg):
        from point_sam_amd.proposals import Proposals
        n = self.xyz.shape[0]
        mask = np.stack([self.xyz[:, 0].numpy() < -0.2, self.xyz[:, 0].numpy() > 0.3])
        labels = torch.from_numpy(np.where(mask[0], 0, np.where(mask[1], 1, -1)).astype(np.int32))
        return [Proposals(n_points=n, bits=torch.from_numpy(G.words(mask)), candidate=torch.tensor([0, 3]), prompt_index=torch.tensor([0, 1]),
                          score=torch.tensor([0.95, 0.5]), area=torch.from_numpy(mask.sum(1).astype(np.int32)), stability=torch.ones(2), labels=labels)]

    def mask_geometry(self, masks, cloud=0, oriented=True):
        from point_sam_amd.geometry import mask_geometry
        self.log.append(("mask_geometry", tuple(masks.bits.shape)))
        return mask_geometry(self.xyz, masks.bits, self.rgb, oriented)


@pytest.fixture()
def demo(monkeypatch, tmp_path):
    from point_sam_amd.demo_server import DemoSession, serve
    _reference_geometry_ops(monkeypatch)
    pred = FakePredictor()
    sess = DemoSession(pred, models_dir=str(tmp_path), output_dir=str(tmp_path / "results"), device="cpu", crop_points=77)
    srv = serve(sess, "127.0.0.1", 0)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    yield srv.server_address[1], sess, pred
    srv.shutdown()


def _raw(port, path, body=None):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=30)
    c.request("POST", path, None if body is None else json.dumps(body), {"Content-Type": "application/json"})
    r = c.getresponse()
    return r.status, r.read()


def _load(port, n=120, seed=0):
    pts = np.random.default_rng(seed).uniform(-0.6, 0.6, (n, 3))
    flat = {str(i): float(v) for i, v in enumerate(pts.reshape(-1))}
    col = {str(i): float(v) for i, v in enumerate(np.random.default_rng(seed + 1).uniform(0, 1, n * 3))}
    assert _raw(port, "/sampled_pointcloud", {"points": flat, "colors": col})[0] == 200
    return pts


def test_pack_mask_is_the_librarys_layout():
    from point_sam_amd.demo_server import pack_mask
    rng = np.random.default_rng(3)
    for n in (1, 63, 64, 65, 200):
        m = rng.random(n) < 0.5
        m[-1] = True
        assert np.array_equal(pack_mask(torch.from_numpy(m)).numpy(), G.words(m[None])[0])
    full = np.ones(128, dtype=bool)
    assert pack_mask(torch.from_numpy(full)).tolist() == [-1, -1]


def test_instances_route_adds_boxes_to_segment_all(demo):
    port, sess, pred = demo
    st, body = _raw(port, "/instances", {})
    assert st == 400 and b"/instances before a point cloud" in body
    pts = _load(port)
    st_all, all_before = _raw(port, "/segment_all", {})
    st, body = _raw(port, "/instances", {"nms_thresh": 0.5})
    assert st == 200 and st_all == 200
    out = json.loads(body)
    plain = json.loads(all_before)
    assert set(out) == set(plain) | {"boxes"} and {k: out[k] for k in plain} == plain and out["num_masks"] == 2
    assert ("mask_geometry", (2, 2)) in pred.log
    assert len(out["boxes"]) == 2
    for k, box in enumerate(out["boxes"]):
        assert set(box) == {"center", "half", "axes", "aabb_lo", "aabb_hi", "count", "mean_rgb"}
        sel = pts[:, 0] < -0.2 if k == 0 else pts[:, 0] > 0.3
        assert box["count"] == int(sel.sum()) and isinstance(box["count"], int)
        assert np.array(box["axes"]).shape == (3, 3) and [len(box[n]) for n in ("center", "half", "aabb_lo", "aabb_hi", "mean_rgb")] == [3] * 5
        assert np.allclose(box["aabb_lo"], pts[sel].astype(f32).min(0)) and np.allclose(box["aabb_hi"], pts[sel].astype(f32).max(0))
        ax = np.array(box["axes"])
        q = (pts[sel] - np.array(box["center"])) @ ax.T
        assert (np.abs(q) <= np.array(box["half"]) + 1e-5).all() and abs(np.linalg.det(ax) - 1) < 1e-5
        assert all(0 <= v <= 1 for v in box["mean_rgb"])
    assert _raw(port, "/instances", {"nms_threshold": 0.5})[0] == 400 and _raw(port, "/instances", [1])[0] == 400
    # the existing route answers as before, byte for byte
    assert _raw(port, "/segment_all", {}) == (200, all_before)
    assert json.loads(all_before) == {"labels": plain["labels"], "num_masks": 2, "scores": plain["scores"]}


def test_crop_selection_route(demo):
    port, sess, pred = demo
    st, body = _raw(port, "/crop/selection", {})
    assert st == 400 and b"before a point cloud" in body
    pts = _load(port)
    st, body = _raw(port, "/crop/selection", {})
    assert st == 400 and b"before any /segment" in body and sess.crop is None
    crop_req = {"center": [0.1, 0.0, -0.1], "radius": 0.45}
    st_crop, crop_before = _raw(port, "/crop", crop_req)
    assert st_crop == 200
    assert _raw(port, "/crop/clear")[0] == 200
    click = {"prompt_point": pts[7].tolist(), "prompt_label": 1}
    st, seg = _raw(port, "/segment", click)
    seg = np.array(json.loads(seg)["seg"])
    assert st == 200 and 0 < seg.sum() < len(pts) and sess.segment_mask is not None
    for bad in ({"margin": -1}, {"margin": "big"}, {"margin": True}, {"margin": float("inf")}, {"radius": 1.0}, [0.1]):
        st, body = _raw(port, "/crop/selection", bad)
        assert st == 400 and sess.crop is None and sess.segment_mask is not None and len(sess.prompts) == 1, bad
    st, body = _raw(port, "/crop/selection", {"margin": 0.2})
    out = json.loads(body)
    assert st == 200 and out["status"] == "cropped" and set(out) == {"status", "center", "radius", "members", "working_points"}
    member = pts[seg].astype(f32).astype(np.float64)
    assert np.allclose(out["center"], member.mean(0), atol=1e-6)
    far = np.linalg.norm(member - np.array(out["center"]), axis=1).max()
    assert abs(out["radius"] - 1.2 * far) < 1e-5 and out["members"] >= int(seg.sum())
    assert sess.crop == (tuple(out["center"]), out["radius"]) and sess.prompts == [] and sess.segment_mask is None
    assert ("set_crop_to_mask", 0.2, 77, {}) in pred.log and pred.log[-1][0] == "set_crop" and pred.log[-1][3] == 77
    # from here on as after /crop: the next click runs under the same (cached) crop
    st, seg2 = _raw(port, "/segment", click)
    assert st == 200 and pred.log[-1] == ("set_crop", tuple(out["center"]), out["radius"], 77, {})
    assert set(np.nonzero(json.loads(seg2)["seg"])[0]) <= set(np.nonzero(np.linalg.norm(pts - np.array(out["center"]), axis=1) <= out["radius"] + 1e-6)[0])
    # an empty selection is a 400 and leaves the crop
    sess.segment_mask = torch.zeros(len(pts), dtype=torch.bool)
    st, body = _raw(port, "/crop/selection", {})
    assert st == 400 and b"empty" in body and sess.crop == (tuple(out["center"]), out["radius"]) and sess.segment_mask is not None
    # the existing /crop answers as before, byte for byte
    assert _raw(port, "/crop/clear")[0] == 200 and sess.crop is None
    assert _raw(port, "/crop", crop_req) == (200, crop_before)
    assert json.loads(crop_before)["status"] == "cropped"
