"""Builds csrc/libpointsam_hip.so for gfx950 with hipcc (cross-compiles without a GPU).

    python -m point_sam_amd.build [--force]

The library is built IN-TREE so that it travels with the repository snapshot to the GPU box.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB = os.path.join(CSRC, "libpointsam_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"
COMMON = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wall", "-Wno-unused-function"]
# (source, extra flags).  The tokenizer must not contract a*b+c into fma: FPS / kNN indices are bit-exact
# against the oracle's fp32 arithmetic (oracle/tokenizer_oracle.c is built with -ffp-contract=off too).
# PSAM_BUILD_EXPERIMENTS=1: also build the measured-and-rejected paths under csrc/experiments/ (the unit-ring GEMM gemm_f16x3q.hip, the persistent GEMMs gemm_f16x3s.hip (stream-K) and gemm_f16x3c.hip (continuous), the one-launch token side twoway.hip, the
# forked two-way decoder, the 128x512 row-LayerNorm GEMM tile) -- off by default: they are not on the product path, and their objects, exports, ISA
# lint and tests cost every build and every test run (tests that need them skip unless the library was built with them).
EXPERIMENTS = os.environ.get("PSAM_BUILD_EXPERIMENTS", "0") == "1"
SOURCES = [
    ("tokenizer.hip", ["-ffp-contract=off"]),
    ("gemm.hip", []),
    ("gemm_split.hip", []),
    ("gemm_f16x3p.hip", []),
    ("gemm_f16x3pp.hip", []),
    ("patch_rowln.hip", []),
    ("attention.hip", []),
    ("rowops.hip", []),
    ("blocks.hip", []),
    ("masks.hip", []),
    ("scene.hip", ["-ffp-contract=off"]),      # voxel cells: floorf((x - origin) * inv_h) with every operation rounded on its own
    ("regions.hip", ["-ffp-contract=off"]),    # the same cells as scene.hip (csrc/voxel_cell.h)
    ("crops.hip", ["-ffp-contract=off"]),      # membership, normalised coordinates and cells of a ball of the scan: every fp32 operation rounded on its own
    ("scene_interp.hip", ["-ffp-contract=off"]),      # 3-NN blend over the voxel neighbourhood: distances, weights and the blend rounded one operation at a time
    # radius 3-NN into another cloud: the cells of scene.hip, the distances and weights of scene_interp.hip.  No SLP vectorisation, as for geometry.hip
    # below: it packs two rows of the pose into a v_pk_mul_f32 that broadcasts one half of a register pair.
    ("transfer.hip", ["-ffp-contract=off", "-fno-slp-vectorize"]),
    # one ICP step on transfer.hip's index: the same candidates bit for bit (csrc/transfer_index.h), so the same flags, for the same reasons.
    ("align.hip", ["-ffp-contract=off", "-fno-slp-vectorize"]),
    # one point-to-plane ICP step: align.hip's pair bit for bit (the same shared headers), so align.hip's flags.
    ("align_plane.hip", ["-ffp-contract=off", "-fno-slp-vectorize"]),
    # the score of a pose search: align.hip's posed coordinate, cell and candidates for P poses at once, so align.hip's flags.
    ("align_score.hip", ["-ffp-contract=off", "-fno-slp-vectorize"]),
    # camera views: the projection's fp32 operations rounded one at a time; the pose is transfer.hip's (csrc/rigid_pose.h), and so is the reason for
    # leaving SLP vectorisation off.
    ("views.hip", ["-ffp-contract=off", "-fno-slp-vectorize"]),
    # RGB-D frames: unprojection, normalisation and the keys' depth rounded one operation at a time; the pose arithmetic is views.hip's.
    ("frames.hip", ["-ffp-contract=off", "-fno-slp-vectorize"]),
    # label fusion: the projection and the visibility test are views.hip's (csrc/view_camera.h), and so are the flags.
    ("fusion.hip", ["-ffp-contract=off", "-fno-slp-vectorize"]),
    # instance geometry: the extents' fp32 operations rounded one at a time, the moments' fp64 terms exact.  No SLP vectorisation: it packs the three
    # projections into v_pk_mul_f32 / v_pk_add_f32 that broadcast one half of a register pair, the form isa_lint.py refuses; the kernels are gather-bound.
    ("geometry.hip", ["-ffp-contract=off", "-fno-slp-vectorize"]),
    # normals: the scatter matrix is integer, the fp64 eigen-solve and the sign test rounded one operation at a time; flags as for geometry.hip.
    ("normals.hip", ["-ffp-contract=off", "-fno-slp-vectorize"]),
    # superpoints: the join rule's fp64 dot product is (x x' + y y') + z z' with nothing contracted, so that a host reference decides every edge alike.
    ("superpoints.hip", ["-ffp-contract=off", "-fno-slp-vectorize"]),
    # scan maps: scene.hip's cells of the pose of csrc/rigid_pose.h, and an fp64 mean rounded one operation at a time; flags as for transfer.hip.
    ("scanmap.hip", ["-ffp-contract=off", "-fno-slp-vectorize"]),
    # scan map carving: scanmap.hip's point, pose and cell bit for bit (csrc/map_block.h), so scanmap.hip's flags; the walk itself is integer.
    ("carve.hip", ["-ffp-contract=off", "-fno-slp-vectorize"]),
    # scan map tracking, point to point and point to plane: scanmap.hip's point, cell and voxel mean (csrc/map_block.h) and the distance and sums of
    # align.hip / align_plane.hip, so the flags of all three.
    ("track.hip", ["-ffp-contract=off", "-fno-slp-vectorize"]),
    # scan map normals: scanmap.hip's voxel mean and fixed point (csrc/map_block.h) and normals.hip's eigen-solve (csrc/normal_eigen.h), so the flags of both.
    ("map_normals.hip", ["-ffp-contract=off", "-fno-slp-vectorize"]),
    # scan map relocalisation: track.hip's posed coordinate, cell, voxel mean and distance for P poses at once (csrc/map_block.h), so track.hip's flags.
    ("track_score.hip", ["-ffp-contract=off", "-fno-slp-vectorize"]),
    # scan map views: carve.hip's integer walk from the eye's cell, scanmap.hip's voxel mean (csrc/map_block.h) and views.hip's depth
    # (csrc/view_camera.h), so the flags of all three.
    ("map_view.hip", ["-ffp-contract=off", "-fno-slp-vectorize"]),
    ("error.cpp", ["-x", "hip"]),
] + ([("experiments/gemm_f16x3q.hip", ["-I" + CSRC]), ("experiments/gemm_f16x3s.hip", ["-I" + CSRC]), ("experiments/gemm_f16x3c.hip", ["-I" + CSRC]),
        ("experiments/twoway.hip", ["-I" + CSRC])] if EXPERIMENTS else [])
if EXPERIMENTS:
    COMMON = COMMON + ["-DPSAM_BUILD_EXPERIMENTS"]
FLAGS_STAMP = os.path.join(CSRC, ".build_flags")
# measurement aid of bench.py (matrix-pipe ceiling probe): its own small library, not part of the product ABI
PROBE_SRC = os.path.join(CSRC, "probe", "mfma_probe.hip")
PROBE_LIB = os.path.join(CSRC, "probe", "libpsam_probe.so")


def _stale(out, deps):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)


def build_library(force: bool = False, verbose: bool = False) -> str:
    hdrs = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith(".h")]   # every header: an edit to any rebuilds all objects
    hdrs.append(os.path.join(os.path.dirname(os.path.dirname(CSRC)), "include", "pointsam_hip.h"))   # the public ABI header is part of every translation unit (common.h)
    flags = " ".join(COMMON)
    # another flag set than the objects were built with (experiments on / off): every object is stale.  No stamp = a tree built before the stamp
    # existed, or a snapshot that dropped it: the default flags are assumed (the GPU box must not spend minutes rebuilding a library that travelled).
    if (open(FLAGS_STAMP).read() != flags) if os.path.exists(FLAGS_STAMP) else EXPERIMENTS:
        force = True
    jobs = []
    for src, extra in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(CSRC, os.path.splitext(src)[0] + ".o")
        if force or _stale(o, [s, os.path.abspath(__file__)] + hdrs):
            jobs.append([HIPCC] + COMMON + extra + ["-c", s, "-o", o])
    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stderr)
        return r.stderr
    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, jobs))
    objs = [os.path.join(CSRC, os.path.splitext(s)[0] + ".o") for s, _ in SOURCES]
    if force or jobs or _stale(LIB, objs):
        # Link under a temporary name and move it into place only once the ISA lint has passed: a library that could not be linted (llvm-objdump
        # missing, lint crashed) or that failed it never sits at LIB, where the next build_library() would find it "fresh" and return it unchecked.
        tmp = LIB + ".unlinted"
        run([HIPCC, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", tmp] + objs)
        # no packed-FP32 instruction with a non-uniform op_sel may ship: wrong lanes 48-63 beside another stream's GEMM workgroups (isa_lint.py)
        try:
            from . import isa_lint
        except ImportError:      # run as a script
            sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
            import isa_lint
        bad = isa_lint.lint(tmp)
        if bad:
            os.replace(tmp, LIB + ".rejected")
            raise RuntimeError("libpointsam_hip.so contains packed-FP32 instructions with a non-uniform op_sel (see point_sam_amd/isa_lint.py):\n" +
                               "\n".join(f"  {k}: {i}" for k, i in bad))
        os.replace(tmp, LIB)
        with open(FLAGS_STAMP, "w") as f:
            f.write(flags)
    if force or _stale(PROBE_LIB, [PROBE_SRC]):
        run([HIPCC, "--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-shared", "-o", PROBE_LIB, PROBE_SRC])
    return LIB


if __name__ == "__main__":
    print(build_library(force="--force" in sys.argv, verbose=True))
