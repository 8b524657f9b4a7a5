"""The sizes at which the integer kernels of csrc/masks.hip and the scan of csrc/voxel_table.h (scene.hip's and crops.hip's downsample) change their
code path, read from the sources: which nms_walk_kernel<NW> instance the host code launches for which K, how many positions a thread of
paint_rank_kernel takes, how many block counts a thread of the two offsets kernels (both scan_block_offsets) scans.
The literal size lists below are what the GPU tests run; tests/test_proposals_cpu.py derives the same
lists from the parsed constants, so a new instance or a changed constant without a matching size fails without a GPU."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "point_sam_amd", "csrc")

NMS_SIZES = (4096, 4097, 4300, 8192, 8193, 8400, 12500, 16384)
NMS_SEGMENT_SIZES = (4300, 8400, 12500, 16384)      # every segment of these is held to the per-segment input conditions
NMS_SEGMENT = 4096                                  # positions per register of the walk's `removed` set: 64 lanes x 64 bits
PAINT_SIZES = (1, 1024, 1025, 2049, 4300)
VALID_SIZES = (255, 256, 257, 4300)
SCAN_SIZES = (1024 * 1024, 1024 * 1024 + 1, 2 * 1024 * 1024 + 1024 + 1)


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def _constant(src, name):
    m = re.findall(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", src)
    assert len(m) == 1, (name, m)
    return int(m[0])


def mask_constants():
    """-> dict: NMS_MAX_K, NMS_PF, RANK_THREADS, VALID_THREADS and `walks`, the launches of nms_walk_kernel in dispatch order as
    [(NW, largest KW)] (the last launch, the plain `else`, is bounded by NMS_MAX_K)."""
    src = _read("masks.hip")
    out = {n: _constant(src, n) for n in ("NMS_MAX_K", "NMS_PF", "RANK_THREADS")}
    host = src[src.index("PSAM_API int32_t psam_mask_nms("):]
    host = host[:host.index("\n}\n")]
    launches = re.findall(r"(if\s*\(KW\s*<=\s*(\d+)\)|else)\s+hipLaunchKernelGGL\(nms_walk_kernel<(\d+)>", host)
    assert len(launches) == len(re.findall(r"nms_walk_kernel<", host)) >= 1, "a launch of nms_walk_kernel this parser does not understand"
    walks = []
    for n, (cond, kw, nw) in enumerate(launches):
        last = n == len(launches) - 1
        assert (cond == "else") == last, "the last launch, and only the last, is the unconditional one"
        walks.append((int(nw), (out["NMS_MAX_K"] + 63) // 64 if last else int(kw)))
    out["walks"] = walks
    m = re.search(r"hipLaunchKernelGGL\(mask_valid_kernel, dim3\(\(unsigned\)psam_cdiv\(K, (\d+)\)\), dim3\((\d+)\)", src)
    assert m and m.group(1) == m.group(2)
    out["VALID_THREADS"] = int(m.group(1))
    return out


def scan_constants():
    """The one SCAN_THREADS of voxel_table.h under both names: scene.hip and crops.hip define none of their own."""
    for f in ("scene.hip", "crops.hip"):
        assert '#include "voxel_table.h"' in _read(f) and "SCAN_THREADS =" not in _read(f), f
    T = _constant(_read("voxel_table.h"), "SCAN_THREADS")
    return {"SCAN_THREADS": T, "CROP_SCAN_THREADS": T}


def nms_sizes(c):
    """Per instance: its last K (every word full) and, past the first instance, its first K (one live bit in the last word; odd, so the NMS_PF
    prefetch ends in a ragged group).  Per 64-word register s >= 1 of the largest instance: a K that ends about 200 positions into that register's
    segment -- the first multiple of 100 at least 200 past the segment's start."""
    sizes, first = set(), 1
    for nw, kw in c["walks"]:
        assert kw <= nw * 64, f"nms_walk_kernel<{nw}> holds {nw * 64} words, dispatched up to {kw}"
        last = min(kw * 64, c["NMS_MAX_K"])
        sizes.add(last)
        if first > 1:
            sizes.add(first)
        first = last + 1
    assert first == c["NMS_MAX_K"] + 1, "the instances must cover every K up to NMS_MAX_K"
    for s in range(1, max(nw for nw, _ in c["walks"])):
        sizes.add(-(-(s * NMS_SEGMENT + 200) // 100) * 100)
    return tuple(sorted(sizes))


def walk_of(c, K):
    """The NW the host code launches for K candidates."""
    for nw, kw in c["walks"]:
        if (K + 63) // 64 <= kw:
            return nw
    raise ValueError(K)


def paint_sizes(c):
    """per = ceil(K / RANK_THREADS) of 1 (one thread, every thread), 2 (one position past: all but 513 threads on empty spans), 3 and 5 (ragged)."""
    T = c["RANK_THREADS"]
    return (1, T, T + 1, 2 * T + 1, 4300)


def valid_sizes(c):
    T = c["VALID_THREADS"]
    return (T - 1, T, T + 1, 4300)


def scan_sizes(T):
    """per = ceil(blocks / T) of 1, 2 and 3 block counts per thread of the offsets kernels, the last with a ragged final span."""
    return (T * T, T * T + 1, 2 * T * T + T + 1)
