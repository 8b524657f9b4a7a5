"""The integer kernels of csrc/masks.hip at the sizes where they take another code path (tests/kernel_sizes.py, derived from the source by
tests/test_proposals_cpu.py): every nms_walk_kernel<NW> instance at its first and last K and part-way into every register of its suppression set,
paint_rank_kernel with 1 to 5 positions per thread, mask_valid_kernel over several workgroups, psam_mask_pack with a row stride, merge_proposals
over thousands of rows.  The candidates are intervals of a line (mask_reference.interval_family): areas and intersections are known in closed form, and
the greedy suppression of 16384 of them takes numpy half a second.  Everything is integer arithmetic or a copy: every comparison is equality."""
import functools

import numpy as np
import pytest
import torch

import kernel_sizes as KS
import mask_reference as R

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = 64


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd import ops
    return ops


@functools.lru_cache(maxsize=2)
def _family(K):
    """interval_family(K, seed=K) with its order; shared by the tests of one K and never modified (they copy what they change)."""
    N, s, e, score, valid = R.interval_family(K, seed=K)
    out = dict(K=K, N=N, s=s, e=e, score=score, valid=valid, order=R.order_of(score))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _dev_bits(s, e, N, rows=512):
    """The packed masks of the intervals, built on the host through the reference's own words() in chunks of `rows` rows (at K = 16384 the boolean
    masks would be 512 MiB at once)."""
    K = len(s)
    return torch.cat([torch.from_numpy(R.words(R.interval_masks(s, e, N, slice(r0, min(r0 + rows, K)))).view(np.int64)).cuda() for r0 in range(0, K, rows)])


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).cuda()


def _u8(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint8)).cuda()


def _assert_inter_closed_form(inter, s, e, rows=1024):
    """inter [K, K] on the device against max(0, min(e_i, e_j) - max(s_i, s_j)), in row chunks with plain torch (1 GiB at K = 16384: never downloaded)."""
    ds, de = _i32(s), _i32(e)
    K = len(s)
    assert inter.dtype == torch.int32 and tuple(inter.shape) == (K, K)
    for r0 in range(0, K, rows):
        r1 = min(r0 + rows, K)
        want = (torch.minimum(de[r0:r1, None], de[None]) - torch.maximum(ds[r0:r1, None], ds[None])).clamp_(min=0)
        assert torch.equal(inter[r0:r1], want), f"inter rows {r0} .. {r1 - 1}"


def _segments(K, kept_pos, dropped_pos):
    seg = np.arange(K) // KS.NMS_SEGMENT
    n = int(seg[-1]) + 1
    return " / ".join(map(str, np.bincount(seg[kept_pos], minlength=n))), " / ".join(map(str, np.bincount(seg[dropped_pos], minlength=n)))


def _nms_and_paint(ops, fam, bits, inter, area, iou_thr, tag):
    """Device NMS + paint against the interval reference; prints the reference's kept / suppressed counts (per segment of 4096 positions)."""
    K, N, s, e, order, valid = (fam[k] for k in ("K", "N", "s", "e", "order", "valid"))
    want_keep, sup = R.nms_intervals(s, e, order, valid, iou_thr)
    want_labels = R.paint_intervals(s, e, order, want_keep, N)
    d_order = _i32(order)
    keep = ops.mask_nms(d_order, _u8(valid), area, inter, iou_thr)
    labels = ops.mask_paint(bits, d_order, keep, N)
    got_keep = keep.cpu().numpy().astype(bool)
    kk, dd = _segments(K, want_keep[order], sup >= 0)
    print(f"{tag}: K={K} KW={(K + 63) // 64}: reference keeps {int(want_keep.sum())} ({kk}), suppresses {int((sup >= 0).sum())} ({dd}), "
          f"invalid {int((~valid).sum())}; device keeps {int(got_keep.sum())}")
    assert keep.dtype == torch.uint8 and int(keep.max()) <= 1
    wrong = np.nonzero(got_keep[order] != want_keep[order])[0]
    assert wrong.size == 0, f"{tag}: {wrong.size} positions differ, the first at {wrong[:8]} (segment {wrong[0] // KS.NMS_SEGMENT})"
    assert np.array_equal(labels.cpu().numpy(), want_labels), tag
    return want_keep, sup


# ------------------------------------------------------------------------------------------------ a. every walk instance
@pytest.mark.parametrize("K", KS.NMS_SIZES)
def test_nms_and_paint_at_every_walk_instance(ops, K):
    """mask_intersections -> mask_nms -> mask_paint at IoU 0.5.  The input conditions (enough kept and suppressed candidates in every segment,
    suppressors from segment 0 and from later segments) are asserted on the reference in tests/test_proposals_cpu.py for these K and this seed."""
    fam = _family(K)
    s, e = fam["s"], fam["e"]
    bits = _dev_bits(s, e, fam["N"])
    assert tuple(bits.shape) == (K, ops.mask_words(fam["N"]))
    inter = ops.mask_intersections(bits)
    _assert_inter_closed_form(inter, s, e)
    area = inter.diagonal().contiguous()
    assert np.array_equal(area.cpu().numpy(), e - s)
    want_keep, sup = _nms_and_paint(ops, fam, bits, inter, area, 0.5, "walk")
    assert want_keep.sum() >= K / 8 and (sup >= 0).sum() >= K / 8


# ------------------------------------------------------------------------------------------------ b. the thresholds' ends
def test_nms_thresholds_one_and_zero(ops):
    """K = 4300.  At 1.0 nothing overlaps more than completely: only validity decides.  At 0.0 any shared point suppresses: the kept intervals are
    pairwise disjoint."""
    fam = _family(4300)
    bits = _dev_bits(fam["s"], fam["e"], fam["N"])
    inter = ops.mask_intersections(bits)
    area = inter.diagonal().contiguous()
    keep1, sup1 = _nms_and_paint(ops, fam, bits, inter, area, 1.0, "thr 1.0")
    assert np.array_equal(keep1, fam["valid"]) and (sup1 < 0).all()
    keep0, sup0 = _nms_and_paint(ops, fam, bits, inter, area, 0.0, "thr 0.0")
    k = np.nonzero(keep0)[0]
    k = k[np.argsort(fam["s"][k])]
    assert len(k) >= 64 and (fam["e"][k][:-1] <= fam["s"][k][1:]).all() and (sup0 >= 0).sum() >= 4300 / 2


# ------------------------------------------------------------------------------------------------ c. corrupt entries of `order`
def test_nms_skips_corrupt_order_entries_and_stays_inside_keep(ops):
    """K = 4300, 20 entries of `order` replaced by -1, K and 2^31 - 1, in both segments and at half of them in the place of a candidate the clean
    run keeps.  The candidates still present must match a reference that skips the corrupt positions; the entries of the absent ones are
    unspecified; psam_mask_nms, called through ctypes, writes nothing outside keep[0 : K] (guard bytes on both sides)."""
    from point_sam_amd import _lib
    fam = _family(4300)
    K, N, s, e, valid = fam["K"], fam["N"], fam["s"], fam["e"], fam["valid"]
    clean_keep, _ = R.nms_intervals(s, e, fam["order"], valid, 0.5)
    rng = np.random.default_rng(12)
    kept_pos = np.nonzero(clean_keep[fam["order"]])[0]
    pos = np.concatenate([[0], rng.choice(kept_pos[(kept_pos > 0) & (kept_pos < 4096)], 7, replace=False), rng.choice(kept_pos[kept_pos >= 4096], 3, replace=False),
                          rng.choice(np.arange(1, 4096), 5, replace=False), rng.choice(np.arange(4096, K), 4, replace=False)])
    pos = np.unique(pos)
    assert 16 <= len(pos) <= 20 and (pos < 4096).sum() >= 8 and (pos >= 4096).sum() >= 4
    order = fam["order"].astype(np.int64).copy()
    absent = order[pos].copy()
    order[pos] = np.resize(np.array([-1, K, 2 ** 31 - 1], dtype=np.int64), len(pos))
    present = np.setdiff1d(np.arange(K), absent)
    want_keep, sup = R.nms_intervals(s, e, order, valid, 0.5)
    assert not want_keep[absent].any() and (want_keep[present] != clean_keep[present]).any()      # the corruption changes decisions

    bits = _dev_bits(s, e, N)
    inter = ops.mask_intersections(bits)
    area = inter.diagonal().contiguous()
    d_order, d_valid = _i32(order), _u8(valid)
    L = _lib.load()
    nbytes = L.psam_mask_nms_workspace_bytes(K)
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device="cuda")
    buf = torch.full((K + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    st = L.psam_mask_nms(d_order.data_ptr(), d_valid.data_ptr(), area.data_ptr(), inter.data_ptr(), K, 0.5, buf.data_ptr() + GUARD, ws.data_ptr(),
                         ws.numel() * 8, torch.cuda.current_stream().cuda_stream)
    assert st == 0, L.psam_last_error_string()
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:GUARD] == 0xA5).all() and (got[GUARD + K:] == 0xA5).all(), "psam_mask_nms wrote outside keep[0 : K]"
    got = got[GUARD:GUARD + K]
    print(f"corrupt order: {len(pos)} positions {pos.tolist()}; reference keeps {int(want_keep.sum())}, suppresses {int((sup >= 0).sum())}")
    assert np.array_equal(got[present], want_keep[present].astype(np.uint8))
    # the binding agrees, and the paint skips the same positions (keep of the absent candidates given as 0)
    keep = ops.mask_nms(d_order, d_valid, area, inter, 0.5)
    assert np.array_equal(keep.cpu().numpy()[present], want_keep[present].astype(np.uint8))
    labels = ops.mask_paint(bits, d_order, _u8(want_keep), N)
    assert np.array_equal(labels.cpu().numpy(), R.paint_intervals(s, e, order, want_keep, N))


# ------------------------------------------------------------------------------------------------ d. paint
@pytest.mark.parametrize("K", KS.PAINT_SIZES)
def test_paint_with_one_to_five_positions_per_rank_thread(ops, K):
    """per = ceil(K / 1024) = 1, 1, 2, 3, 5 (at 1025 all but 513 threads have an empty span).  `keep` is random, not an NMS result: kept masks
    overlap, so the first in `order` must win a point; the candidate at the last position is kept and moved over a point no other kept mask covers.  Then nothing kept (every label -1), and a kept count that is no multiple of 4 (the paint
    loop's group of four words)."""
    N, s, e, score, _ = R.interval_family(K, seed=1000 + K)
    order = R.order_of(score)
    rng = np.random.default_rng(K)
    keep = rng.random(K) < 0.3
    last = order[-1]                                      # the last position of the last non-empty span: kept, and it must own a point
    keep[last] = False
    if (keep.sum() + 1) % 4 == 0:
        keep[np.nonzero(~keep & (np.arange(K) != last))[0][0]] = True
    u = int(np.nonzero(R.paint_intervals(s, e, order, keep, N) < 0)[0][0])      # a point no other kept mask covers
    s[last] = min(u, N - 4)
    e[last] = s[last] + 4
    keep[last] = True
    assert keep.sum() % 4 != 0
    bits, d_order = _dev_bits(s, e, N), _i32(order)
    want = R.paint_intervals(s, e, order, keep, N)
    assert want[u] == keep.sum() - 1
    print(f"paint K={K}: per {-(-K // 1024)}, kept {int(keep.sum())}, unlabelled points {int((want < 0).sum())} of {N}")
    assert K < 1024 or len(np.unique(want)) >= 64         # many ranks win some point
    got = ops.mask_paint(bits, d_order, _u8(keep), N)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    none = ops.mask_paint(bits, d_order, torch.zeros(K, dtype=torch.uint8, device="cuda"), N)
    assert tuple(none.shape) == (N,) and bool((none == -1).all())
    every = ops.mask_paint(bits, d_order, torch.ones(K, dtype=torch.uint8, device="cuda"), N)
    assert np.array_equal(every.cpu().numpy(), R.paint_intervals(s, e, order, np.ones(K, dtype=bool), N))


# ------------------------------------------------------------------------------------------------ e. validity
@pytest.mark.parametrize("K", KS.VALID_SIZES)
def test_valid_over_several_workgroups_with_every_equality(ops, K):
    """One short of, exactly and one past a workgroup of 256, and 17 workgroups.  N = 4096, at least 25 points, under 0.75 N = 3072 exactly, score
    cut 0.6 (fp32), stability 0.75 (exact in fp32).  The special rows sit at both ends and around candidate 256."""
    N, min_points, frac, stab = 4096, 25, 0.75, 0.75
    cut = f32(0.6)
    rng = np.random.default_rng(K)
    area = rng.integers(0, N + 1, K)
    lo = np.minimum(area + rng.integers(0, 200, K), N)
    hi = np.maximum(area - rng.integers(0, 200, K), 0)
    score = rng.random(K, dtype=f32)
    special = [((25, 25, 25, cut), True),                                     # area at min_points, score at the cut: both pass (>=)
               ((24, 24, 24, 0.9), False),
               ((3072, 3072, 3072, 0.9), False),                              # area == max_area_frac * N: "under" is strict
               ((3071, 3071, 3071, 0.9), True),
               ((100, 100, 100, np.nextafter(cut, f32(0))), False),
               ((100, 100, 100, np.nan), False),
               ((100, 0, 0, 0.9), False),                                     # area_lo == 0
               ((350, 300, 400, 0.9), True),                                  # hi == stab * lo exactly
               ((350, 299, 400, 0.9), False),
               ((0, 0, 0, 1.0), False)]
    where = np.unique(np.concatenate([np.arange(10), np.arange(K - 10, K), np.arange(250, 262)]))
    where = where[where < K]
    expect = {}
    for n, k in enumerate(where):
        (area[k], hi[k], lo[k], score[k]), expect[int(k)] = special[n % len(special)]
    want = R.validity(area, hi, lo, score, N, min_points, frac, float(cut), stab)
    for k, ok in expect.items():
        assert want[k] == ok, (k, area[k], hi[k], lo[k], score[k])
    assert K - 1 in expect and 0.05 < want.mean() < 0.95
    got = ops.mask_valid(_i32(area), _i32(hi), _i32(lo), torch.from_numpy(score).cuda(), N, min_points, frac, float(cut), stab)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (K,)
    assert np.array_equal(got.cpu().numpy(), want.astype(np.uint8))


# ------------------------------------------------------------------------------------------------ f. pack with a row stride
def test_pack_with_a_row_stride_and_a_ragged_second_trip(ops):
    """psam_mask_pack through ctypes with ld = N + 5 and N = 64 * 65 + 3: W = 66 words, so wave 0 makes a second trip whose group of four words has
    two past the row's end.  The 5 pad columns of every row hold +inf: they lie in the last word's range of the row before and must never count."""
    from point_sam_amd import _lib
    K, N, pad = 7, 64 * 65 + 3, 5
    W = ops.mask_words(N)
    assert W == 66
    thr, off = f32(0.25), f32(0.5)
    rng = np.random.default_rng(66)
    special = np.array([thr, thr + off, thr - off, np.nextafter(thr, f32(1)), np.nextafter(thr, f32(-1)), -0.0, np.nan, np.inf, -np.inf], dtype=f32)
    view = np.where(rng.random((K, N)) < 0.1, rng.choice(special, (K, N)), rng.normal(0.25, 1.0, (K, N))).astype(f32)
    view[0] = -1.0                                        # an empty row: its pad columns would be its only points
    view[1] = 1.0                                         # a full row
    view[2, -3:] = (1.0, -1.0, 1.0)                       # the three live bits of the last word
    full = np.full((K, N + pad), np.inf, dtype=f32)       # the [K, N] view of this is the input
    full[:, :N] = view
    m, area, hi, lo = R.pack(view, thr, off)
    assert area[0] == 0 and area[1] == N
    dev = torch.from_numpy(full).cuda()
    bits = torch.full((K, W), -1, dtype=torch.int64, device="cuda")
    out = [torch.full((K,), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
    L = _lib.load()
    st = L.psam_mask_pack(dev.data_ptr(), N + pad, K, N, float(thr), float(off), 0, bits.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                          torch.cuda.current_stream().cuda_stream)
    assert st == 0, L.psam_last_error_string()
    torch.cuda.synchronize()
    got = bits.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, R.words(m))
    assert (got[:, -1] >> np.uint64(N % 64)).max() == 0, "a pad column was packed"
    for t, w in zip(out, (area, hi, lo)):
        assert np.array_equal(t.cpu().numpy(), w.astype(np.int32))


# ------------------------------------------------------------------------------------------------ g. merge_proposals
def test_merge_proposals_of_4300_rows_in_three_layers(ops):
    """The interval family of K = 4300 cut into the layers base (-1), crop 0 and crop 1, every row valid.  128 rows of the later layers are twins of
    base rows (the same interval, the same score): the stable order puts the base row first, and the twin goes (IoU 1).  64 more share a score with
    a base row but not its interval.  Kept rows and their order, crop_index, candidate, score, area and labels against the interval reference."""
    from point_sam_amd.proposals import Proposals, merge_proposals
    fam = _family(4300)
    K, N = fam["K"], fam["N"]
    s, e, score = fam["s"].copy(), fam["e"].copy(), fam["score"].copy()
    cuts = (0, 1500, 3000, K)
    first_candidate = (0, 10000, 20000)
    rng = np.random.default_rng(43)
    base = rng.choice(1500, 192, replace=False)
    later = 1500 + rng.choice(K - 1500, 192, replace=False)
    score[later] = score[base]
    s[later[:128]], e[later[:128]] = s[base[:128]], e[base[:128]]
    valid = np.ones(K, dtype=bool)
    order = R.order_of(score)
    where = np.empty(K, dtype=np.int64)
    where[order] = np.arange(K)
    assert (where[base] < where[later]).all()                                       # the reference's order: the earlier layer first on a tie
    keep, sup = R.nms_intervals(s, e, order, valid, 0.5)
    assert not keep[later[:128]].any() and keep[base[:128]].sum() >= 16 and keep[later[128:]].sum() >= 8 and (later >= 3000).sum() >= 32
    sel = order[keep[order]]
    bits = _dev_bits(s, e, N)
    layers, layer_of, cand_of = [], np.empty(K, dtype=np.int64), np.empty(K, dtype=np.int64)
    for n in range(3):
        a, b = cuts[n], cuts[n + 1]
        cand = torch.arange(first_candidate[n], first_candidate[n] + b - a, dtype=torch.int64, device="cuda")
        layer_of[a:b], cand_of[a:b] = n - 1, np.arange(first_candidate[n], first_candidate[n] + b - a)
        layers.append((n - 1, Proposals(N, bits[a:b], cand, cand // 3, torch.from_numpy(score[a:b]).cuda(), _i32((e - s)[a:b]), torch.ones(b - a, device="cuda"),
                                        torch.full((N,), -1, dtype=torch.int32, device="cuda"))))
    out = merge_proposals(layers, N, 0.5)
    print(f"merge: {K} rows in layers of {[b - a for a, b in zip(cuts, cuts[1:])]}: reference keeps {len(sel)}, suppresses {int((sup >= 0).sum())}; device keeps {len(out)}")
    assert len(out) == len(sel)
    assert np.array_equal(out.candidate.cpu().numpy(), cand_of[sel])
    assert np.array_equal(out.crop_index.cpu().numpy(), layer_of[sel]) and set(layer_of[sel]) == {-1, 0, 1}
    assert np.array_equal(out.prompt_index.cpu().numpy(), cand_of[sel] // 3)
    assert np.array_equal(out.score.cpu().numpy(), score[sel]) and np.array_equal(out.area.cpu().numpy(), (e - s)[sel])
    assert np.array_equal(out.bits.cpu().numpy().view(np.uint64), R.words(R.interval_masks(s, e, N))[sel])
    assert np.array_equal(out.labels.cpu().numpy(), R.paint_intervals(s, e, order, keep, N))
