"""Plain numpy reference of the mask-proposal post-processing (pack, intersections, validity, greedy NMS, paint): loops over boolean arrays,
written from the definitions in include/pointsam_hip.h and independent of the package.  The tests compare the kernels against THIS."""
import numpy as np

f32 = np.float32


def pack(logits, thr, off):
    """logits [K, N] f32 -> (masks [K, N] bool, area, area_hi, area_lo [K] int64).  Thresholds rounded to fp32; NaN compares false."""
    logits = np.asarray(logits, dtype=f32)
    thr, off = f32(thr), f32(off)
    hi, lo = f32(thr + off), f32(thr - off)
    with np.errstate(invalid="ignore"):
        m = logits > thr
        return m, m.sum(1), (logits > hi).sum(1), (logits > lo).sum(1)


def words(masks):
    """[K, N] bool -> [K, ceil(N / 64)] uint64: bit n % 64 of word n / 64 is point n, tail bits zero."""
    K, N = masks.shape
    W = (N + 63) // 64
    padded = np.zeros((K, W * 64), dtype=np.uint8)
    padded[:, :N] = masks
    return np.packbits(padded, axis=1, bitorder="little").view("<u8").reshape(K, W)


def unwords(w, N):
    """Inverse of words()."""
    w = np.ascontiguousarray(w).view("<u8")
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little")[:, :N].astype(bool)


def intersections(a, b, exact_int=True):
    """[Ka, N], [Kb, N] bool -> [Ka, Kb] int64.  exact_int False: the 0/1 matmul in fp32 (BLAS) -- every partial sum is an integer below 2^24
    for N <= 2^24, so it is exact too, and it is the only form that finishes for thousands of masks."""
    if exact_int:
        return a.astype(np.int64) @ b.astype(np.int64).T
    assert a.shape[1] <= 1 << 24
    return (a.astype(f32) @ b.astype(f32).T).astype(np.int64)


def validity(area, area_hi, area_lo, score, N, min_points, max_area_frac, pred_iou_thr, stab_thr):
    out = np.zeros(len(area), dtype=bool)
    for k in range(len(area)):
        s = f32(score[k])
        out[k] = (int(area[k]) >= min_points and float(area[k]) < float(f32(max_area_frac)) * N and bool(s >= f32(pred_iou_thr))
                  and int(area_lo[k]) > 0 and float(area_hi[k]) >= float(f32(stab_thr)) * float(area_lo[k]))
    return out


def order_of(score):
    """Stable descending sort: ties keep the lower candidate index first (NaN scores are invalid, their place does not matter)."""
    return np.argsort(-np.asarray(score, dtype=f32), kind="stable")


def nms(order, valid, area, inter, iou_thr):
    thr = float(f32(iou_thr))
    keep = np.zeros(len(order), dtype=bool)
    kept = []
    for i in order:
        if not valid[i]:
            continue
        if any(float(inter[i, j]) > thr * float(int(area[i]) + int(area[j]) - int(inter[i, j])) for j in kept):
            continue
        keep[i] = True
        kept.append(i)
    return keep


def paint(masks, order, keep):
    labels = np.full(masks.shape[1], -1, dtype=np.int32)
    rank = 0
    for i in order:
        if keep[i]:
            labels[(labels < 0) & masks[i]] = rank
            rank += 1
    return labels


def proposals(logits, score, N, thr, off, min_points, max_area_frac, pred_iou_thr, stab_thr, nms_thr):
    """The whole post-processing of one cloud -> dict of everything the kernels produce."""
    m, area, hi, lo = pack(logits, thr, off)
    valid = validity(area, hi, lo, score, N, min_points, max_area_frac, pred_iou_thr, stab_thr)
    order = order_of(score)
    inter = intersections(m, m)
    keep = nms(order, valid, area, inter, nms_thr)
    return dict(masks=m, area=area, area_hi=hi, area_lo=lo, valid=valid, order=order, inter=inter, keep=keep, labels=paint(m, order, keep),
                candidate=np.array([i for i in order if keep[i]], dtype=np.int64))


# ------------------------------------------------------------------------------------------------ intervals: overlaps in closed form
# Thousands of candidates need no [K, N] booleans and no K x K matrix on the host when every mask is an interval of a line: area = e - s and
# inter(i, j) = max(0, min(e_i, e_j) - max(s_i, s_j)).  nms() and paint() above stay the definition; the two functions below apply the same rules to
# the closed form (tests/test_proposals_cpu.py holds them to nms() / paint() on the explicit masks).
def interval_family(K, seed):
    """-> (N, s, e [K] int64, score [K] f32, valid [K] bool): candidate i is [s_i, e_i) on a line of N = 2 K + 37 points, its length uniform in
    4 .. 96, its start uniform over the positions that fit, its score uniform in [0, 1), about one row in ten invalid."""
    rng = np.random.default_rng(seed)
    N = 2 * K + 37
    length = rng.integers(4, min(96, N) + 1, K)          # 96 fits every line of K >= 30 candidates
    s = rng.integers(0, N - length + 1)
    score = rng.random(K, dtype=f32)
    valid = rng.random(K) >= 0.1
    return N, s.astype(np.int64), (s + length).astype(np.int64), score, valid


def interval_masks(s, e, N, rows=None):
    """The explicit [k, N] boolean masks of the intervals (of the rows `rows`, a slice: the whole family can be gigabytes)."""
    rows = slice(None) if rows is None else rows
    n = np.arange(N, dtype=np.int64)[None]
    return (n >= np.asarray(s)[rows, None]) & (n < np.asarray(e)[rows, None])


def nms_intervals(s, e, order, valid, iou_thr):
    """Greedy NMS with the decision rule of nms(), vectorised over the kept list.  -> (keep [K] bool by candidate, suppressor [K] int64 by POSITION in
    `order`: the position of the first kept candidate that suppresses the one at this position, -1 for a kept or an invalid one).  An entry of
    `order` outside [0, K) is skipped: it is no candidate."""
    s, e = np.asarray(s, dtype=np.int64), np.asarray(e, dtype=np.int64)
    K = len(s)
    thr = float(f32(iou_thr))
    keep = np.zeros(K, dtype=bool)
    suppressor = np.full(len(order), -1, dtype=np.int64)
    ks, ke, kpos = np.empty(K, dtype=np.int64), np.empty(K, dtype=np.int64), np.empty(K, dtype=np.int64)
    n = 0
    for p, i in enumerate(order):
        i = int(i)
        if not 0 <= i < K or not valid[i]:
            continue
        inter = np.maximum(np.minimum(e[i], ke[:n]) - np.maximum(s[i], ks[:n]), 0)
        union = (e[i] - s[i]) + (ke[:n] - ks[:n]) - inter
        hit = inter.astype(np.float64) > thr * union.astype(np.float64)
        if hit.any():
            suppressor[p] = kpos[np.argmax(hit)]
            continue
        keep[i] = True
        ks[n], ke[n], kpos[n] = s[i], e[i], p
        n += 1
    return keep, suppressor


def paint_intervals(s, e, order, keep, N):
    """paint() for intervals.  Entries of `order` outside [0, K) are skipped."""
    labels = np.full(N, -1, dtype=np.int32)
    rank = 0
    for i in order:
        i = int(i)
        if 0 <= i < len(keep) and keep[i]:
            part = labels[s[i]:e[i]]
            part[part < 0] = rank
            rank += 1
    return labels
