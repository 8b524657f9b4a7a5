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
