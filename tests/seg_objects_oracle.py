"""numpy / scipy restatement of the object-level contract (include/cae_hip.h, "Objects of a label plane"); no tests here.
Written from the contract's words and the reference's procedure (test_cae_classifier.py:97-157, 267-370), not from the
library's code: objects by scipy.ndimage.label with the full 3x3 structure (one call per distinct value for by_value),
boxes from find_objects widened by one pixel and clipped to the extent, the cover by adding 1 over every box -- and the
object-level record and histogram the way the reference makes them: the box regions of target and logits are cut out
and CONCATENATED, and the concatenation goes through the plain restatements of cae_seg_predict
(tests/test_seg_predict.py: oracle; for several classes `record` below, which states the contract's argmax for NaN
logits too and equals that oracle wherever no logit is NaN) and of the ROC histogram (tests/seg_roc_oracle.py).  Nothing
here weights by the cover: that the two agree is what the tests check.
"""
import numpy as np
from scipy import ndimage

import seg_roc_oracle as RO
from test_seg_predict import oracle as predict_oracle

EIGHT = np.ones((3, 3), dtype=np.int64)


def record(logits, target, t, top_k):
    """logits (N,C,K) float32, target (N,K) uint8 -> (N,6) int64, the counts of cae_seg_predict by the contract's words
    (include/cae_hip.h, "Prediction from the head's logits").  One class: test_seg_predict's oracle (logit > t is false
    for NaN in numpy as in the kernel).  Several: the class is the lowest index of the largest logit where "larger" is the
    strict fp32 compare, so a NaN never wins and a NaN at class 0 is never beaten -- numpy's argmax, which that oracle
    uses, returns the first NaN instead; the rank of the target's logit counts l_j > l_t and l_j == l_t for j < t, both
    false against NaN."""
    n, c, k = logits.shape
    if c == 1:
        return predict_oracle(logits, target, t, top_k)[1]
    best, idx = logits[:, 0].copy(), np.zeros((n, k), dtype=np.int64)
    for j in range(1, c):
        wins = logits[:, j] > best
        best, idx = np.where(wins, logits[:, j], best), np.where(wins, j, idx)
    tgt = target.astype(np.int64)
    lt = np.take_along_axis(logits, np.minimum(tgt, c - 1)[:, None, :], axis=1)
    below = np.arange(c)[None, :, None] < tgt[:, None, :]
    rank = (logits > lt).sum(1) + ((logits == lt) & below).sum(1)
    tp = (idx == tgt).sum(1)
    top = ((tgt < c) & (rank < min(top_k, c))).sum(1)
    full = np.full(n, k)
    return np.stack([tp, 0 * tp, full - tp, full - tp, full, top], axis=1).astype(np.int64)


def clamp_extent(extent, i, h, w):
    if extent is None:
        return h, w
    return min(max(int(extent[i][0]), 0), h), min(max(int(extent[i][1]), 0), w)


def plane_objects(plane, rows, cols, by_value):
    """(H,W) uint8 -> (labels (H,W) int64 in canonical form, list of boxes (y0, y1, x0, x1), end exclusive)"""
    h, w = plane.shape
    seen = np.zeros((h, w), dtype=np.int64)
    seen[:rows, :cols] = plane[:rows, :cols]
    labels = np.zeros((h, w), dtype=np.int64)
    boxes = []
    index = np.arange(h * w, dtype=np.int64).reshape(h, w)
    values = [int(v) for v in np.unique(seen) if v] if by_value else [None]
    for v in values:
        mask = seen == v if by_value else seen > 0
        lab, count = ndimage.label(mask, structure=EIGHT)
        for k, sl in enumerate(ndimage.find_objects(lab), start=1):
            own = lab[sl] == k
            labels[sl][own] = 1 + index[sl][own].min()
            (ymin, ymax), (xmin, xmax) = (sl[0].start, sl[0].stop - 1), (sl[1].start, sl[1].stop - 1)
            boxes.append((max(0, ymin - 1), min(rows, ymax + 2), max(0, xmin - 1), min(cols, xmax + 2)))
    return labels, boxes


def components(target, extent=None, by_value=False):
    """target (N,H,W) uint8 -> (labels (N,H,W) int32, n_objects (N,) int64, list per plane of boxes)"""
    target = np.asarray(target)
    n, h, w = target.shape
    labels, counts, boxes = np.zeros((n, h, w), dtype=np.int32), np.zeros(n, dtype=np.int64), []
    for i in range(n):
        rows, cols = clamp_extent(extent, i, h, w)
        lab, bx = plane_objects(target[i], rows, cols, by_value)
        labels[i], counts[i] = lab, len(bx)
        boxes.append(bx)
    return labels, counts, boxes


def cover(boxes, h, w):
    """list per plane of boxes -> (N,H,W) int64: 1 added over every box"""
    out = np.zeros((len(boxes), h, w), dtype=np.int64)
    for i, bx in enumerate(boxes):
        for y0, y1, x0, x1 in bx:
            out[i, y0:y1, x0:x1] += 1
    return out


def boxes_of_labels(labels, extent=None):
    """canonical labels (N,H,W) -> the boxes per plane (every label value is one object)"""
    labels = np.asarray(labels)
    n, h, w = labels.shape
    out = []
    for i in range(n):
        rows, cols = clamp_extent(extent, i, h, w)
        bx = []
        for sl in ndimage.find_objects(labels[i].astype(np.int64)):
            if sl is not None:
                bx.append((max(0, sl[0].start - 1), min(rows, sl[0].stop + 1), max(0, sl[1].start - 1), min(cols, sl[1].stop + 1)))
        out.append(bx)
    return out


def _cut(plane_logits, plane_target, boxes):
    """the reference's concatenation: logits (C,H,W), target (H,W) -> (C,K), (K,) over the pixels of all boxes"""
    c = plane_logits.shape[0]
    lg = [plane_logits[:, y0:y1, x0:x1].reshape(c, -1) for y0, y1, x0, x1 in boxes]
    tg = [plane_target[y0:y1, x0:x1].reshape(-1) for y0, y1, x0, x1 in boxes]
    if not boxes:
        return np.zeros((c, 0), dtype=np.float32), np.zeros((0,), dtype=np.uint8)
    return np.concatenate(lg, axis=1), np.concatenate(tg)


def object_counts(logits, target, boxes, t, top_k):
    """logits (N,C,H,W) float32, target (N,H,W) uint8, boxes per plane -> (N,6) int64: the plain record of the
    concatenated box pixels"""
    n = logits.shape[0]
    out = np.zeros((n, 6), dtype=np.int64)
    for i in range(n):
        lg, tg = _cut(logits[i], target[i], boxes[i])
        if tg.size:
            out[i] = record(lg[None], tg[None], t, top_k)[0]
    return out


def object_histogram(logits, target, boxes, bits, per_image=False):
    """logits (N,1,H,W) float32 -> int64 (2, 2^bits) or (N, 2, 2^bits): the plain histogram of the concatenated box pixels"""
    n = logits.shape[0]
    out = np.zeros((n, 2, 1 << bits), dtype=np.int64)
    for i in range(n):
        lg, tg = _cut(logits[i], target[i], boxes[i])
        if tg.size:
            out[i] = RO.histogram(lg.reshape(1, 1, 1, -1), tg.reshape(1, 1, -1), bits)
    return out if per_image else out.sum(axis=0)


# ---- the same sums with a weight per pixel: what the library computes for any uint16 weights -----------------------
def weighted_counts(logits, target, weight, t, top_k):
    """(N,C,HW), (N,HW), (N,HW) integer weights -> (N,6): every pixel repeated `weight` times, through the plain record"""
    n, c, hw = logits.shape
    out = np.zeros((n, 6), dtype=np.int64)
    for i in range(n):
        rep = np.asarray(weight[i], dtype=np.int64)
        if rep.sum():
            out[i] = record(np.repeat(logits[i], rep, axis=1)[None], np.repeat(target[i], rep)[None], t, top_k)[0]
    return out


def weighted_histogram(logits, target, weight, bits, extent=None, per_image=False):
    """the plain histogram with np.bincount weights, in integers"""
    logits = np.asarray(logits, dtype=np.float32)
    n, h, w = logits.shape[0], logits.shape[-2], logits.shape[-1]
    logits, target = logits.reshape(n, h, w), np.asarray(target).reshape(n, h, w)
    weight = np.asarray(weight).reshape(n, h, w).astype(np.int64)
    B = 1 << bits
    out = np.zeros((n, 2, B), dtype=np.int64)
    for i in range(n):
        rows, cols = clamp_extent(extent, i, h, w)
        b = RO.bin_of(logits[i, :rows, :cols], bits).reshape(-1)
        pos = (target[i, :rows, :cols] > 0).reshape(-1)
        wt = weight[i, :rows, :cols].reshape(-1)
        np.add.at(out[i, 0], b[~pos], wt[~pos])
        np.add.at(out[i, 1], b[pos], wt[pos])
    return out if per_image else out.sum(axis=0)
