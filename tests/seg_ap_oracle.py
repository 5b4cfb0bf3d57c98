"""numpy restatement of the score histogram contract (include/cae_hip.h, "Score histograms of a head of several
classes") and of average precision; no tests here.  Written from the contract's words, not from the library's code: the
bin of an fp32 score on uint32 views, the histogram of a batch as np.bincount per class, the bin edges by a search over
every score that can matter, and the average precision of unbinned scores from sklearn's definition by sorting.
"""
import math

import numpy as np


def score_bin(s, bits):
    """float32 array -> int64 bin in 0 .. 2^bits - 1"""
    s = np.asarray(s, dtype=np.float32)
    B, sh = 1 << bits, np.uint32(31 - bits)
    zero = np.isnan(s) | (s <= 0)  # NaN, negatives, both zeros
    one = s >= 1
    safe = np.where(zero | one, np.float32(0.25), s)
    low = safe < np.float32(0.5)
    t = np.float32(1) - safe  # exact where safe >= 0.5
    v = np.where(low, safe, t).astype(np.float32).view(np.uint32) >> sh
    b = np.where(low, v.astype(np.int64), B - 1 - v.astype(np.int64))
    return np.where(zero, 0, np.where(one, B - 1, b)).astype(np.int64)


def linear_bin(s, bits):
    """a wrong bin on purpose (the judge case): linear in the score"""
    s = np.nan_to_num(np.asarray(s, dtype=np.float64), nan=0.0)
    return np.clip(np.floor(np.clip(s, 0, 1) * (1 << bits)), 0, (1 << bits) - 1).astype(np.int64)


def score_hist(scores, target, bits, extent=None, bin_of=score_bin, positive=None):
    """scores (N,C,H,W) float32, target (N,H,W) uint8, extent (N,2) ints | None -> int64 (N, C, 2, 2^bits): row 1 the
    pixels with target == k, row 0 the other labelled ones; labels >= C and pixels outside the extent nowhere.
    ``positive(target, k)``: another rule for row 1 (the judge case)"""
    scores = np.asarray(scores, dtype=np.float32)
    n, c, h, w = scores.shape
    target = np.asarray(target).reshape(n, h, w)
    B = 1 << bits
    out = np.zeros((n, c, 2, B), dtype=np.int64)
    for i in range(n):
        rows, cols = (h, w) if extent is None else (min(max(int(extent[i][0]), 0), h), min(max(int(extent[i][1]), 0), w))
        t = target[i, :rows, :cols].reshape(-1)
        labelled = t < c
        for k in range(c):
            b = bin_of(scores[i, k, :rows, :cols], bits).reshape(-1)
            pos = (t == k) if positive is None else positive(t, k)
            out[i, k, 0] = np.bincount(b[labelled & ~pos], minlength=B)
            out[i, k, 1] = np.bincount(b[labelled & pos], minlength=B)
    return out


def edges(bits):
    """float32 (2^bits,): the smallest score in [0, 1] of every bin, NaN for a bin without one.  By search: below 0.5 a
    bin is a run of 2^(31 - bits) >= 2^17 bit patterns, so its smallest score has 16 zero low bits; from 0.5 on the
    scores are the multiples of 2^-24, all of which are candidates."""
    lower = (np.arange(0x3F00, dtype=np.uint32) << np.uint32(16)).view(np.float32)  # [0, 0.5)
    upper = (np.arange(1 << 23, 1 << 24, dtype=np.float64) * 2.0 ** -24).astype(np.float32)  # [0.5, 1)
    cand = np.concatenate([lower, upper, np.ones(1, np.float32)])
    assert (np.diff(cand) > 0).all()
    b = score_bin(cand, bits)
    assert (np.diff(b) >= 0).all()  # monotone in the score
    out = np.full(1 << bits, np.nan, dtype=np.float32)
    first = np.flatnonzero(np.concatenate(([True], np.diff(b) > 0)))
    out[b[first]] = cand[first]
    return out


def ap_sorted(target_onehot, scores):
    """sklearn's average_precision_score (micro over whatever is passed): sum_k (R_k - R_{k-1}) P_k over the distinct
    scores from the top down, ties forming one threshold; sorted in float64, the terms divided in Python integers and
    added with math.fsum, so the result is within 2^-51 of the exact value.  NaN without positives"""
    y = np.asarray(target_onehot).reshape(-1).astype(bool)
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    P = int(y.sum())
    if P == 0:
        return float('nan')
    order = np.argsort(-s, kind='stable')
    y, s = y[order], s[order]
    last = np.flatnonzero(np.concatenate((np.diff(s) != 0, [True])))  # the last index of every run of equal scores
    tp = np.cumsum(y)[last]
    seen = last + 1
    gain = np.diff(np.concatenate(([0], tp)))
    return math.fsum(int(g) * int(t) / int(m) for g, t, m in zip(gain, tp, seen) if g) / P


# ---- the inputs that the host judge case and the GPU tests share ---------------------------------------------------------
SHAPES = [(2, 3, 37, 45), (1, 2, 96, 100), (2, 17, 8, 12), (3, 5, 16, 16)]  # (N, C, H, W)
EXTENTS = {(3, 5, 16, 16): [(16, 16), (5, 7), (0, 3)]}


def draw(n, c, h, w, seed):
    """logits (n,c,h,w) float32, sharp on some pixels and flat on others, with the target's class raised on most, and a
    target (n,h,w) uint8 with a share of labels >= c (c, 200, 255)"""
    rng = np.random.default_rng(seed)
    scale = rng.choice(np.array([0.3, 1.0, 4.0, 12.0], dtype=np.float32), (n, 1, h, w))
    logits = (scale * rng.standard_normal((n, c, h, w))).astype(np.float32)
    target = rng.integers(0, c, (n, h, w)).astype(np.uint8)
    lift = rng.choice(np.array([0.0, 1.0, 3.0], dtype=np.float32), (n, h, w))
    np.put_along_axis(logits, target[:, None].astype(np.int64), np.take_along_axis(
        logits, target[:, None].astype(np.int64), axis=1) + lift[:, None], axis=1)
    unlabelled = rng.random((n, h, w)) < 0.05
    target = np.where(unlabelled, rng.choice(np.array([c, 200, 255], dtype=np.uint8), (n, h, w)), target).astype(np.uint8)
    return logits, target


def softmax32(logits):
    """float32 softmax over axis 1 (the host's; the device's scores differ in the last bits)"""
    x = logits.astype(np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def special_values(bits):
    """every edge with its two fp32 neighbours, 0, -0, denormals, 0.5 +- 1 ulp, 1 and its neighbours, NaN, negatives,
    values above 1, infinities"""
    e = edges(bits)
    e = e[~np.isnan(e)]
    one, half = np.float32(1), np.float32(0.5)
    with np.errstate(over='ignore'):
        return np.concatenate([e, np.nextafter(e, np.float32(-1)), np.nextafter(e, np.float32(2)), np.array(
            [0.0, -0.0, 1e-45, 1e-41, 1e-39, 1.1754944e-38, np.nextafter(half, np.float32(0)), half,
             np.nextafter(half, one), 0.25, 0.75, np.nextafter(one, np.float32(0)), one, np.nextafter(one, np.float32(2)),
             np.nan, -np.nan, -1e-45, -0.5, -3.0, 1.5, 1e30, np.inf, -np.inf], dtype=np.float32)]).astype(np.float32)
