"""numpy restatement of the ROC histogram contract (include/cae_hip.h, "ROC histograms of a one-class head"); no tests
here.  Written from the contract's words, not from the library's code: key and bin of an fp32 logit, the histogram of a
batch with an extent, the bin edges by a search over bit patterns, and the exact AUC by ranks with ties.
"""
import numpy as np


def key(x):
    """float32 array -> uint32 order-preserving key; NaN -> 0"""
    x = np.asarray(x, dtype=np.float32)
    xp = x + np.float32(0.0)  # -0 -> +0; numpy keeps denormals
    u = xp.view(np.uint32)
    k = np.where(u >> np.uint32(31), ~u, u | np.uint32(0x80000000))
    return np.where(np.isnan(x), np.uint32(0), k).astype(np.uint32)


def bin_of(x, bits):
    return (key(x) >> np.uint32(32 - bits)).astype(np.int64)


def histogram(logits, target, bits, extent=None, per_image=False):
    """logits (N,1,H,W) | (N,H,W) float32, target (N,H,W) uint8, extent (N,2) ints | None -> int64 (2, 2^bits), or
    (N, 2, 2^bits) per image: row 0 the negatives (target == 0), row 1 the positives"""
    logits = np.asarray(logits, dtype=np.float32)
    n, h, w = logits.shape[0], logits.shape[-2], logits.shape[-1]
    logits, target = logits.reshape(n, h, w), np.asarray(target).reshape(n, h, w)
    B = 1 << bits
    out = np.zeros((n, 2, B), dtype=np.int64)
    for i in range(n):
        rows, cols = (h, w) if extent is None else (min(max(int(extent[i][0]), 0), h), min(max(int(extent[i][1]), 0), w))
        b = bin_of(logits[i, :rows, :cols], bits).reshape(-1)
        pos = (target[i, :rows, :cols] > 0).reshape(-1)
        out[i, 0] = np.bincount(b[~pos], minlength=B)
        out[i, 1] = np.bincount(b[pos], minlength=B)
    return out if per_image else out.sum(axis=0)


def edges(bits):
    """float32 (2^bits,): the smallest non-NaN value of every bin, NaN for a bin without one.  By search: a bin is a run
    of 2^(32 - bits) >= 2^18 consecutive keys, so its smallest value has a bit pattern whose low 16 bits are all zero
    (positive values, and -inf) or all one (negative values); the candidates are all patterns of those two kinds."""
    hi = np.arange(1 << 16, dtype=np.uint32) << np.uint32(16)
    cand = np.concatenate([hi, hi | np.uint32(0xFFFF)]).view(np.float32)
    cand = cand[~np.isnan(cand)]
    cand = cand[cand.view(np.uint32) != np.uint32(0x80000000)]  # -0 is counted as +0: never a value of its own
    order = np.argsort(cand, kind='stable')
    cand = cand[order]
    b = bin_of(cand, bits)
    assert (np.diff(b) >= 0).all()  # monotone in the value
    out = np.full(1 << bits, np.nan, dtype=np.float32)
    first = np.flatnonzero(np.concatenate(([True], np.diff(b) > 0)))
    out[b[first]] = cand[first]
    return out


def exact_auc(logits, target):
    """the AUC of unbinned logits: P(pos > neg) + P(pos == neg) / 2 over all pairs, by counting on the full 32-bit key
    (ranks with ties) in Python integers; NaN without positives or negatives"""
    k = key(np.asarray(logits, dtype=np.float32).reshape(-1))
    pos = np.asarray(target).reshape(-1) > 0
    P, N = int(pos.sum()), int((~pos).sum())
    if P == 0 or N == 0:
        return float('nan')
    vals, inv = np.unique(k, return_inverse=True)
    pk = np.bincount(inv[pos], minlength=vals.size)
    nk = np.bincount(inv[~pos], minlength=vals.size)
    below = np.concatenate(([0], np.cumsum(nk)[:-1]))
    twice = sum(int(p) * (2 * int(b) + int(m)) for p, b, m in zip(pk, below, nk) if p)
    return twice / (2 * P * N)
