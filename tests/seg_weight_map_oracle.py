"""The reference's weight map (WeightsDistances, utils/datasets/_augs.py:102-136) in numpy / scipy, for one label plane:
scipy.ndimage.label with the 3x3 structure, one full-plane distance_transform_edt per object, the per-pixel sort, and
the U-Net weight.  Beside the reference's own float32 result it returns what the tests compare with: the sorted integer
squared distances and the map in float64.  No tests in this file."""
import numpy as np
from scipy import ndimage

EIGHT = np.ones((3, 3))


def distances(plane, labels=None):
    """plane (h, w), foreground where != 0 (or `labels` (h, w) integers: one object per distinct non-zero value) ->
    (count, dist float64 [count, h, w] sorted along axis 0): per object the distance of every pixel to it"""
    if labels is None:
        lab, count = ndimage.label(np.asarray(plane) != 0, structure=EIGHT)
        names = range(1, count + 1)
    else:
        lab = np.asarray(labels)
        names = [v for v in np.unique(lab) if v != 0]
        count = len(names)
    dist = [ndimage.distance_transform_edt(lab != name) for name in names]
    if not dist:
        return 0, np.zeros((0,) + lab.shape)
    return count, np.sort(np.stack(dist), axis=0)


def squared(plane, labels=None):
    """-> (count, d2 int64 [2, h, w]): rint(d^2) of the two smallest distances, -1 where there is no such object.
    (A float64 root of an integer below 2^31 squares back to within 2^-21 of it.)"""
    count, dist = distances(plane, labels)
    shape = np.asarray(plane if labels is None else labels).shape
    d2 = np.full((2,) + shape, -1, dtype=np.int64)
    for i in range(min(count, 2)):
        d2[i] = np.rint(dist[i] ** 2).astype(np.int64)
    return count, d2


def exponent(count, dist, sigma):
    """the argument of the exponential in float64, (d_0 + d_1)^2 / (2 sigma^2) (one object: d_0^2 / (2 sigma^2)), from
    the float64 distances; None for a plane without objects"""
    if count == 0:
        return None
    s = dist[0] + dist[1] if count > 1 else dist[0]
    return s ** 2 / (2.0 * float(sigma) ** 2)


def weight_map(target, class_weights, sigma=5, w_0=10):
    """target (h, w) of integer label values -> dict(count, d2, arg, e, w64, w32): `e` = exp(-arg) and `w64` the map in
    float64, `w32` the reference's own float32 evaluation and `e32` its exponential part"""
    target = np.asarray(target)
    cw = np.take(np.asarray(class_weights), target.astype(np.int32))
    count, dist = distances(target)
    _, d2 = squared(target)
    arg = exponent(count, dist, sigma)
    w32 = cw.astype(np.float32)
    if count == 0:
        return dict(count=0, d2=d2, arg=None, e=np.zeros(target.shape), w64=cw.astype(np.float64), w32=w32)
    e = np.exp(-arg)
    d32 = dist.astype(np.float32)
    sigma_2 = 2 * sigma ** 2
    w_1 = np.exp(-(d32[0] + d32[1]) ** 2 / sigma_2) if count > 1 else np.exp(-d32[0] ** 2 / sigma_2)
    return dict(count=count, d2=d2, arg=arg, e=e, w64=cw.astype(np.float64) + float(w_0) * e, w32=w32 + w_0 * w_1,
                e32=w_1)


def bound(arg, e):
    """what the exponential part of a float32 evaluation may differ from `e` by: five fp32 roundings on the way to arg
    (two roots, their sum, the square, the quotient) each shift e by arg 2^-24 relative, plus a few ulps of expf; the
    constants carry about 2x headroom.  2^-126: a result below the normal range may be flushed to zero."""
    return (8.0 * arg + 4.0) * 2.0 ** -24 * e + 2.0 ** -126


def brute(labels):
    """labels (h, w) integers -> d2 int64 [2, h, w] by a search over all pixel pairs: per pixel the smallest squared
    distance to every object, then the two smallest of them"""
    labels = np.asarray(labels)
    h, w = labels.shape
    yy, xx = np.mgrid[0:h, 0:w]
    per = []
    for name in np.unique(labels):
        if name == 0:
            continue
        ys, xs = np.nonzero(labels == name)
        per.append(((yy[..., None] - ys) ** 2 + (xx[..., None] - xs) ** 2).min(axis=-1))
    d2 = np.full((2, h, w), -1, dtype=np.int64)
    if per:
        s = np.sort(np.stack(per), axis=0)
        d2[:min(len(per), 2)] = s[:2]
    return d2


def blobs(h, w, density, seed, smooth=2.0):
    """a (h, w) uint8 mask of Gaussian-filtered noise thresholded at the `density` quantile"""
    rng = np.random.default_rng(seed)
    f = ndimage.gaussian_filter(rng.standard_normal((h, w)), smooth, mode='wrap')
    return (f > np.quantile(f, 1.0 - density)).astype(np.uint8)
