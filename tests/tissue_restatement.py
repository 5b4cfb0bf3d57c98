"""The tissue mask restated in numpy / scipy (no tests here): what tests/test_tissue.py holds the device against, by
equality.  Nothing here shares a formulation with the product where another one exists: the histogram is numpy's own,
Otsu's threshold comes from the definition (explicit class sums per split, exactly summed), the area filters from
scipy.ndimage.label and numpy.bincount, the dilation from scipy.ndimage.binary_dilation with the disk as footprint (no
distance transform), the downscale from integer numpy sums.
"""
import math

import numpy as np
from scipy import ndimage as ndi

EIGHT = np.ones((3, 3), dtype=bool)


def gray(img):
    """(H,W,3) uint8 -> float64, elementwise"""
    rgb = np.asarray(img).astype(np.float64) / 255.0
    return (0.2125 * rgb[..., 0] + 0.7154 * rgb[..., 1]) + 0.0721 * rgb[..., 2]


def histogram(g):
    return np.histogram(g, 256)


def otsu_by_definition(counts, edges):
    """for every split k (bins 0..k against bins k+1..) the between-class variance w1 w2 (m1 - m2)^2 from the classes' own
    sums, each an exactly rounded sum (math.fsum); the centre of the first bin at which it is largest"""
    counts = [float(c) for c in counts]
    centres = [(float(a) + float(b)) / 2 for a, b in zip(edges[:-1], edges[1:])]
    best, at = -1.0, None
    for k in range(len(counts) - 1):
        w1, w2 = math.fsum(counts[:k + 1]), math.fsum(counts[k + 1:])
        if w1 == 0 or w2 == 0:
            continue
        m1 = math.fsum(c * x for c, x in zip(counts[:k + 1], centres[:k + 1])) / w1
        m2 = math.fsum(c * x for c, x in zip(counts[k + 1:], centres[k + 1:])) / w2
        v = w1 * w2 * (m1 - m2) ** 2
        if v > best:
            best, at = v, k
    return centres[at]


def small_components(plane, connectivity, least):
    """bool (H,W) -> bool: the pixels of the components of `plane` with fewer than `least` pixels"""
    lab, _ = ndi.label(plane, structure=EIGHT if connectivity == 8 else None)
    area = np.bincount(lab.ravel())
    small = area < least
    small[0] = False
    return small[lab]


def canonical_labels(plane, connectivity):
    """int32 (H,W): 0 on background, else 1 + the smallest row-major index of the pixel's component"""
    lab, count = ndi.label(plane, structure=EIGHT if connectivity == 8 else None)
    first = np.full(count + 1, lab.size, dtype=np.int64)
    np.minimum.at(first, lab.ravel(), np.arange(lab.size))
    out = (first[lab] + 1).astype(np.int32)
    out[lab == 0] = 0
    return out


def disk(radius):
    r = int(radius)
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    return yy * yy + xx * xx <= r * r


def dilate(plane, radius):
    return ndi.binary_dilation(plane, structure=disk(radius))


def tissue_mask(img, min_size=256, area_threshold=16384, radius=16):
    """-> dict(gray, counts, thr, thresholded, objects, holes, mask) of one (H,W,3) image"""
    g = gray(img)
    lo, hi = g.min(), g.max()
    if lo == hi:
        counts, thr = np.zeros(256, dtype=np.int64), float(lo)
    else:
        counts, edges = histogram(g)
        thr = otsu_by_definition(counts, edges)
    thresholded = g <= thr
    objects = thresholded & ~small_components(thresholded, 8, min_size)
    holes = objects | small_components(~objects, 4, area_threshold)
    return dict(gray=g, counts=counts, thr=thr, thresholded=thresholded, objects=objects, holes=holes,
                mask=dilate(holes, radius))


def downscale(img, f):
    """(H,W,C) uint8 -> (ceil(H/f), ceil(W/f), C) uint8: (2 sum + count) // (2 count) over the real pixels of each block"""
    img = np.asarray(img)
    h, w, c = img.shape
    oh, ow = -(-h // f), -(-w // f)
    pad = np.zeros((oh * f, ow * f, c), dtype=np.int64)
    pad[:h, :w] = img
    one = np.zeros((oh * f, ow * f), dtype=np.int64)
    one[:h, :w] = 1
    total = pad.reshape(oh, f, ow, f, c).sum(axis=(1, 3))
    cnt = one.reshape(oh, f, ow, f).sum(axis=(1, 3))[..., None]
    return ((2 * total + cnt) // (2 * cnt)).astype(np.uint8)
