"""The contract of cae_t_sample_labeled_patches (include/cae_hip.h) restated literally in float64 numpy, for the labelled
sampler tests: the recursive quartic B-spline prefilter with its exact half-sample-symmetric start, the repeated
reflection of indices, the 5 x 5 tap weights and the nearest-neighbour rule of the mask.

The image patch p itself (crop, u8 / 255, Philox noise, clamp, normalise, padding) is the one of cae_t_sample_patches and
comes from sampler_restatement.patch; nothing is restated twice, and nothing here comes from the product.
"""
import numpy as np

import sampler_restatement as R

# the poles of the quartic B-spline's recursive inverse filter
Z1 = np.sqrt(664.0 - np.sqrt(438976.0)) + np.sqrt(304.0) - 19.0
Z2 = np.sqrt(664.0 + np.sqrt(438976.0)) - np.sqrt(304.0) - 19.0
POLES = (Z1, Z2)
GAIN = float(np.prod([(1.0 - z) * (1.0 - 1.0 / z) for z in POLES]))
# The l1 gain of the prefilter along one axis (the bound of the GPU tests is built from it).  One pole's two-sided
# response is ((1 - z) / (1 + z)) z^|k|, of l1 norm ((1 + |z|) / (1 - |z|))^2 for z < 0; both poles: 4.8.  It is also the
# product of the l1 gains of the steps the line goes through (gain, causal, anticausal, per pole).
L1_GAIN = float(np.prod([(1.0 + abs(z)) / (1.0 - abs(z)) for z in POLES])) ** 2


def prefilter_line(line):
    """the interpolation coefficients of a line of n >= 1 samples (the last axis; every line of an array alike), float64"""
    c = np.array(line, dtype=np.float64) * GAIN
    n = c.shape[-1]
    for z in POLES:
        zn = z ** n
        acc = c[..., 0] + zn * c[..., n - 1]
        zi = z
        for i in range(1, n):
            acc = acc + zi * (c[..., i] + zn * c[..., n - 1 - i])
            zi *= z
        c[..., 0] = c[..., 0] + z / (1.0 - zn * zn) * acc
        for i in range(1, n):
            c[..., i] += z * c[..., i - 1]
        c[..., n - 1] *= z / (z - 1.0)
        for i in range(n - 2, -1, -1):
            c[..., i] = z * (c[..., i + 1] - c[..., i])
    return c


def prefilter(planes):
    """rows, then columns, of [..., ps, ps] planes"""
    rows = prefilter_line(planes)
    return np.swapaxes(prefilter_line(np.swapaxes(rows, -1, -2)), -1, -2)


def reflect(idx, n):
    """d c b a | a b c d | d c b a, as often as needed"""
    m = np.mod(idx, 2 * n)
    return np.where(m >= n, 2 * n - 1 - m, m)


def weight(d):
    """the quartic B-spline at distance d"""
    d = np.abs(d)
    return np.where(d < 0.5, d * d * (d * d / 4.0 - 5.0 / 8.0) + 115.0 / 192.0,
                    np.where(d < 1.5, d * (d * (d * (5.0 / 6.0 - d / 6.0) - 5.0 / 4.0) + 5.0 / 24.0) + 55.0 / 96.0,
                             np.where(d < 2.5, (d - 2.5) ** 4 / 24.0, 0.0)))


def source_points(ps, cos_a, sin_a):
    """(y, x) float64 [ps, ps] of every output pixel (i, j); cos_a, sin_a as the kernel gets them"""
    ca, sa = float(cos_a), float(sin_a)
    c = (ps - 1) / 2.0
    i, j = np.meshgrid(np.arange(ps, dtype=np.float64), np.arange(ps, dtype=np.float64), indexing='ij')
    return ca * (i - c) + sa * (j - c) + c, -sa * (i - c) + ca * (j - c) + c


def rotate_image(p, cos_a, sin_a):
    """p [C, ps, ps] float64 -> the spline rotation, reflected edges, no clipping"""
    ch, ps, _ = p.shape
    y, x = source_points(ps, cos_a, sin_a)
    ys, xs = np.floor(y + 0.5).astype(np.int64) - 2, np.floor(x + 0.5).astype(np.int64) - 2
    out = np.zeros((ch, ps, ps))
    coef = prefilter(p)
    for a in range(5):
        wy, ry = weight(y - (ys + a)), reflect(ys + a, ps)
        for b in range(5):
            out += wy * weight(x - (xs + b)) * coef[:, ry, reflect(xs + b, ps)]
    return out


def rotate_mask(m, cos_a, sin_a):
    """m [K, ps, ps] -> nearest neighbour, reflected edges"""
    ps = m.shape[-1]
    y, x = source_points(ps, cos_a, sin_a)
    return m[:, reflect(np.floor(y + 0.5).astype(np.int64), ps), reflect(np.floor(x + 0.5).astype(np.int64), ps)]


def near_a_tie(ps, cos_a, sin_a, eps=1e-4):
    """[ps, ps] bool: y + 0.5 or x + 0.5 of the source point lies within eps of an integer (the nearest neighbour is then
    decided by the last bits of the coordinate)"""
    y, x = source_points(ps, cos_a, sin_a)
    return (np.abs(y + 0.5 - np.round(y + 0.5)) <= eps) | (np.abs(x + 0.5 - np.round(x + 0.5)) <= eps)


def mask_patch(labels, tile, y0, x0, ps, map_labels=False, tile_hw=None):
    """m of one sample: float64 [Kt, ps, ps], 0 outside the tile's valid extent"""
    t_, h, w, k = labels.shape
    hv, wv = (h, w) if tile_hw is None else (int(tile_hw[tile][0]), int(tile_hw[tile][1]))
    py, px = np.meshgrid(np.arange(ps), np.arange(ps), indexing='ij')
    iy, ix = y0 + py, x0 + px
    inside = (iy >= 0) & (iy < hv) & (ix >= 0) & (ix < wv)
    m = np.where(inside[..., None], labels[tile, np.clip(iy, 0, h - 1), np.clip(ix, 0, w - 1)].astype(np.float64), 0.0)
    m = m.transpose(2, 0, 1)
    return m.sum(axis=0, keepdims=True) if map_labels else np.ascontiguousarray(m)


def batch(pool, labels, tile, y0, x0, ps, angle=None, seed=0, noise_std=0.0, normalize=False, sample_base=0, tile_hw=None,
          map_labels=False, info=None):
    """(x float64 [n, C, ps, ps], t float64 [n, Kt, ps, ps]); `info`, a dict, receives 'coef_max', the largest
    interpolation coefficient of the batch in magnitude (the bound of the GPU tests scales with it)"""
    xs, ts = [], []
    if info is not None:
        info['coef_max'] = 0.0
    for s in range(len(tile)):
        p = R.patch(pool, int(tile[s]), int(y0[s]), int(x0[s]), ps, sample_base + s, seed, noise_std, normalize, tile_hw)
        m = mask_patch(labels, int(tile[s]), int(y0[s]), int(x0[s]), ps, map_labels, tile_hw)
        if info is not None:
            info['coef_max'] = max(info['coef_max'], float(np.abs(prefilter(p)).max()))
        if angle is not None:
            cs = R.cos_sin_f32(angle[s])
            p, m = rotate_image(p, *cs), rotate_mask(m, *cs)
        xs.append(p)
        ts.append(m)
    return np.stack(xs), np.stack(ts)
