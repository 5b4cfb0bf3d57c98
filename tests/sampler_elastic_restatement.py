"""The contract of cae_t_elastic_deform (include/cae_hip.h) restated literally in float64 numpy, for the elastic
deformation tests: the displacement field of a 3 x 3 grid, the clamp, the repeated reflection of indices, the recursive
cubic B-spline prefilter with its exact half-sample-symmetric start, the 4 x 4 taps and the nearest-neighbour rule of the
mask.  Nothing here comes from the product.

`deform(..., defect=...)` plants one wrong reading of the contract (tests/test_sampler_elastic_host.py shows that each
falls outside the bound of the GPU tests), and `deform_f32` walks the kernels' arithmetic in float32, operation by
operation (without the fused multiply-adds a compiler may form), so the bound can be checked where no GPU is.
"""
import numpy as np

POLE = np.sqrt(3.0) - 2.0
GAIN = (1.0 - POLE) * (1.0 - 1.0 / POLE)  # 6
# the l1 gain of the prefilter along one axis: ((1 + |z|) / (1 - |z|))^2 = 3
L1_GAIN = ((1.0 + abs(POLE)) / (1.0 - abs(POLE))) ** 2
M = np.array([[2.0 / 3.0, 1.0 / 3.0, 0.0], [1.0 / 6.0, 2.0 / 3.0, 1.0 / 6.0], [0.0, 1.0 / 3.0, 2.0 / 3.0]])
START_TERMS, POWER_TERMS = 22, 64  # what the kernels keep of the start (the contract names both)


def beta(r):
    """the cubic B-spline"""
    r = np.abs(r)
    return np.where(r < 1.0, 2.0 / 3.0 - r * r + r * r * r / 2.0, np.where(r < 2.0, (2.0 - r) ** 3 / 6.0, 0.0))


def coefficients(d):
    """coef[k] = M^-1 d[k] M^-T for displacement grids [n, 2, 3, 3], float64"""
    d = np.asarray(d, dtype=np.float64)
    return np.linalg.solve(M, np.linalg.solve(M, d.swapaxes(-1, -2)).swapaxes(-1, -2))


def coefficients_f32(d):
    """as the kernel gets them: solved in float64, rounded once"""
    return coefficients(d).astype(np.float32)


def folded_weights(ps, extension='mirror'):
    """W[a][i] = W_a(u_i), [3, ps]"""
    u = 2.0 * np.arange(ps, dtype=np.float64) / (ps - 1) if ps > 1 else np.zeros(1)
    if extension == 'mirror':   # ... 2 1 | 0 1 2 | 1 0 ...
        return np.stack([beta(u), beta(u - 1.0) + beta(u + 1.0) + beta(u - 3.0), beta(u - 2.0)])
    assert extension == 'reflect'  # the planted defect: ... 1 0 | 0 1 2 | 2 1 ...
    return np.stack([beta(u) + beta(u + 1.0), beta(u - 1.0), beta(u - 2.0) + beta(u - 3.0)])


def field(coef, ps, extension='mirror'):
    """D[k][i][j] of one sample's coefficients [2, 3, 3]"""
    w = folded_weights(ps, extension)
    with np.errstate(invalid='ignore', over='ignore'):
        return np.einsum('ai,bj,kab->kij', w, w, np.asarray(coef, dtype=np.float64))


def source_points(coef, ps, extension='mirror', swap=False):
    """(y, x) float64 [ps, ps], clamped; a NaN becomes -ps"""
    d = field(coef, ps, extension)
    if swap:
        d = d[::-1]
    i, j = np.meshgrid(np.arange(ps, dtype=np.float64), np.arange(ps, dtype=np.float64), indexing='ij')
    lo, hi = -float(ps), 2.0 * ps
    return np.fmin(np.fmax(i + d[0], lo), hi), np.fmin(np.fmax(j + d[1], lo), hi)


def reflect(idx, n):
    """d c b a | a b c d | d c b a, as often as needed"""
    m = np.mod(idx, 2 * n)
    return np.where(m >= n, 2 * n - 1 - m, m)


def prefilter_line(line, start='reflect'):
    """the interpolation coefficients of lines of n >= 1 samples (the last axis), float64"""
    c = np.array(line, dtype=np.float64) * GAIN
    n, z = c.shape[-1], POLE
    if start == 'reflect':
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
    else:
        assert start == 'mirror' and n >= 2  # the planted defect: the whole-sample symmetric start and end
        ext = np.concatenate([c, c[..., -2:0:-1]], axis=-1)  # one period, 2 n - 2 samples
        c[..., 0] = (ext * z ** np.arange(2 * n - 2)).sum(-1) / (1.0 - z ** (2 * n - 2))
        for i in range(1, n):
            c[..., i] += z * c[..., i - 1]
        c[..., n - 1] = z / (z * z - 1.0) * (c[..., n - 1] + z * c[..., n - 2])
    for i in range(n - 2, -1, -1):
        c[..., i] = z * (c[..., i + 1] - c[..., i])
    return c


def prefilter(planes, start='reflect'):
    """rows, then columns, of [..., ps, ps] planes"""
    rows = prefilter_line(planes, start)
    return np.swapaxes(prefilter_line(np.swapaxes(rows, -1, -2), start), -1, -2)


def near_a_tie(y, x, eps):
    """[ps, ps] bool: y + 0.5 or x + 0.5 of the source point lies within eps of an integer (the nearest neighbour is then
    decided by the last bits of the coordinate)"""
    return (np.abs(y + 0.5 - np.round(y + 0.5)) <= eps) | (np.abs(x + 0.5 - np.round(x + 0.5)) <= eps)


DEFECTS = ('field_reflect', 'axes_swapped', 'no_prefilter', 'window_from_round', 'mirror_start')


def deform(x, t, coef, defect=None, info=None):
    """x [n, c, ps, ps], t [n, kt, ps, ps] or None, coef [n, 2, 3, 3] (as the kernel gets them) -> float64 (x', t').
    `info`, a dict, receives 'coef_max' (the largest interpolation coefficient in magnitude), 'x_max' and 'field_max'
    (the largest field coefficient of a sample whose coefficients are all finite and below 1e20)."""
    assert defect is None or defect in DEFECTS
    x = np.asarray(x, dtype=np.float64)
    n, ch, ps, _ = x.shape
    if defect == 'no_prefilter':
        cf = x
    else:
        cf = prefilter(x, 'mirror' if defect == 'mirror_start' else 'reflect')
    if info is not None:
        tame = [np.abs(c).max() for c in np.asarray(coef, dtype=np.float64) if np.isfinite(c).all() and np.abs(c).max() < 1e20]
        info.update(coef_max=float(np.abs(cf).max()), x_max=float(np.abs(x).max()), field_max=float(max(tame, default=0.0)))
    x_out = np.zeros((n, ch, ps, ps))
    t_out = None if t is None else np.empty(np.shape(t), dtype=np.float64)
    for s in range(n):
        y, xx = source_points(coef[s], ps, 'reflect' if defect == 'field_reflect' else 'mirror', defect == 'axes_swapped')
        if t is not None:
            t_out[s] = np.asarray(t[s])[:, reflect(np.floor(y + 0.5).astype(np.int64), ps),
                                        reflect(np.floor(xx + 0.5).astype(np.int64), ps)]
        shift = 0.5 if defect == 'window_from_round' else 0.0
        ys, xs = np.floor(y + shift).astype(np.int64) - 1, np.floor(xx + shift).astype(np.int64) - 1
        for a in range(4):
            wy, ry = beta(y - (ys + a)), reflect(ys + a, ps)
            for b in range(4):
                x_out[s] += wy * beta(xx - (xs + b)) * cf[s][:, ry, reflect(xs + b, ps)]
    return x_out, t_out


# ------------------------------------------------------------------------------- the kernels' arithmetic in float32
F = np.float32


def _beta_f32(d):
    d = np.abs(d).astype(F)
    near = d * d * (F(0.5) * d - F(1.0)) + F(2.0) / F(3.0)
    e = F(2.0) - np.minimum(d, F(2.0))
    return np.where(d < F(1.0), near, e * e * e * (F(1.0) / F(6.0))).astype(F)


def _filter_line_f32(c):
    """the last axis of float32 `c`, in place"""
    n, z, gain = c.shape[-1], F(POLE), F(6.0)
    zn = F(1.0)
    for _ in range(min(n, POWER_TERMS)):
        zn = zn * z
    if n > POWER_TERMS:
        zn = F(0.0)
    c0 = gain * c[..., 0]
    acc, zi = c0 + zn * (gain * c[..., n - 1]), z
    for i in range(1, min(n, START_TERMS)):
        acc = acc + zi * (gain * (c[..., i] + zn * c[..., n - 1 - i]))
        zi = zi * z
    v = c0 + z / (F(1.0) - zn * zn) * acc
    c[..., 0] = v
    for i in range(1, n):
        v = gain * c[..., i] + z * v
        c[..., i] = v
    v = v * (z / (z - F(1.0)))
    c[..., n - 1] = v
    for i in range(n - 2, -1, -1):
        v = z * (v - c[..., i])
        c[..., i] = v
    return c


def deform_f32(x, t, coef):
    """(x', t') as the kernels compute them, every operation rounded to float32"""
    x = np.array(x, dtype=F)
    coef = np.asarray(coef, dtype=F)
    n, ch, ps, _ = x.shape
    cf = _filter_line_f32(x)
    cf = np.swapaxes(_filter_line_f32(np.ascontiguousarray(np.swapaxes(cf, -1, -2))), -1, -2)
    scale = F(2.0) / F(ps - 1) if ps > 1 else F(0.0)
    u = np.arange(ps).astype(F) * scale
    w = np.stack([_beta_f32(u), (_beta_f32(u - F(1.0)) + _beta_f32(u + F(1.0))) + _beta_f32(u - F(3.0)), _beta_f32(u - F(2.0))])
    i, j = np.meshgrid(np.arange(ps).astype(F), np.arange(ps).astype(F), indexing='ij')
    x_out = np.zeros((n, ch, ps, ps), dtype=F)
    t_out = None if t is None else np.empty(np.shape(t), dtype=F)
    with np.errstate(invalid='ignore', over='ignore'):
        for s in range(n):
            d = []
            for k in range(2):
                acc = np.zeros((ps, ps), dtype=F)
                for a in range(3):
                    r = np.zeros(ps, dtype=F)
                    for b in range(3):
                        r = r + w[b] * coef[s, k, a, b]
                    acc = acc + w[a][:, None] * r[None, :]
                d.append(acc)
            lo, hi = F(-ps), F(2 * ps)
            y, xx = np.fmin(np.fmax(i + d[0], lo), hi), np.fmin(np.fmax(j + d[1], lo), hi)
            if t is not None:
                t_out[s] = np.asarray(t[s])[:, reflect(np.floor(y + F(0.5)).astype(np.int64), ps),
                                            reflect(np.floor(xx + F(0.5)).astype(np.int64), ps)]
            ys, xs = np.floor(y).astype(np.int64) - 1, np.floor(xx).astype(np.int64) - 1
            acc = np.zeros((ch, ps, ps), dtype=F)
            for a in range(4):
                r = np.zeros((ch, ps, ps), dtype=F)
                for b in range(4):
                    r = r + _beta_f32(xx - (xs + b).astype(F)) * cf[s][:, reflect(ys + a, ps), reflect(xs + b, ps)]
                acc = acc + _beta_f32(y - (ys + a).astype(F)) * r
            x_out[s] = acc
    return x_out, t_out
