"""The contract of cae_t_sample_patches (include/cae_hip.h) restated literally in float64 numpy, for the sampler tests.

Philox4x32-10 is exact integer arithmetic (uint64 products of 32-bit words); Box-Muller, the noise sum, the clamp, the
normalisation and the four-tap rotation are float64.  The one float32 value of the contract, the correctly rounded
quotient u8 / 255, enters as that float32 value.  Nothing here comes from the product.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two ints -> four uint64 arrays holding 32-bit words"""
    c = [np.asarray(v, dtype=np.uint64) for v in counter]
    c = [np.array(v) for v in np.broadcast_arrays(*c)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def normals(seed, sample, pixel):
    """float64 [..., 4]: the four normals of counter (sample, pixel, 0, 0) under key (seed low, seed high)"""
    w = philox4x32_10((sample, pixel, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))
    u = [(x.astype(np.float64) + 0.5) * 2.0 ** -32 for x in w]
    g = np.empty(w[0].shape + (4,))
    for pair in (0, 1):
        r = np.sqrt(-2.0 * np.log(u[2 * pair]))
        g[..., 2 * pair] = r * np.cos(2.0 * np.pi * u[2 * pair + 1])
        g[..., 2 * pair + 1] = r * np.sin(2.0 * np.pi * u[2 * pair + 1])
    return g


def patch(pool, tile, y0, x0, ps, sample=0, seed=0, noise_std=0.0, normalize=False, tile_hw=None):
    """p of one sample: float64 [C, ps, ps]"""
    t_, h, w, c = pool.shape
    hv, wv = (h, w) if tile_hw is None else (int(tile_hw[tile][0]), int(tile_hw[tile][1]))
    std = float(np.float32(noise_std))  # the entry point takes a float
    py, px = np.meshgrid(np.arange(ps), np.arange(ps), indexing='ij')
    g = normals(seed, sample, py * ps + px) if std != 0.0 else np.zeros((ps, ps, 4))
    iy, ix = y0 + py, x0 + px
    inside = (iy >= 0) & (iy < hv) & (ix >= 0) & (ix < wv)
    u8 = pool[tile, np.clip(iy, 0, h - 1), np.clip(ix, 0, w - 1)]  # [ps, ps, C]
    q = (u8.astype(np.float32) / np.float32(255.0)).astype(np.float64)  # the correctly rounded float32 quotient
    v = np.clip(q + std * g[..., :c], 0.0, 1.0)
    v = np.where(inside[..., None], v, 0.0)
    out = (v - 0.5) / 0.5 if normalize else v
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def rotate(p, cos_a, sin_a):
    """the four-tap rotation of p [C, ps, ps] about its centre, zero fill; cos_a, sin_a as the kernel gets them"""
    c, ps, _ = p.shape
    ca, sa = float(cos_a), float(sin_a)
    cx = cy = (ps - 1) / 2.0
    i, j = np.meshgrid(np.arange(ps, dtype=np.float64), np.arange(ps, dtype=np.float64), indexing='ij')
    sx = cx + ca * (j - cx) - sa * (i - cy)
    sy = cy + sa * (j - cx) + ca * (i - cy)
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    fx, fy = sx - x0, sy - y0
    out = np.zeros_like(p)
    for ty, tx, wt in ((y0, x0, (1 - fy) * (1 - fx)), (y0, x0 + 1, (1 - fy) * fx),
                       (y0 + 1, x0, fy * (1 - fx)), (y0 + 1, x0 + 1, fy * fx)):
        inside = (ty >= 0) & (ty < ps) & (tx >= 0) & (tx < ps)  # a tap outside the patch contributes 0
        out += np.where(inside, wt, 0.0) * p[:, np.clip(ty, 0, ps - 1), np.clip(tx, 0, ps - 1)]
    return out


def cos_sin_f32(angle_deg):
    """what the host hands the kernel: float64 cos / sin of the angle, rounded once to float32"""
    a = np.deg2rad(np.float64(angle_deg))
    return np.float32(np.cos(a)), np.float32(np.sin(a))


def batch(pool, tile, y0, x0, ps, angle=None, seed=0, noise_std=0.0, normalize=False, sample_base=0, tile_hw=None):
    """float64 [n, C, ps, ps]"""
    out = []
    for s in range(len(tile)):
        p = patch(pool, int(tile[s]), int(y0[s]), int(x0[s]), ps, sample_base + s, seed, noise_std, normalize, tile_hw)
        if angle is not None:
            p = rotate(p, *cos_sin_f32(angle[s]))
        out.append(p)
    return np.stack(out)
