"""Yardsticks of the metric kernels (tile_sse, tile_ssim, tile_delta_e, msssim_level, u8hwc_to_planes and their reduce
kernels in csrc/cae_kernels.hpp), the inputs of their tests, and emulations of the kernels that can plant defects, so that
CPU tests can show which defects the allowances of test_metrics_kernels.py reject.

* ``ssim_exact``: the five 7x7 window sums as exact integers (int64 summed-area tables), then skimage's formula in
  float64; returns the tile mean and mean|map|, the scale of the SSIM allowance (a tile mean near zero says nothing
  about the size of its summands).
* ``level_maps``: the per-pixel ssim and cs maps of one MS-SSIM scale in float32 or float64 (msssim_restatement's
  formula with the 11-tap window and data range 255); ``level_allowance`` pools |map32 - map64| over a whole case.
* ``emulate_level_fp32``: numpy float32 in the order msssim_level_kernel works in (vertical pass with sequential adds,
  horizontal pass, index in float32, mean in float64), with the defects of LEVEL_DEFECTS.
* delta-E is judged against oracle.cae_oracle.delta_cielab_uint8 and the SSE against numpy int64; only their inputs are
  here.

A helper module, not a test file and not a conftest.
"""
import functools

import numpy as np
import torch

import msssim_restatement as R

# ---- SSIM -------------------------------------------------------------------------------------------------------------
SSIM_RTOL = 1e-12  # of mean|map|, per tile
SSIM_SHAPES = ((2, 7, 7, 1), (1, 7, 45, 3), (1, 45, 7, 3), (2, 38, 38, 3), (3, 39, 40, 4), (2, 70, 101, 1))
SSIM_PAIRS = ('decorrelated', 'pm12', 'identical', 'flat', 'black_white', 'checkerboard')
SSIM_DEFECTS = ('window6', 'population', 'last_block_column', 'tile0')


def _box_sums(a, wy, wx):
    """exact sums of every wy x wx window of the int64 (H, W) array a -> (H - wy + 1, W - wx + 1)"""
    s = np.zeros((a.shape[0] + 1, a.shape[1] + 1), dtype=np.int64)
    s[1:, 1:] = a.cumsum(0).cumsum(1)
    return s[wy:, wx:] - s[:-wy, wx:] - s[wy:, :-wx] + s[:-wy, :-wx]


def ssim_map_exact(a, b, defect=None):
    """SSIM map (h - 6, w - 6) of two uint8 (h, w) planes: exact window sums, skimage's formula in float64"""
    a, b = a.astype(np.int64), b.astype(np.int64)
    ow = a.shape[1] - 6
    wx = 6 if defect == 'window6' else 7  # the defect: the horizontal sum stops one tap early
    s = [_box_sums(q, 7, wx)[:, :ow] for q in (a, b, a * a, b * b, a * b)]
    cov_norm = 1.0 if defect == 'population' else 49.0 / 48.0
    c1, c2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
    ux, uy = s[0] / 49.0, s[1] / 49.0
    vx, vy, vxy = cov_norm * (s[2] / 49.0 - ux * ux), cov_norm * (s[3] / 49.0 - uy * uy), cov_norm * (s[4] / 49.0 - ux * uy)
    return ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))


def ssim_exact(x, y, defect=None):
    """(mean SSIM, mean |SSIM map|) of two uint8 (h, w, c) tiles, over all channels and valid pixels"""
    maps = np.stack([ssim_map_exact(x[..., c], y[..., c], defect) for c in range(x.shape[2])])
    scale = float(np.abs(maps).mean())
    if defect == 'last_block_column':  # the 32-wide block column that holds the last output is left out of the sum
        maps = maps[..., :(maps.shape[2] - 1) // 32 * 32]
        return float(maps.sum() / (x.shape[2] * (x.shape[0] - 6) * (x.shape[1] - 6))), scale
    return float(maps.mean()), scale


def ssim_exact_batch(x, y, defect=None):
    """ssim_exact per tile of two (n, h, w, c) batches -> (means [n], scales [n]); 'tile0' reads every tile's pixels
    from tile 0 (a tile stride that is lost), the others are ssim_exact's"""
    if defect == 'tile0':
        res = [ssim_exact(x[0], y[0])] * len(x)
    else:
        res = [ssim_exact(a, b, defect) for a, b in zip(x, y)]
    return np.array([r[0] for r in res]), np.array([r[1] for r in res])


@functools.lru_cache(maxsize=None)
def ssim_pair(shape, kind):
    """the committed (x, y) uint8 (n, h, w, c) inputs of a case, read-only; the content differs per tile and per channel
    wherever the kind allows it (black against white and the checkerboard are the same in every tile and channel)"""
    n, h, w, c = shape
    rng = np.random.default_rng([SSIM_PAIRS.index(kind), n, h, w, c])
    if kind == 'decorrelated':
        x, y = rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8)
    elif kind == 'pm12':
        x = rng.integers(0, 256, shape, dtype=np.uint8)
        y = np.clip(x.astype(int) + rng.integers(-12, 13, shape), 0, 255).astype(np.uint8)
    elif kind == 'identical':
        x = rng.integers(0, 256, shape, dtype=np.uint8)
        y = x.copy()
    elif kind == 'flat':  # 200 against 201 in tile 0 / channel 0, one level lower per further tile and channel
        x = np.empty(shape, dtype=np.uint8)
        x[...] = 200 - 7 * np.arange(n)[:, None, None, None] - np.arange(c)
        y = x + 1
    elif kind == 'black_white':
        x, y = np.zeros(shape, dtype=np.uint8), np.full(shape, 255, dtype=np.uint8)
    else:
        x = np.empty(shape, dtype=np.uint8)
        x[...] = (255 * ((np.arange(h)[:, None] + np.arange(w)) % 2))[None, :, :, None]
        y = 255 - x
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


# ---- one MS-SSIM scale -------------------------------------------------------------------------------------------------
LEVEL_SHAPES = ((8, 11, 11), (8, 11, 12), (8, 13, 11), (2, 42, 42), (3, 43, 44), (2, 12, 75), (2, 75, 12), (4, 80, 107))
LEVEL_RECIPES = ('decorrelated', 'half_equal', 'quarters', 'identical', 'bright_flat')
LEVEL_INDEX_RECIPES = LEVEL_RECIPES[:3]  # the decorrelated ones: what index errors are judged on
LEVEL_DEFECTS = ('edge_column', 'dropped_row', 'dropped_tap', 'swapped_constants', 'cs_in_ssim_slot')
LEVEL_FACTOR, LEVEL_FLOOR = 16.0, 2.0 ** -22


def window11(dtype=torch.float32):
    return R.window(11, 1.5, dtype)


def level_maps(X, Y, dtype):
    """(ssim map, cs map), each (planes, h - 10, w - 10) torch tensors of `dtype`, of two (planes, h, w) arrays"""
    X, Y = (torch.as_tensor(np.array(t)).to(dtype)[None] for t in (X, Y))  # (a copy: the cases are read-only)
    ssim_map, cs_map = R.level_maps(X, Y, window11(dtype), (0.01 * 255) ** 2, (0.03 * 255) ** 2)
    return ssim_map[0], cs_map[0]


def level_reference(X, Y):
    """-> (float64 means (planes, 2) [ssim, cs], allowance [2]): the allowance of quantity q is 16 E_q + 2^-22 with E_q
    the mean of |map32_q - map64_q| over every output pixel of every plane of the case"""
    m64, m32 = level_maps(X, Y, torch.float64), level_maps(X, Y, torch.float32)
    ref = np.stack([m.flatten(1).mean(1).numpy() for m in m64], axis=1)
    allow = np.array([LEVEL_FACTOR * float((a.double() - b).abs().mean()) + LEVEL_FLOOR for a, b in zip(m32, m64)])
    return ref, allow


def emulate_level_fp32(X, Y, defect=None):
    """msssim_level_kernel + msssim_reduce_kernel in numpy float32 -> (planes, 2) float64 [mean ssim, mean cs]"""
    X, Y = np.asarray(X, dtype=np.float32), np.asarray(Y, dtype=np.float32)
    g = window11(torch.float32).numpy()
    planes, h, w = X.shape
    oh, ow = h - 10, w - 10
    q = np.stack([X, Y, X * X, Y * Y, X * Y])
    v = np.zeros((5, planes, oh, w), dtype=np.float32)
    for k in range(11):  # rows first
        v += g[k] * q[:, :, k:k + oh, :]
    m = np.zeros((5, planes, oh, ow), dtype=np.float32)
    for k in range(11):
        if defect == 'dropped_tap' and k == 10:  # a loop bound one short
            continue
        m += g[k] * v[..., k:k + ow]
    if defect == 'edge_column' and ow > 32:
        # output column 32, the first of the second block, takes its window from columns 33.. (zeros past the image,
        # as the kernel's staging fills them)
        vp = np.concatenate([v, np.zeros((5, planes, oh, 1), dtype=np.float32)], axis=-1)
        col = np.zeros((5, planes, oh), dtype=np.float32)
        for k in range(11):
            col += g[k] * vp[..., 33 + k]
        m[..., 32] = col
    c1 = (np.float32(0.01) * np.float32(255)) * (np.float32(0.01) * np.float32(255))
    c2 = (np.float32(0.03) * np.float32(255)) * (np.float32(0.03) * np.float32(255))
    if defect == 'swapped_constants':
        c1, c2 = c2, c1
    two = np.float32(2)
    mu1, mu2 = m[0], m[1]
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = m[2] - mu1_sq, m[3] - mu2_sq, m[4] - mu12
    cs = (two * s12 + c2) / (s1 + s2 + c2)
    ss = ((two * mu12 + c1) / (mu1_sq + mu2_sq + c1)) * cs
    assert cs.dtype == np.float32 and ss.dtype == np.float32
    if defect == 'dropped_row':  # `<` for `<=` in the row validity test: the last row never enters the sum
        ss, cs = ss[:, :-1], cs[:, :-1]
    out = np.stack([ss.astype(np.float64).sum((1, 2)), cs.astype(np.float64).sum((1, 2))], axis=1) / (oh * ow)
    if defect == 'cs_in_ssim_slot':
        out[:, 0] = out[:, 1]
    return out


def level_defect_reachable(defect, shape):
    """the edge-column defect needs a second block column (more than 32 output columns); the others act at every shape"""
    return defect != 'edge_column' or shape[2] - 10 > 32


@functools.lru_cache(maxsize=None)
def level_case(shape, recipe):
    """the committed float32 (X, Y) planes of a case, read-only, distinct per plane"""
    rng = np.random.default_rng([100 + LEVEL_RECIPES.index(recipe), *shape])
    if recipe == 'decorrelated':
        x, y = rng.integers(0, 256, shape), rng.integers(0, 256, shape)
    elif recipe == 'half_equal':
        x, y = rng.integers(0, 256, shape), rng.integers(0, 256, shape)
        y = np.where(rng.integers(0, 2, shape) == 1, x, y)
    elif recipe == 'quarters':  # what cae_avgpool2 hands to level 1
        x, y = rng.integers(0, 1021, shape) / 4.0, rng.integers(0, 1021, shape) / 4.0
    elif recipe == 'identical':
        x = rng.integers(0, 256, shape)
        y = x
    else:  # bright and nearly flat: float32 cancellation in the variances, no index error is judged on it
        x = 240 + rng.integers(-3, 4, shape)
        y = x + rng.integers(-2, 3, shape)
    x, y = x.astype(np.float32), y.astype(np.float32)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def level_case_reference(shape, recipe):
    ref, allow = level_reference(*level_case(shape, recipe))
    ref.setflags(write=False)
    allow.setflags(write=False)
    return ref, allow


# ---- delta-E inputs ----------------------------------------------------------------------------------------------------
DELTA_E_RTOL = 1e-11
DELTA_E_PIXELS = (1, 255, 256, 257, 32768, 32769)
DELTA_E_KINDS = ('cube', 'grey', 'primaries', 'random1', 'random60', 'identical')


@functools.lru_cache(maxsize=None)
def delta_e_pair(kind, n, pixels):
    """the committed (x, y) uint8 (n, pixels, 3) inputs, read-only, distinct per tile.  'cube' is every (r, g, b) of the
    levels 0..31 (every combination of the f(t) branches around 0.008856: a grey of level 31 has t = 0.0137, one of level
    23 has t = 0.0086) against the same colour one level up in channel tile % 3; it needs 32768 pixels, and further pixels
    are random."""
    rng = np.random.default_rng([DELTA_E_KINDS.index(kind), n, pixels])
    x = rng.integers(0, 256, (n, pixels, 3), dtype=np.uint8)
    if kind == 'cube':
        assert pixels >= 32768
        lv = np.arange(32, dtype=np.uint8)
        cube = np.stack(np.meshgrid(lv, lv, lv, indexing='ij'), axis=-1).reshape(-1, 3)
        y = np.clip(x.astype(int) + rng.integers(-60, 61, x.shape), 0, 255).astype(np.uint8)
        for t in range(n):
            x[t, :32768] = np.roll(cube, 977 * t, axis=0)  # another pixel order per tile
            y[t, :32768] = x[t, :32768]
            y[t, :32768, t % 3] += 1
    elif kind == 'grey':  # all 256 levels (from 256 pixels on), against the level t + 1 further on
        i = np.arange(pixels)
        for t in range(n):
            x[t] = ((i + 5 * t) % 256)[:, None]
        y = ((x.astype(int) + 1 + np.arange(n)[:, None, None]) % 256).astype(np.uint8)
    elif kind == 'primaries':  # the 8 corners of the cube against the corner t + 1 further on
        corners = 255 * np.array([[b >> 2 & 1, b >> 1 & 1, b & 1] for b in range(8)], dtype=np.uint8)
        i = np.arange(pixels)
        y = np.empty_like(x)
        for t in range(n):
            x[t] = corners[(i + t) % 8]
            y[t] = corners[(i + 2 * t + 1) % 8]
    elif kind in ('random1', 'random60'):
        amp = int(kind[6:])
        y = np.clip(x.astype(int) + rng.integers(-amp, amp + 1, x.shape), 0, 255).astype(np.uint8)
    else:
        y = x.copy()
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y
