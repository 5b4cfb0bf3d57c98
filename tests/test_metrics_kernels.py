"""The metric kernels (csrc/cae_kernels.hpp: tile_sse, tile_ssim, tile_delta_e, msssim_level, u8hwc_to_planes and their
reduce kernels) one by one through the C entry points, on caller-owned buffers of exactly the documented size between
sentinels, at the smallest shapes where their indexing changes, against exact or float64 references
(metrics_restatement.py).  The CPU tests show that each allowance accepts a faithful emulation of its kernel and rejects
the defects planted into it.

Allowances (none comes from what the kernels give):
  tile_sse, u8hwc_to_planes  equality.
  tile_ssim      |got - ssim_exact| <= 1e-12 * mean|map| per tile (the project's 1e-12, on the scale of the summands so
                 that a tile mean near zero neither empties nor breaks the test); identical tiles give exactly 1.0.
  tile_delta_e   rtol 1e-11 against oracle.cae_oracle.delta_cielab_uint8 (non-negative summands); identical tiles 0.0.
  msssim_level   per plane and quantity q in {ssim, cs}: 16 E_q + 2^-22, E_q = the mean of |map32_q - map64_q| over
                 every output pixel of every plane of the case; X == Y gives exactly (1.0, 1.0).  The faithful float32
                 emulation stays below 0.5 of it on every committed input (worst 0.16).
  compute_ms_ssim  rtol 2e-5 against msssim_restatement.ms_ssim in float64.

What the defects cannot reach: the shifted block-edge column needs more than 32 output columns, so of the level shapes
only (3,43,44), (2,12,75) and (4,80,107); 'tile0' (every tile read from tile 0) needs a second tile, so not (1,7,45,3)
and (1,45,7,3).  Index defects are judged on the decorrelated recipes: on X == Y every window gives 1.0 wherever it
sits, and the bright, nearly flat pair (240 +- 3 against +- 2 more) has E_q about 1e-4 from float32 cancellation in the
variances -- it is there to show that the kernel gives no NaN and nothing wild, not to catch an index error.  For SSIM
the defects are judged on the decorrelated and the +-12 pairs: flat, black/white and identical pairs have zero variance
or identical windows, which the population-covariance and window defects do not change.

Worst err / allowance seen on an MI355X (CAE_TEST_VERBOSE=1 prints every one): tile_ssim 0.00044 ((3,39,40,4), flat),
tile_delta_e 0.0054 (one random pixel pair at amplitude 1, n = 3; the dark-colour cube 1.9e-5), msssim_level 0.15 for
ssim and for cs ((8,11,12), quarters; the emulation gives 0.11 there), compute_ms_ssim 0.12 ((2,161,161,3)),
compute_psnr / compute_rmse 0 (equal to the float64 formula).

The exactness cases found three defects, all of one kind -- the compiler's choice of where to fuse a multiply into an
add -- and the kernels now pin that choice: tile_ssim gave 1 - 1 ulp for a single-window identical pair ((2,7,7,1)),
tile_delta_e gave about 1e-15 instead of 0 for identical tiles at every size, and msssim_level gave 1 +- 4e-7 for X == Y
(2.75 of the allowance where a plane has a single output pixel), because the filtered x y was accumulated with separate
multiplies and adds while x x and y y were fused.
"""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import metrics_restatement as M
import msssim_restatement as R
from oracle import cae_oracle as O

ARG = -1
GUARD = 8
SENTINEL = -777.25
VERBOSE = bool(os.environ.get('CAE_TEST_VERBOSE'))


def _note(kernel, case, ratio):
    if VERBOSE:
        print(f'{kernel} {case}: err / allowance = {ratio:.3g}')


# ======================================================================================================================
# CPU: the references and what their allowances accept and reject
# ======================================================================================================================
@pytest.mark.parametrize('shape', M.SSIM_SHAPES)
def test_ssim_exact_anchors_to_the_oracle(shape):
    """ssim_exact (exact integer window sums) and oracle.cae_oracle.ssim_uint8 (scipy's running-sum filter in float64) are
    two statements of one formula: they agree within the SSIM allowance on every committed pair"""
    for kind in M.SSIM_PAIRS:
        x, y = M.ssim_pair(shape, kind)
        ref, scale = M.ssim_exact_batch(x, y)
        got = np.array([O.ssim_uint8(a, b) for a, b in zip(x, y)])
        ratio = float((np.abs(got - ref) / (M.SSIM_RTOL * scale)).max())
        _note('ssim oracle', (shape, kind), ratio)
        assert ratio <= 1.0, (shape, kind, ratio)
        if kind == 'identical':
            assert (ref == 1.0).all()
        if kind == 'checkerboard':
            assert (np.abs(ref + 0.996) < 1e-3).all()


@pytest.mark.parametrize('shape', M.SSIM_SHAPES)
def test_ssim_allowance_rejects_planted_defects(shape):
    """a 6-wide window in x, population covariance, the last block column left out of the sum and every tile read from
    tile 0 each miss the allowance on every tile they can reach (tile0: every tile but the first)"""
    for kind in ('decorrelated', 'pm12'):
        x, y = M.ssim_pair(shape, kind)
        ref, scale = M.ssim_exact_batch(x, y)
        for defect in M.SSIM_DEFECTS:
            got, _ = M.ssim_exact_batch(x, y, defect)
            ratio = np.abs(got - ref) / (M.SSIM_RTOL * scale)
            reached = ratio[1:] if defect == 'tile0' else ratio
            _note('ssim defect', (shape, kind, defect), float(reached.min()) if len(reached) else float('nan'))
            assert (reached > 1.0).all(), (shape, kind, defect, ratio)
            if defect == 'tile0':
                assert ratio[0] == 0.0


def test_level_maps_means_equal_the_restatement():
    for shape in ((8, 11, 12), (3, 43, 44)):
        for recipe in ('decorrelated', 'quarters'):
            X, Y = M.level_case(shape, recipe)
            for dtype in (torch.float32, torch.float64):
                ssim_map, cs_map = M.level_maps(X, Y, dtype)
                assert ssim_map.dtype == dtype and tuple(cs_map.shape) == (shape[0], shape[1] - 10, shape[2] - 10)
                Xt, Yt = torch.from_numpy(X.copy()).to(dtype)[None], torch.from_numpy(Y.copy()).to(dtype)[None]
                ssim, cs = R.level(Xt, Yt, R.window(11, 1.5, dtype), (0.01 * 255) ** 2, (0.03 * 255) ** 2)
                assert torch.equal(ssim_map.flatten(1).mean(1), ssim[0]) and torch.equal(cs_map.flatten(1).mean(1), cs[0])


@pytest.mark.parametrize('shape', M.LEVEL_SHAPES)
def test_level_allowance_accepts_the_faithful_emulation(shape):
    """the float32 emulation of msssim_level_kernel stays at or below half the allowance on every committed input"""
    for recipe in M.LEVEL_RECIPES:
        X, Y = M.level_case(shape, recipe)
        ref, allow = M.level_case_reference(shape, recipe)
        got = M.emulate_level_fp32(X, Y)
        ratio = float((np.abs(got - ref) / allow).max())
        _note('level emulation', (shape, recipe), ratio)
        assert ratio <= 0.5, (shape, recipe, ratio)
        if recipe == 'identical':
            assert (got == 1.0).all() and (ref == 1.0).all()


@pytest.mark.parametrize('shape', M.LEVEL_SHAPES)
def test_level_allowance_rejects_planted_defects(shape):
    """each defect, at each shape it can reach and on each decorrelated recipe, puts a plane outside the allowance; where
    it cannot reach the emulation is unchanged"""
    for recipe in M.LEVEL_INDEX_RECIPES:
        X, Y = M.level_case(shape, recipe)
        ref, allow = M.level_case_reference(shape, recipe)
        for defect in M.LEVEL_DEFECTS:
            got = M.emulate_level_fp32(X, Y, defect)
            if not M.level_defect_reachable(defect, shape):
                assert np.array_equal(got, M.emulate_level_fp32(X, Y))
                continue
            ratio = np.abs(got - ref) / allow
            _note('level defect', (shape, recipe, defect), float(ratio.max()))
            assert ratio.max() > 1.0, (shape, recipe, defect, ratio)
            if defect == 'cs_in_ssim_slot':
                assert ratio[:, 1].max() <= 0.5  # the cs slot itself is right: the ssim slot is what is judged
            if defect == 'dropped_tap':
                assert (ratio > 1.0).all()  # every plane, both outputs


def test_bad_arguments_are_refused_before_any_launch(built_lib):
    """every call here is CAE_ERR_ARG with a message and returns before any HIP call: the pointers are not device memory"""
    from cnn_autoencoder_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(4096)

    def ssim(n=2, h=39, w=40, c=3, ws=8):  # 2 x 2 blocks per tile
        return L.cae_tile_ssim(p, p, n, h, w, c, p, p, ws, None)

    def delta_e(n=3, pixels=257, ws=6):  # 2 blocks per tile
        return L.cae_tile_delta_e(p, p, n, pixels, p, p, ws, None)

    def level(planes=3, h=43, w=44, ws=24):  # 2 x 2 blocks per plane, two doubles each
        return L.cae_msssim_level(p, p, planes, h, w, p, p, p, ws, None)

    def sse(n=2, elems=100):
        return L.cae_tile_sse(p, p, n, elems, p, None)

    def planes(n=2, h=5, w=7, c=3):
        return L.cae_u8hwc_to_planes(p, n, h, w, c, p, None)

    refused = [(ssim, dict(ws=7), b'8 doubles'), (ssim, dict(ws=0), b'8 doubles'), (ssim, dict(h=6), b'7x7'),
               (ssim, dict(w=6), b'7x7'), (ssim, dict(n=0), b'shape'), (ssim, dict(c=0), b'shape'),
               (ssim, dict(n=65536), b'shape'),
               (delta_e, dict(ws=5), b'6 doubles'), (delta_e, dict(pixels=0), b'shape'), (delta_e, dict(n=0), b'shape'),
               (delta_e, dict(n=65536), b'shape'),
               (level, dict(ws=23), b'24 doubles'), (level, dict(h=10), b'11-tap'), (level, dict(w=10), b'11-tap'),
               (level, dict(planes=0), b'plane count'), (level, dict(planes=65536), b'plane count'),
               (sse, dict(n=0), b'shape'), (sse, dict(elems=0), b'shape'), (sse, dict(n=65536), b'shape'),
               (planes, dict(n=0), b'shape'), (planes, dict(c=0), b'shape'), (planes, dict(h=0), b'shape')]
    for fn, bad, msg in refused:
        assert fn(**bad) == ARG, (fn.__name__, bad)
        assert msg in L.cae_last_error(), (fn.__name__, bad, L.cae_last_error())
    with pytest.raises(ValueError, match='bad shape'):
        _lib.check(sse(n=65536))


# ======================================================================================================================
# GPU
# ======================================================================================================================
@pytest.fixture(scope='module')
def cae(built_lib):
    import cnn_autoencoder_amd as cae
    return cae


class _Guarded:
    """`n` floats of device memory between GUARD sentinel elements on either side; the payload starts as NaN bits, so that
    a cell left unwritten, or an accumulator that is not cleared, shows"""

    def __init__(self, n, dtype=torch.float64):
        self.n = n
        self.whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device='cuda')
        self.view = self.whole[GUARD:GUARD + n]
        self.view.fill_(float('nan'))

    def ptr(self):
        return self.view.data_ptr()

    def result(self):
        """the payload on the host, after checking that the sentinels stand"""
        torch.cuda.synchronize()
        host = self.whole.cpu()
        assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + self.n:] == SENTINEL).all(), 'wrote outside its buffer'
        return host[GUARD:GUARD + self.n].numpy()


def _carve(arr, offset=0):
    """the uint8 array at `offset` bytes into a larger device allocation (torch allocations are 512-byte aligned, so
    `offset` is the address modulo 16) -> (the allocation, to keep alive; the device pointer)"""
    flat = np.ascontiguousarray(arr).reshape(-1)
    whole = torch.full((flat.size + offset + 32,), 0xA5, dtype=torch.uint8, device='cuda')
    assert whole.data_ptr() % 16 == 0
    whole[offset:offset + flat.size].copy_(torch.from_numpy(flat.copy()))
    return whole, whole.data_ptr() + offset


# ---- tile_sse ----------------------------------------------------------------------------------------------------------
SSE_BIG = 2 * 262144 + 3 * 16 + 5  # the 64-block cap, the two-vector loop, the single-vector remainder and the byte tail
SSE_ELEMS = (1, 15, 16, 17, 4095, 4096, 8192 + 37, SSE_BIG)


def _sse_raw(L, _lib, a, b, oa=0, ob=0):
    n, elems = a.shape
    keep_a, pa = _carve(a, oa)
    keep_b, pb = _carve(b, ob)
    out = _Guarded(n)
    _lib.check(L.cae_tile_sse(pa, pb, n, elems, out.ptr(), _lib.stream_ptr()))
    return out.result()


def _sse_ref(a, b):
    return ((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum(1)


@pytest.mark.gpu
@pytest.mark.parametrize('elems', SSE_ELEMS)
def test_tile_sse_is_exact_at_every_size_and_alignment(cae, elems):
    """integer equality with numpy int64: one tile and five (with elems % 16 != 0 tile 0 takes the vector path and later
    tiles the byte path), either or both base pointers 1, 8 or 15 bytes off, an accumulator that starts as NaN bits"""
    from cnn_autoencoder_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(elems)
    offsets = [(0, 0)]
    if elems in (17, 4096, 8192 + 37, SSE_BIG):
        offsets += [(o, 0) for o in (1, 8, 15)] + [(0, o) for o in (1, 8, 15)] + [(o, o) for o in (1, 8, 15)]
    for n in (1, 5):
        a, b = rng.integers(0, 256, (n, elems), dtype=np.uint8), rng.integers(0, 256, (n, elems), dtype=np.uint8)
        want = _sse_ref(a, b)
        for oa, ob in offsets:
            got = _sse_raw(L, _lib, a, b, oa, ob)
            assert got.dtype == np.float64 and np.array_equal(got, want.astype(np.float64)), (n, elems, oa, ob, got, want)
    if elems >= 8192:
        zeros, full = np.zeros((5, elems), dtype=np.uint8), np.full((5, elems), 255, dtype=np.uint8)
        for oa, ob in ((0, 0), (8, 1)):
            assert np.array_equal(_sse_raw(L, _lib, zeros, full, oa, ob), np.full(5, 65025.0 * elems))
            assert np.array_equal(_sse_raw(L, _lib, full, zeros, oa, ob), np.full(5, 65025.0 * elems))
            assert np.array_equal(_sse_raw(L, _lib, a, a, oa, ob), np.zeros(5))


@pytest.mark.gpu
def test_psnr_and_rmse_against_float64(cae):
    """compute_psnr / compute_rmse on two of the SSE sizes (17 and 8192 + 37 bytes per tile), rtol 1e-12 (the project's
    figure for them); an identical tile has RMSE 0 and PSNR inf"""
    from cnn_autoencoder_amd import metrics
    rng = np.random.default_rng(3)
    for shape in ((5, 1, 17, 1), (5, 13, 211, 3)):
        x = rng.integers(0, 256, shape, dtype=np.uint8)
        y = np.clip(x.astype(int) + rng.integers(-20, 21, shape), 0, 255).astype(np.uint8)
        y[2] = x[2]
        mse = _sse_ref(x.reshape(shape[0], -1), y.reshape(shape[0], -1)) / float(np.prod(shape[1:]))
        assert mse[2] == 0.0 and (np.delete(mse, 2) > 0).all()
        xs, ys = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        rmse = metrics.compute_rmse(x=xs, x_r=ys).cpu().numpy()
        psnr = metrics.compute_psnr(x=xs, x_r=ys).cpu().numpy()
        assert rmse[2] == 0.0 and psnr[2] == np.inf
        keep = np.arange(shape[0]) != 2
        want_psnr = 20 * math.log10(255.0) - 10 * np.log10(mse[keep])
        for name, got, want in (('rmse', rmse[keep], np.sqrt(mse[keep])), ('psnr', psnr[keep], want_psnr)):
            ratio = float((np.abs(got - want) / (1e-12 * np.abs(want))).max())
            _note('compute_' + name, shape, ratio)
            assert ratio <= 1.0, (name, shape, ratio)


# ---- u8hwc_to_planes ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('shape', ((2, 5, 7, 1), (3, 9, 4, 3), (1, 33, 17, 4)))
def test_u8hwc_to_planes_is_bit_exact(cae, shape):
    from cnn_autoencoder_amd import _lib
    n, h, w, c = shape
    x = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    keep, px = _carve(x, 3)
    out = _Guarded(n * c * h * w, torch.float32)
    _lib.check(_lib.lib().cae_u8hwc_to_planes(px, n, h, w, c, out.ptr(), _lib.stream_ptr()))
    want = np.ascontiguousarray(np.moveaxis(x, 3, 1)).astype(np.float32).reshape(-1)
    assert np.array_equal(out.result().view(np.uint32), want.view(np.uint32))


# ---- tile_ssim ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('shape', M.SSIM_SHAPES)
def test_tile_ssim_against_exact_window_sums(cae, shape):
    """one output; one row and one column of 39 outputs (two blocks); exactly one 32x32 block; 33x34 outputs (slivers of
    1 and 2); 64x95 -- on a workspace of exactly the documented size and inputs at odd addresses"""
    from cnn_autoencoder_amd import _lib
    n, h, w, c = shape
    bpt = ((h - 6 + 31) // 32) * ((w - 6 + 31) // 32)
    for kind in M.SSIM_PAIRS:
        x, y = M.ssim_pair(shape, kind)
        ref, scale = M.ssim_exact_batch(x, y)
        keep_x, px = _carve(x, 1)
        keep_y, py = _carve(y, 6)
        out, ws = _Guarded(n), _Guarded(n * bpt)
        _lib.check(_lib.lib().cae_tile_ssim(px, py, n, h, w, c, out.ptr(), ws.ptr(), n * bpt, _lib.stream_ptr()))
        got = out.result()
        assert np.isfinite(ws.result()).all()
        ratio = float((np.abs(got - ref) / (M.SSIM_RTOL * scale)).max())
        _note('tile_ssim', (shape, kind), ratio)
        assert ratio <= 1.0, (shape, kind, ratio, got, ref)
        if kind == 'identical':
            assert (got == 1.0).all()


@pytest.mark.gpu
def test_compute_ssim_on_a_crop_view(cae):
    """a non-contiguous crop of a larger batch gives what its contiguous copy gives, and that is right"""
    from cnn_autoencoder_amd import metrics
    rng = np.random.default_rng(17)
    big_x = rng.integers(0, 256, (3, 50, 60, 3), dtype=np.uint8)
    big_y = np.clip(big_x.astype(int) + rng.integers(-12, 13, big_x.shape), 0, 255).astype(np.uint8)
    vx, vy = (torch.from_numpy(t).cuda()[:, 5:44, 7:47, :] for t in (big_x, big_y))
    assert not vx.is_contiguous()
    got = metrics.compute_ssim(x=vx, x_r=vy)
    assert torch.equal(got, metrics.compute_ssim(x=vx.contiguous(), x_r=vy.contiguous()))
    ref, scale = M.ssim_exact_batch(big_x[:, 5:44, 7:47, :], big_y[:, 5:44, 7:47, :])
    assert (np.abs(got.cpu().numpy() - ref) <= M.SSIM_RTOL * scale).all()


# ---- tile_delta_e ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('pixels', M.DELTA_E_PIXELS)
def test_tile_delta_e_against_the_oracle(cae, pixels):
    """one pixel; one block less one, exactly, plus one; exactly the 128-block cap (where the dark-colour cube fits: every
    combination of the f(t) branches) and one pixel more, which sends one thread round its loop again"""
    from cnn_autoencoder_amd import _lib
    bpt = min((pixels + 255) // 256, 128)
    for n in (1, 3):
        for kind in M.DELTA_E_KINDS:
            if kind == 'cube' and pixels < 32768:
                continue
            x, y = M.delta_e_pair(kind, n, pixels)
            ref = np.array([O.delta_cielab_uint8(a[None], b[None]) for a, b in zip(x, y)])
            keep_x, px = _carve(x, 1)
            keep_y, py = _carve(y, 2)
            out, ws = _Guarded(n), _Guarded(n * bpt)
            _lib.check(_lib.lib().cae_tile_delta_e(px, py, n, pixels, out.ptr(), ws.ptr(), n * bpt, _lib.stream_ptr()))
            got = out.result()
            assert np.isfinite(ws.result()).all()
            if kind == 'identical':
                assert (got == 0.0).all() and (ref == 0.0).all()
                continue
            err, allow = np.abs(got - ref), M.DELTA_E_RTOL * ref  # (a single random pixel pair may coincide: 0 <= 0)
            ratio = float((err[allow > 0] / allow[allow > 0]).max()) if (allow > 0).any() else 0.0
            _note('tile_delta_e', (n, pixels, kind), ratio)
            assert (err <= allow).all(), (n, pixels, kind, ratio, got, ref)


# ---- msssim_level ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('shape', M.LEVEL_SHAPES)
def test_msssim_level_both_outputs_against_float64(cae, shape):
    """the ssim and the cs mean of every plane: one output pixel; one row or column of two or three; exactly one block;
    33x34 outputs; two and three blocks in a row or a column; 70x97 outputs"""
    from cnn_autoencoder_amd import _lib
    planes, h, w = shape
    bpp = ((h - 10 + 31) // 32) * ((w - 10 + 31) // 32)
    win = M.window11(torch.float32).cuda()
    for recipe in M.LEVEL_RECIPES:
        X, Y = M.level_case(shape, recipe)
        ref, allow = M.level_case_reference(shape, recipe)
        dx, dy = torch.from_numpy(X.copy()).cuda(), torch.from_numpy(Y.copy()).cuda()
        out, ws = _Guarded(2 * planes), _Guarded(2 * planes * bpp)
        _lib.check(_lib.lib().cae_msssim_level(dx.data_ptr(), dy.data_ptr(), planes, h, w, win.data_ptr(), out.ptr(),
                                               ws.ptr(), 2 * planes * bpp, _lib.stream_ptr()))
        got = out.result().reshape(planes, 2)
        assert np.isfinite(ws.result()).all()
        ratio = (np.abs(got - ref) / allow).max(0)
        _note('msssim_level ssim', (shape, recipe), float(ratio[0]))
        _note('msssim_level cs', (shape, recipe), float(ratio[1]))
        assert ratio.max() <= 1.0, (shape, recipe, ratio, got, ref)
        if recipe == 'identical':
            assert (got == 1.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize('shape', ((2, 161, 161, 3), (1, 161, 177, 1), (1, 178, 161, 4)))
def test_compute_ms_ssim_against_float64(cae, shape):
    """the whole pyramid (161 -> 81 -> 41 -> 21 -> 11: a single output pixel at level 4) against the float64 restatement"""
    from cnn_autoencoder_amd import metrics
    rng = np.random.default_rng(sum(shape))
    x = rng.integers(0, 256, shape, dtype=np.uint8)
    y = np.clip(x.astype(int) + rng.integers(-25, 26, shape), 0, 255).astype(np.uint8)
    got = metrics.compute_ms_ssim(x=torch.from_numpy(x).cuda(), x_r=torch.from_numpy(y).cuda()).cpu().numpy()
    planes = [torch.from_numpy(np.moveaxis(t, 3, 1).copy()) for t in (y, x)]
    ref = np.array([float(R.ms_ssim(planes[0][t:t + 1], planes[1][t:t + 1], data_range=255.0, dtype=torch.float64))
                    for t in range(shape[0])])
    ratio = float((np.abs(got - ref) / (2e-5 * np.abs(ref))).max())
    _note('compute_ms_ssim', shape, ratio)
    assert ratio <= 1.0, (shape, ratio, got, ref)
