"""Host side of sparse slides (cnn_autoencoder_amd/tissue.py: fill_from_histogram, fill_sse; csrc/cae_tiles.hip: the
refusals of cae_tile_byte_hist, which all return before any launch; zarrio.compress_image: the arguments it refuses before
any device work).  The reference of the two host functions is brute force over all 256 fill values in Python integers.
No test here needs a GPU.
"""
import os
import re
import sys

import numpy as np
import pytest
import torch

TILE_SYMBOLS = ('cae_tile_byte_hist', 'cae_tile_byte_hist_workspace', 'cae_tile_byte_hist_blocks')


def brute(cnt):
    """(fill, sse) of 256 counts: every f tried, the first of the smallest kept"""
    cnt = [int(k) for k in cnt]
    sse = [sum(k * (v - f) ** 2 for v, k in enumerate(cnt)) for f in range(256)]
    return sse.index(min(sse)), min(sse)


def brute_sse(hist, f):
    return [sum(int(k) * (v - f) ** 2 for v, k in enumerate(row)) for row in hist]


# ---------------------------------------------------------------------------------------------- the host functions
def test_fill_and_sse_of_random_histograms():
    from cnn_autoencoder_amd import tissue
    rng = np.random.default_rng(0)
    for k in range(40):
        hist = rng.integers(0, 5000, (int(rng.integers(1, 6)), 256))
        hist[:, rng.random(256) < rng.choice([0.0, 0.5, 0.97])] = 0
        fill, sse = tissue.fill_from_histogram(hist)
        assert (fill, sse) == brute(hist.sum(axis=0)), k
        assert isinstance(fill, int) and isinstance(sse, int)
        for f in (0, fill, 255, int(rng.integers(0, 256))):
            got = tissue.fill_sse(hist, f)
            assert got.dtype == np.int64 and got.shape == (hist.shape[0],)
            assert got.tolist() == brute_sse(hist, f), (k, f)
        assert int(tissue.fill_sse(hist, fill).sum()) == sse
        # a tensor, one histogram and a stack of one are read alike
        assert tissue.fill_from_histogram(torch.from_numpy(hist)) == (fill, sse)
        assert tissue.fill_from_histogram(hist.sum(axis=0)) == (fill, sse)
        assert tissue.fill_from_histogram(hist.sum(axis=0)[None]) == (fill, sse)


def test_one_bin_a_tie_and_nothing():
    from cnn_autoencoder_amd import tissue
    one = np.zeros((1, 256), dtype=np.int64)
    one[0, 240] = 12345
    assert tissue.fill_from_histogram(one) == (240, 0)
    assert tissue.fill_sse(one, 238).tolist() == [12345 * 4]
    for lo, hi in ((10, 11), (0, 255), (100, 103)):  # equal counts at lo and hi: every f of the middle pair ties
        tie = np.zeros((2, 256), dtype=np.int64)
        tie[0, lo], tie[1, hi] = 7, 7
        fill, sse = tissue.fill_from_histogram(tie)
        assert (fill, sse) == brute(tie.sum(axis=0))
        assert fill == (lo + hi) // 2 and sse == 7 * ((fill - lo) ** 2 + (hi - fill) ** 2)
        assert brute_sse(tie.sum(axis=0)[None], fill + 1)[0] == sse  # the tie is real, and the lower f is taken
    assert tissue.fill_from_histogram(np.zeros((3, 256), dtype=np.int64)) == (0, 0)
    assert tissue.fill_from_histogram(np.zeros((0, 256), dtype=np.int64)) == (0, 0)
    assert tissue.fill_sse(np.zeros((3, 256), dtype=np.int64), 9).tolist() == [0, 0, 0]
    assert tissue.fill_sse(np.zeros((0, 256), dtype=np.int64), 9).shape == (0,)


def test_counts_near_two_to_the_forty_stay_exact():
    """products of such counts with (v - f)^2 and their sums leave 53 bits, and the sum over tiles leaves 63"""
    from cnn_autoencoder_amd import tissue
    hist = np.zeros((3, 256), dtype=np.int64)
    hist[0, 3], hist[0, 250] = 2 ** 40 + 1, 2 ** 40 - 3
    hist[1, 249], hist[1, 251] = 2 ** 40 + 7, 2 ** 39 + 5
    hist[2, 0], hist[2, 255], hist[2, 128] = 2 ** 40 - 1, 2 ** 40 + 11, 3
    fill, sse = tissue.fill_from_histogram(hist)
    assert (fill, sse) == brute(hist.sum(axis=0)) and sse > 2 ** 53
    for f in (fill, 1, 254):
        want = brute_sse(hist, f)
        assert tissue.fill_sse(hist, f).tolist() == want
        assert any(w % 2 for w in want) and max(want) > 2 ** 53  # not representable as float64: nothing was rounded
    big = np.full((1, 256), 2 ** 40, dtype=np.int64)  # 2^40 x sum (v - 0)^2 = 2^40 x 5 559 680 > 2^62: the sum of all
    assert tissue.fill_from_histogram(np.concatenate([big] * 4)) == brute(4 * big[0])  # four tiles leaves int64
    with pytest.raises(OverflowError):
        tissue.fill_sse(4 * big, 0)


def test_the_host_functions_refuse_what_is_no_histogram():
    from cnn_autoencoder_amd import tissue
    good = np.ones((2, 256), dtype=np.int64)
    for bad in (good.astype(np.float64), np.ones((2, 255), dtype=np.int64), np.ones((2, 2, 256), dtype=np.int64), -good):
        with pytest.raises(ValueError, match='histogram'):
            tissue.fill_from_histogram(bad)
        with pytest.raises(ValueError, match='histogram'):
            tissue.fill_sse(bad, 3)
    with pytest.raises(ValueError, match='histogram'):
        tissue.fill_sse(good[0], 3)
    for f in (-1, 256, 1.5, True):
        with pytest.raises(ValueError, match='fill value'):
            tissue.fill_sse(good, f)


# ------------------------------------------------------------------------------------------------------- the ABI
def test_the_new_symbols_are_declared_and_bound(built_lib):
    from cnn_autoencoder_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, 'include', 'cae_hip.h')).read()
    declared = set(re.findall(r'\b(cae_[a-z0-9_]+)\s*\(', hdr))
    L = _lib.lib()
    for name in TILE_SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS, name
        assert getattr(L, name).argtypes is not None


def test_workspace_and_block_queries(built_lib):
    from cnn_autoencoder_amd import _lib
    L = _lib.lib()
    blocks, need = L.cae_tile_byte_hist_blocks, L.cae_tile_byte_hist_workspace
    for shape in ((0, 4, 4, 3), (-1, 4, 4, 3), (1, 0, 4, 3), (1, 4, 0, 3), (1, 4, 4, 0), (1, 4, 4, 5), (1, -3, 4, 1),
                  (1, 1 << 30, 1 << 30, 1), (2, 2 ** 31 - 1, 2 ** 31 - 1, 4)):
        assert blocks(*shape) == 0 and need(*shape) == 0, shape
    for n in (1, 3, 32, 5000):
        last = 0
        for h, w, c in ((1, 1, 1), (7, 9, 3), (16, 16, 3), (50, 100, 4), (264, 265, 3), (512, 512, 3), (1024, 1024, 3),
                        (4096, 4096, 4), (1 << 16, 1 << 15, 1)):
            bx = blocks(n, h, w, c)
            assert bx >= 1 and bx >= last, (n, h, w, c)  # monotone in the bytes of a tile
            assert n * bx <= max(n, 2048)                # the cap of a launch
            assert need(n, h, w, c) == n * bx * 256 * 4
            last = bx
    assert blocks(3, 264, 265, 3) >= 2                       # several blocks per tile in the tests' largest small shape
    assert blocks(1, 4096, 4096, 4) == 2048 and blocks(3, 1400, 1400, 3) == 2048 // 3  # the cap
    assert blocks(1, 1 << 20, 1 << 20, 4) == 2048            # 2^42 bytes: spans of 2^31
    assert blocks(1, 1 << 21, 1 << 20, 4) == 0               # 2^43 bytes: a span would reach 2^32, the end of a 32-bit count


def test_abi_refuses_without_a_device(built_lib):
    """bad arguments are refused before anything touches a device; n == 0 is nothing to do"""
    from cnn_autoencoder_amd import _lib
    L = _lib.lib()
    p = 1 << 20  # a pointer-like value that is aligned to everything; never dereferenced: every call here is refused
    big = 1 << 40
    hist = lambda t=p, e=None, n=1, h=4, w=4, c=3, out=p, ws=p, nbytes=big: L.cae_tile_byte_hist(  # noqa: E731
        t, e, n, h, w, c, out, ws, nbytes, None)
    assert hist(n=0) == 0 and hist(n=0, t=None, out=None, ws=None, nbytes=0) == 0
    need = L.cae_tile_byte_hist_workspace(1, 4, 4, 3)
    assert need == 1024
    for kw in (dict(n=-1), dict(h=0), dict(w=0), dict(h=-2), dict(c=0), dict(c=5), dict(h=1 << 30, w=1 << 30, c=1),
               dict(t=None), dict(out=None), dict(ws=None), dict(nbytes=0), dict(nbytes=need - 1), dict(out=p + 4),
               dict(ws=p + 8), dict(e=p + 2)):
        assert hist(**kw) == -1, kw
        assert b'cae_tile_byte_hist' in L.cae_last_error()
    assert hist(n=0, c=5) == -1 and hist(n=0, h=0) == -1  # a bad shape is a bad shape with no tiles too
    assert b'channels' in L.cae_last_error() or b'shape' in L.cae_last_error()


def test_the_new_kernel_uses_no_scratch(built_lib):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import scratch_check
    table = {k: v for k, v in scratch_check.kernel_table(built_lib).items() if 'tile_byte_hist_kernel' in k}
    assert len(table) == 1, sorted(table)  # (its second launch: seg_histsum_kernel, held to this by tests/test_seg_roc_host.py)
    assert all(v == (0, 0) for v in table.values()), table


# ---------------------------------------------------------------------------------------------- the Python surface
def test_tile_histograms_refuses_bad_arguments():
    from cnn_autoencoder_amd import tissue
    tiles = torch.zeros((2, 8, 9, 3), dtype=torch.uint8)
    for bad in (tiles, tiles.numpy(), tiles.permute(0, 2, 1, 3)):  # host tensors and arrays: there is no CPU path
        with pytest.raises(ValueError, match='on the device'):
            tissue.tile_histograms(bad)
    for bad, what in ((tiles[0], 'N,H,W,C'), (tiles.float(), 'uint8'), (tiles.to(torch.int32), 'uint8'),
                      (torch.zeros((2, 8, 9, 5), dtype=torch.uint8), 'channels'),
                      (torch.zeros((2, 0, 9, 3), dtype=torch.uint8), 'empty')):
        with pytest.raises(ValueError, match=what):
            tissue.tile_histograms(bad)


def test_compress_image_refuses_before_any_device_work(tmp_path, monkeypatch):
    from cnn_autoencoder_amd import zarrio
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    img = np.full((100, 130, 3), 240, dtype=np.uint8)
    mask = np.zeros((4, 5), dtype=bool)
    out = str(tmp_path / 'x.zarr')
    ckpt = str(tmp_path / 'nothing.pth')  # never opened: every call here is refused first
    call = lambda codec='CAE', **kw: zarrio.compress_image(codec, ckpt, img, out, patch_size=64, **kw)  # noqa: E731
    with pytest.raises(ValueError, match='mask_scale'):
        call(mask=mask)
    for codec, kw in (('Zlib', {}), ('None', {}), ('CAE', dict(save_as_bottleneck=True))):
        with pytest.raises(ValueError, match='pixel codec'):
            call(codec, mask=mask, mask_scale=1 / 32, **kw)
        with pytest.raises(ValueError, match='pixel codec'):
            call(codec, fill_value=240, **kw)
    for bad in (-1, 256, 2.5, True, '240'):
        with pytest.raises(ValueError, match='fill_value'):
            call(mask=mask, mask_scale=1 / 32, fill_value=bad)
    for bad in (-0.5, float('nan'), 'x', True):
        with pytest.raises(ValueError, match='max_fill_rmse'):
            call(mask=mask, mask_scale=1 / 32, max_fill_rmse=bad)
    with pytest.raises(ValueError, match='need a mask'):
        call(mask_scale=1 / 32)
    with pytest.raises(ValueError, match='need a mask'):
        call(max_fill_rmse=2.0)
    with pytest.raises(ValueError, match='scale'):
        call(mask=mask, mask_scale=0.0)
    with pytest.raises(ValueError, match=r'\(Y, X\) mask'):
        call(mask=mask[0], mask_scale=1 / 32)
    with pytest.raises(ValueError, match='channels'):
        zarrio.compress_image('CAE', ckpt, np.zeros((64, 64, 5), np.uint8), out, patch_size=64, fill_value=0)
    assert not os.path.exists(out)
