"""The tissue mask on the GPU (csrc/cae_mask.hip, cnn_autoencoder_amd/tissue.py): every kernel on its own through the C
ABI, then tissue_mask, downscale and mask_zarr.

Everything is compared for equality with the numpy / scipy restatement (tests/tissue_restatement.py): the gray values
bit for bit (float64, every operation rounded on its own), everything behind them as integers.  Outputs and workspaces
come poisoned from torch.empty (residue.poisoned_alloc), so nothing depends on what a buffer held before the call.
Shapes: (1,1), (7,9), (33,65) and (264,265) -- several blocks both ways, and more pixels than one block of the histogram
counts between two folds of its 32-bit bins -- with up to three planes in a call, which must not mix.
"""
import functools
import os

import numpy as np
import pytest
import torch

import test_seg_objects as TO
import tissue_restatement as R
from residue import poisoned_alloc  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (7, 9), (33, 65), (264, 265)]
PATTERNS = ('antidiagonal', 'grid', 'spiral', 'comb', 'rings', 'empty', 'full')


def _mods():
    from cnn_autoencoder_amd import _lib, segmenters, tissue
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return _lib, _lib.lib(), segmenters, tissue


def dev(arr, offset=0):
    """`arr` on the device, as a view `offset` elements into a larger buffer"""
    flat = torch.from_numpy(np.ascontiguousarray(arr)).reshape(-1)
    buf = torch.zeros(flat.numel() + offset + 16, dtype=flat.dtype, device='cuda')
    view = buf[offset:offset + flat.numel()]
    view.copy_(flat)
    return view.view(arr.shape)


def ws_of(nbytes):
    return torch.empty(max((int(nbytes) + 7) // 8, 1), dtype=torch.int64, device='cuda')


# ---- the entry points on the test's own buffers ---------------------------------------------------------------------
def raw_gray(img):
    _lib, L, _, _ = _mods()
    n, h, w, _ = img.shape
    gray = torch.empty((n, h, w), dtype=torch.float64, device='cuda')
    minmax = torch.empty((n, 2), dtype=torch.float64, device='cuda')
    _lib.check(L.cae_mask_gray(img.data_ptr(), n, h * w, gray.data_ptr(), minmax.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return gray.cpu().numpy(), minmax.cpu().numpy()


def raw_hist(gray, edges):
    _lib, L, _, _ = _mods()
    n, hw = gray.shape
    counts = torch.empty((n, 256), dtype=torch.int64, device='cuda')
    ws = ws_of(L.cae_mask_hist_workspace(n, hw))
    _lib.check(L.cae_mask_hist(gray.data_ptr(), edges.data_ptr(), n, hw, counts.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                               _lib.stream_ptr()))
    torch.cuda.synchronize()
    return counts.cpu().numpy()


def raw_label(plane, conn, of_zero=0):
    _lib, L, _, _ = _mods()
    n, h, w = plane.shape
    labels = torch.empty((n, h, w), dtype=torch.int32, device='cuda')
    ws = ws_of(L.cae_mask_label_workspace(n, h, w))
    _lib.check(L.cae_mask_label(plane.data_ptr(), n, h, w, conn, of_zero, labels.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                _lib.stream_ptr()))
    return labels


def raw_area_filter(labels, plane, least, value, wide=False):
    """-> (plane after the filter, a copy; the int32 plane or None)"""
    _lib, L, _, _ = _mods()
    n, h, w = plane.shape
    out = plane.clone()
    wide_out = torch.empty((n, h, w), dtype=torch.int32, device='cuda') if wide else None
    ws = ws_of(L.cae_mask_area_workspace(n, h, w))
    _lib.check(L.cae_mask_area_filter(labels.data_ptr(), n, h, w, least, value, out.data_ptr(),
                                      None if wide_out is None else wide_out.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                      _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if wide_out is None else wide_out.cpu().numpy()


def raw_dilate(plane, radius):
    _lib, L, S, _ = _mods()
    n, h, w = plane.shape
    d2 = S.object_distances(plane.to(torch.int32))
    out = torch.empty((n, h, w), dtype=torch.uint8, device='cuda')
    _lib.check(L.cae_mask_within(d2.data_ptr(), n, h * w, radius * radius, out.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------- gray, min and max
@pytest.mark.parametrize('shape', SHAPES)
def test_gray_and_its_range(shape, poisoned_alloc):  # noqa: F811
    """random pixels, a constant image, the extremes 0 and 255; image bytes at offsets 0 and 1 (whole-word and
    single-byte loads)"""
    h, w = shape
    rng = np.random.default_rng(h * w)
    imgs = rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    imgs[1] = (17, 130, 201)
    imgs[2].reshape(-1)[::2] = 0
    imgs[2].reshape(-1)[1::2] = 255
    if h * w >= 63:
        imgs[2, h // 2, w // 2] = 0
        imgs[2, h - 1, w - 1] = 255
    want = np.stack([R.gray(i) for i in imgs])
    for offset in (0, 1):
        for a, b in ((0, 3), (1, 2), (2, 3)):
            got, minmax = raw_gray(dev(imgs[a:b], offset))
            ref = want[a:b]
            assert got.dtype == np.float64 and np.array_equal(got, ref), (shape, offset, a, b)
            assert np.array_equal(minmax[:, 0], ref.reshape(b - a, -1).min(axis=1))
            assert np.array_equal(minmax[:, 1], ref.reshape(b - a, -1).max(axis=1))
    assert want[1].min() == want[1].max()
    if h * w >= 63:
        assert want[2].min() == 0.0 and want[2].max() == R.gray(np.full((1, 1, 3), 255, dtype=np.uint8))[0, 0]
    assert poisoned_alloc.check() > 0


# -------------------------------------------------------------------------------------------------------- histogram
def _edge_plane(lo, hi, hw, seed):
    """hw float64 values in [lo, hi] that hold lo, hi, every edge of linspace(lo, hi, 257) and its two neighbours"""
    edges = np.linspace(lo, hi, 257)
    x = np.concatenate([[lo, hi], edges, np.nextafter(edges, np.inf), np.nextafter(edges, -np.inf)])
    x = x[(x >= lo) & (x <= hi)]
    rng = np.random.default_rng(seed)
    fill = rng.uniform(lo, hi, hw - x.size) if hw > x.size else np.zeros(0)
    fill[: fill.size // 4] = rng.choice(edges, fill.size // 4)  # many more on the edges themselves
    x = np.concatenate([x, fill])[:hw]
    x[:2] = lo, hi
    return rng.permutation(x), edges


@pytest.mark.parametrize('hw', [2, 1000, 264 * 265 + 1])
def test_histogram_counts_are_numpys(hw, poisoned_alloc):  # noqa: F811
    """three planes with ranges of their own; the odd plane size puts the middle plane off the 16-byte grid (single
    loads); the largest gives every block more pixels than one fold of the 32-bit bins holds"""
    _, L, _, _ = _mods()
    planes, edges = zip(*[_edge_plane(lo, hi, hw, k) for k, (lo, hi) in enumerate(((0.0, 1.0), (0.05, 0.93), (1e-3, 1e-3 + 1e-9)))])
    want = np.stack([np.histogram(p, 256)[0] for p in planes])
    for p, e in zip(planes, edges):
        assert np.array_equal(np.histogram(p, 256)[1], e)  # numpy's edges are the uploaded ones
    got = raw_hist(dev(np.stack(planes)), dev(np.stack(edges)))
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(raw_hist(dev(planes[1][None]), dev(edges[1][None])), want[1:2])
    if hw > 1000:
        blocks = L.cae_mask_hist_workspace(3, hw) // (3 * 256 * 8)
        assert hw / blocks > 2 * L.cae_mask_hist_fold()  # (16384 pixels a fold: 34981 a block here, three folds)
    assert poisoned_alloc.check() > 0


# ----------------------------------------------------------------------------------------------------------- labels
@pytest.mark.parametrize('shape', SHAPES)
def test_labels_for_eight_and_four_neighbours(shape, poisoned_alloc):  # noqa: F811
    """8: what segmenters.components gives; 4: scipy's default structure, made canonical; the complement's objects for
    both (of_zero)"""
    _, _, S, _ = _mods()
    h, w = shape
    for i in range(0, len(PATTERNS), 3):
        names = PATTERNS[i:i + 3]
        planes = np.stack([TO.plane(k, h, w) for k in names])
        target = dev(planes, offset=(i // 3) % 2)
        eight = raw_label(target, 8).cpu().numpy()
        assert np.array_equal(eight, S.components(target)[0].cpu().numpy()), (names, shape)
        four = raw_label(target, 4).cpu().numpy()
        four_c = raw_label(target, 4, of_zero=1).cpu().numpy()
        eight_c = raw_label(target, 8, of_zero=1).cpu().numpy()
        for k, name in enumerate(names):
            assert np.array_equal(eight[k], R.canonical_labels(planes[k] != 0, 8)), (name, shape)
            assert np.array_equal(four[k], R.canonical_labels(planes[k] != 0, 4)), (name, shape)
            assert np.array_equal(four_c[k], R.canonical_labels(planes[k] == 0, 4)), (name, shape)
            assert np.array_equal(eight_c[k], R.canonical_labels(planes[k] == 0, 8)), (name, shape)
    if min(h, w) >= 7:  # lines that hold together by corners only fall apart
        assert len(np.unique(R.canonical_labels(TO.plane('antidiagonal', h, w) != 0, 4))) > \
            len(np.unique(R.canonical_labels(TO.plane('antidiagonal', h, w) != 0, 8)))
    assert poisoned_alloc.check() > 0


# ------------------------------------------------------------------------------------------------------ area filter
def _filter_plane():
    """300 x 300: one object of 262 x 262 = 68644 pixels (more than 2^16) with two holes of 12 and 11 pixels and a notch
    of 6 pixels on the plane's upper border, an object of 10 and one of 9 pixels"""
    a = np.zeros((300, 300), dtype=np.uint8)
    a[0:262, 0:262] = 1
    a[50:53, 60:64] = 0       # a hole of exactly 12
    a[100:103, 60:64] = 0     # 11: one corner stays tissue
    a[100, 60] = 1
    a[0:2, 100:103] = 0       # 6 pixels of complement on the border
    a[270:272, 10:15] = 1     # exactly 10
    a[270:273, 30:33] = 1     # 9
    return a


def test_area_filter_at_its_limits(poisoned_alloc):  # noqa: F811
    h = w = 300
    planes = np.stack([_filter_plane(), (TO.plane('b40', h, w) != 0).astype(np.uint8)])
    assert planes[0, :262, :262].sum() > 2 ** 16
    target = dev(planes)
    objects, _ = raw_area_filter(raw_label(target, 8), target, 10, 0)
    for k in range(2):
        assert np.array_equal(objects[k] != 0, (planes[k] != 0) & ~R.small_components(planes[k] != 0, 8, 10)), k
    assert objects[0, 270:272, 10:15].all() and not objects[0, 270:273, 30:33].any()  # 10 stays, 9 goes
    assert np.array_equal(objects[0, :262], planes[0, :262]) and not np.array_equal(objects[1], planes[1])
    after = dev(objects)
    holes, wide = raw_area_filter(raw_label(after, 4, of_zero=1), after, 12, 1, wide=True)
    for k in range(2):
        assert np.array_equal(holes[k] != 0, (objects[k] != 0) | R.small_components(objects[k] == 0, 4, 12)), k
    assert not holes[0, 50:53, 60:64].any() and holes[0, 100:103, 60:64].all()  # 12 stays, 11 is filled
    assert holes[0, 0:2, 100:103].all()                                         # the border gives no exemption
    assert wide.dtype == np.int32 and np.array_equal(wide, (holes != 0).astype(np.int32))
    assert set(np.unique(holes)) <= {0, 1}
    # limits that clear nothing and everything
    same, _ = raw_area_filter(raw_label(target, 8), target, 0, 0)
    none, _ = raw_area_filter(raw_label(target, 8), target, 2 ** 31 - 1, 0)
    assert np.array_equal(same, planes) and not none.any()
    assert poisoned_alloc.check() > 0


@pytest.mark.parametrize('shape', SHAPES)
def test_area_filter_on_the_patterns(shape, poisoned_alloc):  # noqa: F811
    h, w = shape
    names = ('b10', 'b40', 'rings')
    planes = np.stack([(TO.plane(k, h, w) != 0).astype(np.uint8) for k in names])
    target = dev(planes, offset=1)
    for conn, of_zero, least, value in ((8, 0, 3, 0), (4, 0, 2, 0), (4, 1, 3, 1), (8, 1, 5, 1)):
        got, wide = raw_area_filter(raw_label(target, conn, of_zero), target, least, value, wide=True)
        for k in range(3):
            fg = planes[k] != 0
            small = R.small_components(fg != bool(of_zero), conn, least)
            assert np.array_equal(got[k] != 0, (fg & ~small) if value == 0 else (fg | small)), (names[k], shape, conn, of_zero)
        assert np.array_equal(wide, (got != 0).astype(np.int32))
    assert poisoned_alloc.check() > 0


# --------------------------------------------------------------------------------------------------------- dilation
@pytest.mark.parametrize('shape', SHAPES)
def test_dilation_by_a_disk(shape, poisoned_alloc):  # noqa: F811
    h, w = shape
    corner = np.zeros((h, w), dtype=np.uint8)
    corner[h - 1, 0] = 1
    planes = np.stack([np.zeros((h, w), dtype=np.uint8), np.ones((h, w), dtype=np.uint8), corner,
                       (TO.plane('b10', h, w) != 0).astype(np.uint8) if h * w > 100 else corner[::-1, ::-1]])
    for radius in (0, 1, 3, 16):
        got = raw_dilate(dev(planes), radius)
        assert set(np.unique(got)) <= {0, 1}
        for k in range(len(planes)):
            assert np.array_equal(got[k] != 0, R.dilate(planes[k] != 0, radius)), (shape, radius, k)
        assert not got[0].any() and got[1].all()
    assert poisoned_alloc.check() > 0


# -------------------------------------------------------------------------------------------------------- downscale
@pytest.mark.parametrize('shape', SHAPES + [(70, 128)])
def test_downscale(shape, poisoned_alloc):  # noqa: F811
    """factors that do not divide the sizes; (70, 128) has rows that are runs of 16-byte groups (the wide loads) and a
    ragged last block row; windows of a larger image are read where they stand"""
    _, _, _, T = _mods()
    h, w = shape
    rng = np.random.default_rng(h + w)
    for c in (3, 1, 4):
        imgs = rng.integers(0, 256, (2, h, w, c), dtype=np.uint8)
        imgs[1, : h // 2] = 255  # no sum may wrap
        on_dev = dev(imgs)
        for f in (1, 2, 3, 16, 32):
            got = T.downscale(on_dev, f)
            torch.cuda.synchronize()
            assert got.dtype == torch.uint8 and got.shape == (2, -(-h // f), -(-w // f), c)
            for k in range(2):
                assert np.array_equal(got[k].cpu().numpy(), R.downscale(imgs[k], f)), (shape, c, f, k)
        if c == 3 and h > 8:
            win = on_dev[:, : h - 3, : w - 5]
            assert not win.is_contiguous()
            got = T.downscale(win, 2).cpu().numpy()
            assert np.array_equal(got[1], R.downscale(imgs[1, : h - 3, : w - 5], 2))
            assert np.array_equal(T.downscale(imgs[0], 3).cpu().numpy(), R.downscale(imgs[0], 3))  # host (H,W,C) input
    assert poisoned_alloc.check() > 0


# ------------------------------------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def tile(h, w, idx):
    from cnn_autoencoder_amd import synth
    img = synth.histo_tile(h, idx, w)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def truth(h, w, idx, params):
    return R.tissue_mask(tile(h, w, idx), *params)


def judge_mask(T, imgs, wants, params, batched=True):
    mask, tap = T.tissue_mask(dev(imgs) if batched else torch.from_numpy(imgs[0].copy()), *params, taps=True)
    torch.cuda.synchronize()
    assert mask.dtype == torch.bool and mask.is_cuda
    mask = mask.cpu().numpy() if batched else mask.cpu().numpy()[None]
    for k, want in enumerate(wants):
        assert np.array_equal(tap['gray'][k].cpu().numpy(), want['gray']), k
        assert np.array_equal(tap['counts'][k], want['counts']), k
        assert tap['thr'][k] == want['thr'], (k, tap['thr'][k], want['thr'])
        for name in ('thresholded', 'objects', 'holes'):
            assert np.array_equal(tap[name][k].cpu().numpy() != 0, want[name]), (k, name)
        assert np.array_equal(mask[k], want['mask']), k
    assert np.array_equal(mask, T.tissue_mask(dev(imgs), *params).cpu().numpy())  # without taps: the same mask


@pytest.mark.parametrize('case', [((96, 80), (2, 5, 11), (16, 64, 3)), ((264, 265), (3, 9), (16, 64, 3)),
                                  ((400, 420), (8,), (256, 16384, 16))])
def test_tissue_mask_of_procedural_tiles(case, poisoned_alloc):  # noqa: F811
    _, _, _, T = _mods()
    (h, w), idxs, params = case
    wants = [truth(h, w, i, params) for i in idxs]
    for want in wants:  # the case is not trivial
        assert 0.05 <= want['mask'].mean() <= 0.95
        assert (want['thresholded'] != want['objects']).any()
        if params[1] < 16384:
            assert (want['holes'] != want['objects']).any()
    imgs = np.stack([tile(h, w, i) for i in idxs])
    judge_mask(T, imgs, wants, params, batched=len(idxs) > 1)
    if len(idxs) > 1:  # a plane alone gives what it gives in a batch
        judge_mask(T, imgs[1:2], wants[1:2], params)
    assert poisoned_alloc.check() > 0


def test_constant_and_tiny_planes(poisoned_alloc):  # noqa: F811
    """a constant plane has no histogram: its threshold is its value and all of it is tissue; beside a varied plane"""
    _, _, _, T = _mods()
    rng = np.random.default_rng(5)
    for h, w in ((1, 1), (7, 9)):
        imgs = rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)
        imgs[1] = (200, 100, 50)
        params = (2, 3, 1)
        wants = [R.tissue_mask(i, *params) for i in imgs]
        assert wants[1]['mask'].all() and not wants[1]['counts'].any()
        judge_mask(T, imgs, wants, params)
    empty = T.tissue_mask(torch.zeros((0, 4, 4, 3), dtype=torch.uint8))
    assert empty.shape == (0, 4, 4) and empty.dtype == torch.bool
    assert poisoned_alloc.check() > 0


# -------------------------------------------------------------------------------------------------------- mask_zarr
def test_mask_zarr_of_a_plain_store(tmp_path, poisoned_alloc):  # noqa: F811
    """64 x 64 chunks, a ragged edge, factor 4: masks/0/0 is the restatement's mask of the numpy-downscaled image"""
    _, _, _, T = _mods()
    from cnn_autoencoder_amd.sampler import PatchSampler
    from cnn_autoencoder_amd.zarrio import ZarrArray, Zlib
    img = tile(150, 201, 4)
    store = str(tmp_path / 'slide.zarr')
    ZarrArray.create(store, '0/0', img.shape, (64, 64, 3), np.uint8, codec=Zlib(1))[:] = img
    params = dict(min_size=4, area_threshold=16, radius=2)
    got = T.mask_zarr(store, factor=4, batch_tiles=5, **params)
    want = R.tissue_mask(R.downscale(img, 4), **params)['mask']
    assert 0.05 <= want.mean() <= 0.95
    assert got.dtype == np.bool_ and np.array_equal(got, want)
    z = ZarrArray.open(store, 'masks/0/0')
    assert z.meta['dtype'] == '|b1' and z.meta['compressor'] == {'id': 'zlib', 'level': 9}
    assert z.shape == (38, 51) and z.attrs['scale'] == 0.25 and np.array_equal(z[:], want)
    # to another store; and the samplers take it
    other = str(tmp_path / 'masks.zarr')
    assert np.array_equal(T.mask_zarr(store, other, factor=4, **params), want)
    assert np.array_equal(ZarrArray.open(other, 'masks/0/0')[:], want)
    keep = T.mask_tiles(want, 0.25, img.shape, (64, 64))
    assert PatchSampler.from_zarr([store], patch_size=16, mask_group='masks/0/0').T == int(keep.sum())
    assert poisoned_alloc.check() > 0


def test_mask_zarr_of_a_compressed_store(tmp_path):
    """a 'cae' array: the chunks are decoded in batches and reduced on the device; the mask is that of the decoded image"""
    _, _, _, T = _mods()
    from cnn_autoencoder_amd import synth, zarrio
    img = tile(150, 201, 4)
    path = os.path.join(str(tmp_path), 'ckpt.pth')
    torch.save(synth.synthetic_state(dict(synth.CANONICAL), seed=0), path)
    store = str(tmp_path / 'slide.zarr')
    zarrio.compress_image('CAE', path, img, store, patch_size=64, batch_tiles=4)
    params = dict(min_size=4, area_threshold=16, radius=2)
    got = T.mask_zarr(store, factor=4, batch_tiles=5, **params)
    want = R.tissue_mask(R.downscale(zarrio.decompress_image(store), 4), **params)['mask']
    assert np.array_equal(got, want)
    assert zarrio.ZarrArray.open(store, 'masks/0/0').attrs == {'scale': 0.25}
