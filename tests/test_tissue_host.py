"""Host side of the tissue mask (cnn_autoencoder_amd/tissue.py, csrc/cae_mask.hip): the restatement the GPU tests judge
the kernels by (tests/tissue_restatement.py) is checked against hand-made cases, the product's host steps
(otsu_threshold, mask_tiles, the samplers' mask_group) against it, then the refusals of the new entry points, which all
return before any launch.  No test here needs a GPU.
"""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import tissue_restatement as R

MASK_SYMBOLS = ('cae_mask_gray', 'cae_mask_hist', 'cae_mask_hist_workspace', 'cae_mask_hist_fold', 'cae_mask_threshold',
                'cae_mask_label', 'cae_mask_label_workspace', 'cae_mask_area_filter', 'cae_mask_area_workspace',
                'cae_mask_within', 'cae_mask_downscale')


# ------------------------------------------------------------------------------------------------ the restatement
def test_a_bimodal_histogram_has_the_threshold_between_its_modes():
    """two bins hold everything: every split between them has the same variance, and the first of them is taken"""
    counts = np.zeros(256, dtype=np.int64)
    counts[40], counts[200] = 700, 300
    edges = np.linspace(0.0, 1.0, 257)
    centres = (edges[:-1] + edges[1:]) / 2
    assert R.otsu_by_definition(counts, edges) == centres[40]
    # three bins: 10 at bin 0, 10 at bin 1, 20 at bin 9 of 10 -> the split behind bin 1 (variance 10 * 30 * ... is
    # smaller than 20 * 20 * ...)
    counts = np.array([10, 10, 0, 0, 0, 0, 0, 0, 0, 20])
    edges = np.arange(11.0)
    assert R.otsu_by_definition(counts, edges) == 1.5
    from cnn_autoencoder_amd.tissue import otsu_threshold
    assert otsu_threshold(counts, edges) == 1.5


def test_the_products_threshold_is_the_definitions():
    """cumulative sums from both ends (the product, as skimage writes it) against explicit, exactly rounded class sums
    per split: random counts, counts with runs of empty bins (where whole ranges of splits tie), and the test tiles"""
    from cnn_autoencoder_amd import synth
    from cnn_autoencoder_amd.tissue import otsu_threshold
    rng = np.random.default_rng(0)
    for k in range(120):
        counts = rng.integers(0, 1000, 256)
        counts[rng.random(256) < rng.choice([0.0, 0.3, 0.9])] = 0
        counts[0], counts[-1] = max(counts[0], 1), max(counts[-1], 1)  # min and max of the plane lie in the end bins
        edges = np.linspace(rng.random(), 1 + rng.random(), 257)
        assert otsu_threshold(counts, edges) == R.otsu_by_definition(counts, edges), k
    for idx in (2, 5, 11):
        counts, edges = R.histogram(R.gray(synth.histo_tile(96, idx, 80)))
        assert otsu_threshold(counts, edges) == R.otsu_by_definition(counts, edges), idx
    for bad in ((np.ones(256), np.ones(256)), (np.ones((2, 2)), np.ones(3)), (-np.ones(4), np.arange(5.0))):
        with pytest.raises(ValueError, match='counts'):
            otsu_threshold(*bad)


def test_the_bin_rule_of_the_contract_is_numpys_histogram():
    """the rule cae_mask_hist states -- the scaled estimate, 256 -> 255, one step down or up against the edges -- in
    numpy, on values that sit on, just below and just above every edge, and on random ones"""
    rng = np.random.default_rng(1)
    for lo, hi in ((0.0, 1.0), (0.1, 0.7), (0.2125 * 3 / 255, 0.93), (1e-3, 1e-3 + 1e-9)):
        edges = np.linspace(lo, hi, 257)
        x = np.concatenate([edges, np.nextafter(edges, np.inf), np.nextafter(edges, -np.inf), rng.uniform(lo, hi, 100000)])
        x = x[(x >= lo) & (x <= hi)]
        idx = ((x - lo) * (256 / (hi - lo))).astype(np.int64)
        idx[idx == 256] = 255
        idx[x < edges[idx]] -= 1
        up = (x >= edges[idx + 1]) & (idx != 255)
        idx[up] += 1
        assert np.array_equal(np.bincount(idx, minlength=256), np.histogram(x, 256, range=(lo, hi))[0]), (lo, hi)


def test_hand_made_filters_and_dilation():
    plane = np.zeros((6, 7), dtype=bool)
    plane[0, 0] = plane[1, 1] = True          # two pixels joined by a corner: one object of 2 with 8, two of 1 with 4
    plane[3:6, 3:6] = True
    plane[4, 4] = False                       # a hole of one pixel
    assert R.small_components(plane, 8, 2).sum() == 0 and R.small_components(plane, 8, 3).sum() == 2
    assert R.small_components(plane, 4, 2).sum() == 2
    assert R.small_components(~plane, 4, 2).sum() == 1 and R.small_components(~plane, 4, 1).sum() == 0
    lab = R.canonical_labels(plane, 8)
    assert lab[0, 0] == 1 and lab[1, 1] == 1 and lab[5, 5] == 3 * 7 + 3 + 1 and lab[4, 4] == 0
    assert R.canonical_labels(plane, 4)[1, 1] == 1 * 7 + 1 + 1
    assert R.disk(0).tolist() == [[True]] and R.disk(1).sum() == 5 and R.disk(3).sum() == 29
    one = np.zeros((5, 5), dtype=bool)
    one[0, 0] = True
    assert R.dilate(one, 3).sum() == 11 and not R.dilate(np.zeros((5, 5), dtype=bool), 3).any()
    img = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    small = R.downscale(img, 2)
    assert small.shape == (3, 4, 3)
    assert small[0, 0, 0] == (2 * (0 + 3 + 21 + 24) + 4) // 8 and small[2, 3, 1] == img[4, 6, 1]
    assert np.array_equal(R.downscale(img, 1), img)


# ------------------------------------------------------------------------------------------------------ mask_tiles
def test_mask_tiles_on_ragged_shapes():
    from cnn_autoencoder_amd.tissue import mask_tiles
    # an array of 100 x 150 in chunks of 64: a 2 x 3 grid with a ragged edge; its mask at 1 / 4 is 25 x 38
    mask = np.zeros((25, 38), dtype=bool)
    assert not mask_tiles(mask, 0.25, (100, 150), (64, 64)).any()
    mask[15, 15] = True   # pixel rows 60..63: chunk row 0; columns 60..63: chunk column 0
    assert mask_tiles(mask, 0.25, (100, 150), (64, 64)).tolist() == [[True, False, False], [False, False, False]]
    mask[:] = False
    mask[16, 16] = True   # the first mask pixel of chunk (1, 1)
    assert mask_tiles(mask, 0.25, (100, 150), (64, 64)).tolist() == [[False, False, False], [False, True, False]]
    mask[:] = False
    mask[24, 37] = True   # the last one: the ragged corner chunk, whose footprint rows 16:25 and columns 32:38 it lies in
    assert mask_tiles(mask, 0.25, (100, 150), (64, 64)).tolist() == [[False, False, False], [False, False, True]]
    # a scale whose footprints share a mask pixel: 1 / 48 of chunks of 32 -> mask pixel 0 covers chunks 0 and 1
    mask = np.zeros((2, 2), dtype=bool)
    mask[0, 1] = True
    keep = mask_tiles(mask, 1 / 48, (96, 96), (32, 32))
    assert keep.tolist() == [[False, True, True], [False, True, True], [False, False, False]]
    assert mask_tiles(torch.ones((1, 1), dtype=torch.bool), 1 / 64, (10, 64, 3), (8, 8, 3)).all()
    # a mask smaller than the array's footprint: what lies beyond it is not tissue
    assert mask_tiles(np.ones((1, 1), dtype=bool), 0.25, (16, 16), (4, 4)).tolist() == [[True] + [False] * 3] + [[False] * 4] * 3
    for bad in (dict(scale=0.0), dict(scale=math.nan), dict(scale=-1.0)):
        with pytest.raises(ValueError, match='scale'):
            mask_tiles(mask, bad['scale'], (96, 96), (32, 32))
    with pytest.raises(ValueError, match='mask'):
        mask_tiles(np.zeros((2, 2, 2)), 1.0, (4, 4), (2, 2))


# ---------------------------------------------------------------------------------------------- samplers' mask_group
def _store(tmp_path, mask, scale=0.25, attrs=True):
    """an image and labels of 100 x 150 in 2 x 3 chunks of 64, and a mask"""
    from cnn_autoencoder_amd.zarrio import ZarrArray, Zlib
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (100, 150, 3), dtype=np.uint8)
    lab = rng.integers(0, 2, (100, 150), dtype=np.uint8)
    store = str(tmp_path / 'slide.zarr')
    ZarrArray.create(store, '0/0', img.shape, (64, 64, 3), np.uint8, codec=Zlib(1))[:] = img
    ZarrArray.create(store, 'labels/0/0', lab.shape, (64, 64), np.uint8, codec=Zlib(1))[:] = lab
    m = ZarrArray.create(store, 'masks/0/0', mask.shape, mask.shape, np.bool_, codec=Zlib(9))
    m[:] = mask
    if attrs:
        m.write_attrs({'scale': scale})
    return store, img, lab


def test_the_samplers_draw_inside_the_mask(tmp_path):
    from cnn_autoencoder_amd.sampler import LabeledPatchSampler, PatchSampler
    from cnn_autoencoder_amd.zarrio import ZarrArray
    mask = np.zeros((25, 38), dtype=bool)
    mask[3, 20] = True    # chunk (0, 1)
    mask[20, 36] = True   # chunk (1, 2), the ragged corner: 36 x 22 real pixels
    store, img, lab = _store(tmp_path, mask)
    z = ZarrArray.open(store, 'masks/0/0')
    assert z.meta['dtype'] == '|b1' and z.attrs == {'scale': 0.25} and np.array_equal(z[:], mask)
    everything = PatchSampler.from_zarr([store], patch_size=16)
    assert everything.T == 6
    s = PatchSampler.from_zarr([store], patch_size=16, mask_group='masks/0/0')
    assert s.T == 2 and s.tile_hw.tolist() == [[64, 64], [36, 22]]
    assert np.array_equal(s.pool[0].numpy(), img[0:64, 64:128])
    assert np.array_equal(s.pool[1, :36, :22].numpy(), img[64:100, 128:150])
    assert torch.equal(everything.pool[[1, 5]], s.pool)
    ls = LabeledPatchSampler.from_zarr([store], patch_size=16, mask_group='masks/0/0')
    assert ls.T == 2 and torch.equal(ls.pool, s.pool) and ls.tile_hw.tolist() == [[64, 64], [36, 22]]
    assert np.array_equal(ls.labels[0, :, :, 0].numpy(), lab[0:64, 64:128])
    assert np.array_equal(ls.labels[1, :36, :22, 0].numpy(), lab[64:100, 128:150])
    # None changes nothing
    for cls in (PatchSampler, LabeledPatchSampler):
        a, b = cls.from_zarr([store], patch_size=16), cls.from_zarr([store], patch_size=16, mask_group=None)
        assert torch.equal(a.pool, b.pool) and torch.equal(a.tile_hw, b.tile_hw) and a.T == 6
    # two stores: each store's own mask selects its chunks
    both = PatchSampler.from_zarr([store, store], patch_size=16, mask_group='masks/0/0')
    assert both.T == 4 and torch.equal(both.pool[:2], both.pool[2:])


def test_an_empty_mask_and_a_mask_without_scale_are_refused(tmp_path):
    from cnn_autoencoder_amd.sampler import LabeledPatchSampler, PatchSampler
    (tmp_path / 'a').mkdir()
    (tmp_path / 'b').mkdir()
    empty, _, _ = _store(tmp_path / 'a', np.zeros((25, 38), dtype=bool))
    bare, _, _ = _store(tmp_path / 'b', np.ones((25, 38), dtype=bool), attrs=False)
    for cls in (PatchSampler, LabeledPatchSampler):
        with pytest.raises(ValueError, match='no tile'):
            cls.from_zarr([empty], patch_size=16, mask_group='masks/0/0')
        with pytest.raises(ValueError, match='scale'):
            cls.from_zarr([bare], patch_size=16, mask_group='masks/0/0')
        assert cls.from_zarr([empty], patch_size=16).T == 6


# ---------------------------------------------------------------------------------------------------------- the ABI
def test_the_new_symbols_are_declared_and_bound(built_lib):
    from cnn_autoencoder_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, 'include', 'cae_hip.h')).read()
    declared = set(re.findall(r'\b(cae_[a-z0-9_]+)\s*\(', hdr))
    L = _lib.lib()
    for name in MASK_SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS, name
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is not None, name
    assert {k for k in _lib.SYMBOLS if k.startswith('cae_mask_')} == set(MASK_SYMBOLS)


def test_workspace_queries(built_lib):
    from cnn_autoencoder_amd import _lib
    L = _lib.lib()
    assert L.cae_mask_hist_fold() >= 1024 and L.cae_mask_hist_fold() < 2 ** 32
    for n, hw in ((0, 16), (-1, 16), (1, 0), (1, 2 ** 31)):
        assert L.cae_mask_hist_workspace(n, hw) == 0, (n, hw)
    for n, hw in ((1, 1), (3, 63), (3, 264 * 265), (1, 3072 * 3072), (1, 2 ** 31 - 1)):
        need = L.cae_mask_hist_workspace(n, hw)
        assert need >= n * 256 * 8 and need % (256 * 8) == 0, (n, hw)
    for n, h, w in ((0, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, 0), (1, 32769, 4), (1, 4, 32769), (1, 21846, 21846), (1, 1 << 30, 4)):
        assert L.cae_mask_label_workspace(n, h, w) == 0 and L.cae_mask_area_workspace(n, h, w) == 0, (n, h, w)
    for n, h, w in ((1, 1, 1), (3, 7, 9), (3, 264, 265), (1, 3072, 3072), (1, 32768, 3)):
        assert L.cae_mask_label_workspace(n, h, w) == L.cae_seg_components_workspace(n, h, w) > 0
        assert L.cae_mask_area_workspace(n, h, w) == 4 * n * h * w


def test_abi_refuses_without_a_device(built_lib):
    """bad arguments are refused before anything touches a device; n == 0 is nothing to do"""
    from cnn_autoencoder_amd import _lib
    L = _lib.lib()
    p = 1 << 20  # a pointer-like value that is aligned to everything; never dereferenced: every call here is refused
    big = 1 << 40
    gray = lambda img=p, n=1, hw=16, g=p, mm=p: L.cae_mask_gray(img, n, hw, g, mm, None)  # noqa: E731
    assert gray(n=0) == 0 and gray(n=0, img=None, g=None, mm=None) == 0
    for kw in (dict(n=-1), dict(hw=0), dict(hw=2 ** 31), dict(img=None), dict(g=None), dict(mm=None), dict(g=p + 4), dict(mm=p + 1)):
        assert gray(**kw) == -1, kw
    assert gray(n=0, hw=0) == -1  # a bad shape is a bad shape with no planes too

    hist = lambda g=p, e=p, n=1, hw=16, c=p, ws=p, nbytes=big: L.cae_mask_hist(g, e, n, hw, c, ws, nbytes, None)  # noqa: E731
    assert hist(n=0) == 0 and hist(n=0, g=None, e=None, c=None, ws=None, nbytes=0) == 0
    need = L.cae_mask_hist_workspace(1, 16)
    for kw in (dict(n=-1), dict(hw=0), dict(hw=2 ** 31), dict(g=None), dict(e=None), dict(c=None), dict(ws=None), dict(nbytes=0),
               dict(nbytes=need - 1), dict(g=p + 4), dict(e=p + 2), dict(c=p + 4), dict(ws=p + 4)):
        assert hist(**kw) == -1, kw

    thr = lambda g=p, t=p, n=1, hw=16, out=p: L.cae_mask_threshold(g, t, n, hw, out, None)  # noqa: E731
    assert thr(n=0) == 0 and thr(n=0, g=None, t=None, out=None) == 0
    for kw in (dict(n=-1), dict(hw=0), dict(hw=2 ** 31), dict(g=None), dict(t=None), dict(out=None), dict(g=p + 4), dict(t=p + 4)):
        assert thr(**kw) == -1, kw

    label = lambda plane=p, n=1, h=4, w=4, conn=8, of_zero=0, labels=p, ws=p, nbytes=big: L.cae_mask_label(  # noqa: E731
        plane, n, h, w, conn, of_zero, labels, ws, nbytes, None)
    assert label(n=0) == 0 and label(n=0, plane=None, labels=None, ws=None, nbytes=0) == 0
    need = L.cae_mask_label_workspace(1, 4, 4)
    for kw in (dict(n=-1), dict(h=0), dict(w=0), dict(h=32769), dict(w=32769), dict(h=21846, w=21846), dict(h=1 << 30), dict(conn=6),
               dict(conn=0), dict(plane=None), dict(labels=None), dict(ws=None), dict(nbytes=0), dict(nbytes=need - 1),
               dict(labels=p + 2), dict(ws=p + 4)):
        assert label(**kw) == -1, kw
    assert label(n=0, conn=5) == -1

    area = lambda labels=p, n=1, h=4, w=4, least=2, value=0, plane=p, wide=None, ws=p, nbytes=big: L.cae_mask_area_filter(  # noqa: E731
        labels, n, h, w, least, value, plane, wide, ws, nbytes, None)
    assert area(n=0) == 0 and area(n=0, labels=None, plane=None, ws=None, nbytes=0) == 0
    need = L.cae_mask_area_workspace(1, 4, 4)
    for kw in (dict(n=-1), dict(h=0), dict(w=0), dict(h=32769), dict(h=21846, w=21846), dict(least=-1), dict(value=2), dict(value=-1),
               dict(labels=None), dict(plane=None), dict(ws=None), dict(nbytes=0), dict(nbytes=need - 1), dict(labels=p + 2),
               dict(wide=p + 1), dict(ws=p + 2)):
        assert area(**kw) == -1, kw

    within = lambda d2=p, n=1, hw=16, r2=9, out=p: L.cae_mask_within(d2, n, hw, r2, out, None)  # noqa: E731
    assert within(n=0) == 0 and within(n=0, d2=None, out=None) == 0
    for kw in (dict(n=-1), dict(hw=0), dict(hw=2 ** 31), dict(r2=-1), dict(d2=None), dict(out=None), dict(d2=p + 2)):
        assert within(**kw) == -1, kw

    down = lambda img=p, n=1, h=8, w=8, c=3, rp=24, pp=192, f=2, out=p: L.cae_mask_downscale(  # noqa: E731
        img, n, h, w, c, rp, pp, f, out, None)
    assert down(n=0) == 0 and down(n=0, img=None, out=None) == 0
    for kw in (dict(n=-1), dict(h=0), dict(w=0), dict(h=1 << 16, w=1 << 16, rp=3 << 16), dict(c=0), dict(c=5), dict(f=0), dict(f=65),
               dict(rp=23), dict(n=2, pp=191), dict(img=None), dict(out=None)):
        assert down(**kw) == -1, kw


def test_the_new_kernels_use_no_scratch(built_lib):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import scratch_check
    mine = re.compile(r'cae12_GLOBAL__N_1\d+mask_[a-z0-9_]+_kernel')  # (namespace cae: not the sampler's mask_rows_kernel)
    table = {k: v for k, v in scratch_check.kernel_table(built_lib).items() if mine.search(k)}
    assert len(table) == 8 + 4 + 1, sorted(table)  # the downscale for 1..4 channels; the merge step for 4 neighbours
    assert not any('mask_hist_sum_kernel' in k for k in table)  # (the histogram's partials: seg_histsum_kernel, tests/test_seg_roc_host.py)
    assert all(v == (0, 0) for v in table.values()), table


# -------------------------------------------------------------------------------------------------- Python surface
def test_the_python_surface_refuses_bad_arguments(monkeypatch):
    from cnn_autoencoder_amd import tissue
    img = torch.zeros((2, 8, 9, 3), dtype=torch.uint8)
    for bad in (img.float(), img[0, 0], img.numpy().astype(np.int32), torch.zeros((2, 8, 9, 5), dtype=torch.uint8)):
        with pytest.raises(ValueError, match='uint8|channels'):
            tissue.downscale(bad, 2)
    for f in (0, 65, 1.5, True):
        with pytest.raises(ValueError, match='factor'):
            tissue.downscale(img, f)
    with pytest.raises(ValueError, match='3 channels'):
        tissue.tissue_mask(torch.zeros((8, 9, 4), dtype=torch.uint8))
    with pytest.raises(ValueError, match='empty'):
        tissue.tissue_mask(torch.zeros((1, 0, 9, 3), dtype=torch.uint8))
    for kw in (dict(min_size=-1), dict(area_threshold=1.5), dict(radius=-2), dict(radius=46341)):
        with pytest.raises(ValueError, match='|'.join(kw)):
            tissue.tissue_mask(img, **kw)
    for shape in ((1, 32769, 2, 3), (1, 2, 32769, 3), (1, 21846, 21846, 3)):
        with pytest.raises(ValueError, match='too large'):
            tissue.tissue_mask(torch.zeros(shape, dtype=torch.uint8, device='meta'))
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)  # (so on a machine that has one, too)
    with pytest.raises(RuntimeError, match='no HIP device'):
        tissue.tissue_mask(img)
    with pytest.raises(RuntimeError, match='no HIP device'):
        tissue.downscale(img, 2)


def test_mask_zarr_refuses_before_the_device(tmp_path, monkeypatch):
    from cnn_autoencoder_amd import tissue
    from cnn_autoencoder_amd.zarrio import ZarrArray
    store = str(tmp_path / 's.zarr')
    ZarrArray.create(store, '0/0', (100, 150, 3), (64, 64, 3), np.uint8)
    ZarrArray.create(store, 'labels/0/0', (100, 150), (64, 64), np.uint8)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(ValueError, match='does not divide'):
        tissue.mask_zarr(store, factor=3)
    with pytest.raises(ValueError, match='factor'):
        tissue.mask_zarr(store, factor=128)
    with pytest.raises(ValueError, match='uint8 array'):
        tissue.mask_zarr(store, data_group='labels/0/0', factor=4)
    with pytest.raises(RuntimeError, match='no HIP device'):
        tissue.mask_zarr(store, factor=4)
