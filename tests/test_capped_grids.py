"""The plane kernels where the block cap makes lanes take many turns (csrc/cae_seg_metrics.hpp: blocks_for).

The segmentation-metric, weight-map and tissue-mask launchers give a plane one block per 256 lanes' worth of items until
the whole launch has kBlocksTarget = 4096 blocks; from there the blocks per plane stop growing and a lane walks its plane
with `for (i = first; i < items; i += stride)`.  The other test files stay far below that point, so every lane there runs
its loop body once.  Here every launch is capped:

  regime A   4100 planes: more planes than the cap, so blocks_for clamps 4096 / n = 0 up to one block per plane
  regime B   600 planes: 4096 / 600 = 6 blocks per plane where 18 would be launched, a stride of 1536 lanes; the
             partials of the 6 blocks are merged per plane
  regime C   1100 planes: 3 blocks per plane for cae_seg_predict, whose grid is sized in blocks of 1024 pixels (5 for
             these planes, so that 600 planes do not cap it; its c = 17 case at 600 planes runs uncapped on 5 blocks and
             still takes 4 turns, because the streamed path walks single pixels)
  histograms 1025 planes at 8 bits and 257 at 14 (caps of 1024 and 256): one block takes the span of two

on planes of 65 x 67 = 4355 pixels (odd, hw % 4 == 3, above 4096) and of 64 x 68 = 4352 where cae_seg_predict needs
hw % 4 == 0 for its 16-byte path.  test_the_cases_reach_the_capped_regime (no GPU) reads the blocks per plane from the
library and proves the turns for every row of GRIDS and HISTS; the GPU tests take their shapes from the same tables.

Every comparison follows the rule of the kernel's own test file: integers and the float64 gray values are equal to the
numpy / scipy restatement; the scores of cae_seg_predict lie within 4 E + 2^-24 (tests/test_seg_predict.py) and the weight
map within the bound of tests/test_seg_weight_map.py.  Planes with a cheap reference get content of their own; where the
reference is a scipy call per plane or per object, plane k is distinct[k % 11], the reference computed once per distinct
plane.  Outputs and workspaces come poisoned and fenced (residue.poisoned_alloc).
"""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import seg_objects_oracle as OO
import seg_roc_oracle as RO
import seg_weight_map_oracle as WO
import test_seg_objects as TO
import test_seg_predict as TP
import test_tissue as TT
import tissue_restatement as R
from residue import poisoned_alloc  # noqa: F401  (the fixture)

gpu = pytest.mark.gpu

N_A, N_B, N_C = 4100, 600, 1100
ODD, QUAD = (65, 67), (64, 68)
HW, HW4 = ODD[0] * ODD[1], QUAD[0] * QUAD[1]
PERIOD = 11  # distinct planes where the reference is a scipy call each; neither N_A nor N_B is a multiple of it
LANES = 256


def _ceil(a, b):
    return -(-a // b)


# (kernel, regime): (query, planes, classes, what the library's grid is sized by, items a block's lanes share, turns at
# least).  query 'stride' is blocks_for(n, items, 256, 4096), read off cae_seg_object_counts_workspace: the grid of the
# area filter, cover, object counts and weight map (items = pixels) and of gray, threshold / within and downscale
# (items = groups of 4 pixels, groups of 16, outputs).  query 'predict' is cae_seg_predict's own grid (one block per
# 1024 pixels); its lanes share hw / 4 groups on the 16-byte path and hw single pixels otherwise.
GRIDS = {
    ('gray', 'A'): ('stride', N_A, 1, _ceil(HW, 4), HW // 4, 5),
    ('gray singles', 'A'): ('stride', N_A, 1, _ceil(HW, 4), HW, 5),          # planes off the 4 / 16-byte grids
    ('threshold, within', 'A'): ('stride', N_A, 1, _ceil(HW, 16), HW // 16, 2),
    ('threshold, within singles', 'A'): ('stride', N_A, 1, _ceil(HW, 16), HW, 3),
    ('downscale f=2', 'A'): ('stride', N_A, 1, 33 * 34, 33 * 34, 5),
    ('downscale f=3', 'A'): ('stride', N_A, 1, 22 * 23, 22 * 23, 2),
    ('area filter', 'A'): ('stride', N_A, 1, HW, HW, 18),
    ('area filter', 'B'): ('stride', N_B, 1, HW, HW, 3),
    ('cover', 'A'): ('stride', N_A, 1, HW, HW, 18),
    ('cover', 'B'): ('stride', N_B, 1, HW, HW, 3),
    ('object counts', 'A'): ('stride', N_A, 1, HW, HW, 18),
    ('object counts', 'B'): ('stride', N_B, 1, HW, HW, 3),
    ('weight map', 'A'): ('stride', N_A, 1, HW, HW, 18),
    ('weight map', 'B'): ('stride', N_B, 1, HW, HW, 3),
    ('predict c=1', 'A'): ('predict', N_A, 1, HW, HW // 4, 5),
    ('predict c=3', 'A'): ('predict', N_A, 3, HW4, HW4 // 4, 5),
    ('predict c=17', 'A'): ('predict', N_A, 17, HW, HW, 17),
    ('predict c=1', 'C'): ('predict', N_C, 1, HW, HW // 4, 2),
    ('predict c=3', 'C'): ('predict', N_C, 3, HW4, HW4 // 4, 2),
}
# cae_seg_predict at c = 17 and 600 planes, as the issue asks for it: its 5 blocks per plane are what 1 plane gets, so the
# cap does not bind -- several blocks per plane, merged, each lane 4 turns of single pixels
UNCAPPED = {('predict c=17', 'B'): ('predict', N_B, 17, HW, HW, 3)}
# the count kernel of the area filter: a wave takes one chunk of 1024 pixels at a time, four waves a block
AREA_CHUNK, AREA_WAVES = 1024, 4

# (entry point, bits): (planes, h, w) -- two blocks for one plane, one under the cap
HISTS = {
    ('roc', 8): (1025, 91, 91), ('roc', 14): (257, 91, 91),
    ('object roc', 8): (1025, 211, 311), ('object roc', 14): (257, 211, 311),
}


def blocks_per_plane(L, query, n, c, sized_by):
    """from the library itself: a partial of both entry points is 4 tallies of 8 bytes per (plane, block)"""
    ws = L.cae_seg_predict_workspace(n, c, sized_by) if query == 'predict' else L.cae_seg_object_counts_workspace(n, 1, sized_by)
    assert ws > 0 and ws % (32 * n) == 0
    return ws // (32 * n)


def hist_blocks(L, entry, n, h, w, bits):
    if entry == 'roc':
        return L.cae_seg_roc_blocks(n, h, w, bits)
    ws = L.cae_seg_object_roc_workspace(n, h, w, bits)
    assert ws > 0 and ws % (n * (16 << bits)) == 0  # [n][blocks][2][2^bits] 64-bit words
    return ws // (n * (16 << bits))


def test_the_cases_reach_the_capped_regime(built_lib):
    """no GPU: for every case the library launches fewer blocks per plane than for one plane alone, and the lanes of a
    block share at least twice (where the module says so: three, five, 17, 18 times) as many items as the launch has
    lanes for the plane.  A change of kBlocksTarget or of a launcher's items per block that takes a case out of the
    regime fails here."""
    from cnn_autoencoder_amd import _lib
    L = _lib.lib()
    for key, (query, n, c, sized_by, items, least) in GRIDS.items():
        bx, alone = blocks_per_plane(L, query, n, c, sized_by), blocks_per_plane(L, query, 1, c, sized_by)
        assert bx < alone, (key, bx, alone)
        assert bx == (1 if key[1] == 'A' else 6 if key[1] == 'B' else 3), (key, bx)
        turns = _ceil(items, LANES * bx)
        assert turns >= least >= 2, (key, bx, turns, least)
    for key, (query, n, c, sized_by, items, least) in UNCAPPED.items():
        bx, alone = blocks_per_plane(L, query, n, c, sized_by), blocks_per_plane(L, query, 1, c, sized_by)
        assert 1 < bx == alone and _ceil(items, LANES * bx) >= least, (key, bx, alone)
    # regime B merges partials and ends ragged: 6 blocks, turns of 1536 pixels, the last of 1283
    assert HW - 2 * LANES * 6 == 1283
    # the area filter's count kernel in regime A: 5 chunks on the 4 waves of the one block
    bx = blocks_per_plane(L, *GRIDS['area filter', 'A'][:4])
    assert _ceil(_ceil(HW, AREA_CHUNK), AREA_WAVES * bx) == 2
    for (entry, bits), (n, h, w) in HISTS.items():
        bx, alone = hist_blocks(L, entry, n, h, w, bits), hist_blocks(L, entry, 1, h, w, bits)
        assert bx == 1 and alone == 2, (entry, bits, bx, alone)
    # the shapes are what the module says of them
    assert HW == 4355 and HW % 4 == 3 and HW > 4096 and HW4 % 4 == 0 and HW4 > 4096
    assert N_A % PERIOD and N_B % PERIOD  # neighbouring planes differ and the period does not divide the batch


# ---------------------------------------------------------------------------------------------------------- helpers
def _mods():
    from cnn_autoencoder_amd import _lib, sampler, segmenters, tissue
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return _lib, _lib.lib(), segmenters, tissue, sampler


def planes_of(key):
    return GRIDS[key][1]


def raw_threshold(gray, thr):
    _lib, L, *_ = _mods()
    n, h, w = gray.shape
    out = torch.empty((n, h, w), dtype=torch.uint8, device='cuda')
    _lib.check(L.cae_mask_threshold(gray.data_ptr(), thr.data_ptr(), n, h * w, out.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def raw_within(d2, r2):
    """d2 (n, 2, h, w) int32 on the device -> uint8 (n, h, w): plane 0 within the squared radius"""
    _lib, L, *_ = _mods()
    n, _, h, w = d2.shape
    out = torch.empty((n, h, w), dtype=torch.uint8, device='cuda')
    _lib.check(L.cae_mask_within(d2.data_ptr(), n, h * w, r2, out.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def draw(n, c, hw, seed, sigma=5.0, fine=True):
    """logits (n, c, hw) fp32 with frequent exact ties (half of the pixels hold multiples of a coarse step; all of them
    without `fine`), targets (n, hw) uint8 that include values >= c: every plane has content of its own"""
    rng = np.random.default_rng(seed)
    step = np.float32(4.0 if c > 1 else 0.5)
    x = rng.integers(-12, 13, (n, c, hw), dtype=np.int8).astype(np.float32)
    x *= step
    if fine:
        smooth = rng.standard_normal((n, c, hw), dtype=np.float32)
        smooth *= np.float32(sigma)
        x = np.where(rng.random((n, 1, hw), dtype=np.float32) < 0.5, x, smooth)
    target = rng.integers(0, max(c, 2) + 2, (n, hw), dtype=np.uint8)
    return x, target


# -------------------------------------------------------------------------------------------------- the tissue mask
@functools.lru_cache(maxsize=None)
def images():
    """(N_A, 65, 67, 3) uint8, every plane its own; plane 1 constant; the extremes in the ragged last turn and the tail"""
    rng = np.random.default_rng(65 * 67)
    imgs = rng.integers(0, 256, (N_A,) + ODD + (3,), dtype=np.uint8)
    imgs[1] = (17, 130, 201)
    imgs[2, -1, -1], imgs[3, -1, -1] = 255, 0       # the last pixel: behind the last whole group of four
    imgs[4, -1, -5], imgs[5, -1, -5] = 255, 0       # the last whole group: the ragged last turn
    imgs[N_A - 1, 0, 0], imgs[N_A - 2, -1, -2] = 0, 255
    imgs.setflags(write=False)
    return imgs


@functools.lru_cache(maxsize=None)
def grays():
    g = R.gray(images())
    g.setflags(write=False)
    return g


@gpu
def test_gray_and_its_range(poisoned_alloc):  # noqa: F811
    """one block per plane: five turns of groups of four (the last ragged) and a tail of three where a plane starts on the
    4- and 16-byte grids, 18 turns of single pixels where it does not (offset 1: every plane)"""
    n = planes_of(('gray', 'A'))
    imgs, want = images(), grays()
    flat = want.reshape(n, -1)
    for offset in (0, 1):
        got, minmax = TT.raw_gray(TT.dev(imgs.copy(), offset))
        assert got.dtype == np.float64 and np.array_equal(got, want), offset
        assert np.array_equal(minmax[:, 0], flat.min(axis=1)) and np.array_equal(minmax[:, 1], flat.max(axis=1)), offset
    top = R.gray(np.full((1, 1, 3), 255, dtype=np.uint8))[0, 0]
    assert flat[1].min() == flat[1].max() and flat[2].max() == top == flat[4].max() and flat[3].min() == 0.0 == flat[5].min()
    assert poisoned_alloc.check() > 0


@gpu
def test_threshold_and_within(poisoned_alloc):  # noqa: F811
    """one block per plane: two turns of groups of 16 and three single pixels on the planes that start on the 16-byte
    grid (every 16th of the uint8 output), 18 turns of single pixels on the others.  The threshold of a plane is one of
    its own values, so `<=` holds with equality somewhere; the distances straddle the squared radius and hold -1, and
    their second plane, which is not read, would give another answer"""
    n = planes_of(('threshold, within', 'A'))
    h, w = ODD
    gray = grays()
    rng = np.random.default_rng(3)
    thr = gray.reshape(n, -1)[np.arange(n), rng.integers(0, h * w, n)].copy()
    thr[2], thr[3] = gray[2].max(), gray[3].min()  # everything, and the one darkest pixel
    want = gray <= thr[:, None, None]
    assert want[1].all() and want[2].all() and want[3].sum() >= 1 and 0.2 < want.mean() < 0.8
    got = raw_threshold(TT.dev(gray.copy()), TT.dev(thr))
    assert got.dtype == np.uint8 and np.array_equal(got, want.astype(np.uint8))
    r2 = 25
    d2 = rng.integers(-1, 2 * r2 + 2, (n, 2, h, w)).astype(np.int32)
    d2[:, 1] = np.where(d2[:, 0] <= r2, r2 + 1, 0)
    d2[0, 0].reshape(-1)[-4:] = [r2, r2 + 1, -1, 0]
    inside = (d2[:, 0] >= 0) & (d2[:, 0] <= r2)
    for offset in (0, 1):
        got = raw_within(TT.dev(d2, offset), r2)
        assert np.array_equal(got, inside.astype(np.uint8)), offset
    assert got[0].reshape(-1)[-4:].tolist() == [1, 0, 0, 1]
    assert poisoned_alloc.check() > 0


@gpu
def test_downscale(poisoned_alloc):  # noqa: F811
    """one lane per output pixel: 33 x 34 outputs at f = 2 are five turns of the plane's one block, 22 x 23 at f = 3 two;
    the last output row and column are ragged (65 and 67 are divided by neither)"""
    _, _, _, T, _ = _mods()
    n = planes_of(('downscale f=2', 'A'))
    imgs = images()
    on_dev = TT.dev(imgs.copy())
    h, w = ODD
    for f in (2, 3):
        got = T.downscale(on_dev, f)
        torch.cuda.synchronize()
        assert got.dtype == torch.uint8 and got.shape == (n, _ceil(h, f), _ceil(w, f), 3)
        got = got.cpu().numpy()
        for a in range(0, n, 1025):  # the restatement takes the planes of a slice as channels of one image
            part = imgs[a:a + 1025]
            want = R.downscale(part.transpose(1, 2, 0, 3).reshape(h, w, -1), f)
            want = want.reshape(want.shape[0], want.shape[1], len(part), 3).transpose(2, 0, 1, 3)
            assert np.array_equal(got[a:a + 1025], want), (f, a)
    assert poisoned_alloc.check() > 0


@functools.lru_cache(maxsize=None)
def filter_planes():
    """11 distinct 65 x 67 planes of 0 / 1: blobs, noise, patterns, and one by hand (see test_area_filter)"""
    h, w = ODD
    hand = np.zeros((h, w), dtype=np.uint8)
    hand[15, 14:26] = 1      # 12 pixels in a row across pixel 1024 (row 15, column 19): stays at a limit of 12
    hand[30, 33:44] = 1      # 11 pixels across pixel 2048 (row 30, column 38): goes
    hand[40:61, 5:61] = 1    # 21 x 56 = 1176 pixels: more than a chunk of the count kernel holds
    hand[45, 10:16] = 0      # a hole of 6: stays at a limit of 6
    hand[50, 10:15] = 0      # a hole of 5: filled
    planes = [WO.blobs(h, w, d, 100 + i) for i, d in enumerate((0.15, 0.35, 0.55, 0.75))]
    planes += [(TO.plane(k, h, w) != 0).astype(np.uint8) for k in ('b10', 'b40', 'b60', 'rings', 'comb', 'spiral')]
    planes = np.stack(planes + [hand])
    assert len(planes) == PERIOD
    planes.setflags(write=False)
    return planes


@gpu
@pytest.mark.parametrize('regime', ['A', 'B'])
def test_area_filter(regime, poisoned_alloc):  # noqa: F811
    """A: the plane's one block walks it in 18 turns (init and write) and its four waves take the five chunks of 1024
    pixels in two (count); B: six blocks, three turns, the last of 1283 pixels.  Small objects cleared at 8 neighbours,
    then small holes filled at 4, as tissue_mask does; components on both sides of either limit, across chunk and 64-pixel
    segment borders, and larger than a chunk"""
    n = planes_of(('area filter', regime))
    h, w = ODD
    distinct = filter_planes()
    idx = np.arange(n) % PERIOD
    before = distinct
    for conn, of_zero, least, value in ((8, 0, 12, 0), (4, 1, 6, 1)):
        canon = np.stack([R.canonical_labels((p != 0) != bool(of_zero), conn) for p in before])
        small = np.stack([R.small_components((p != 0) != bool(of_zero), conn, least) for p in before])
        want = np.stack([(p != 0) & ~s if value == 0 else (p != 0) | s for p, s in zip(before, small)])
        # the case is not trivial: components below and at or above the limit, one of them in several chunks
        areas = [np.bincount(c.ravel())[1:] for c in canon]
        sizes = np.concatenate([a[a > 0] for a in areas])
        assert (sizes < least).any() and (sizes == least).any() and (sizes > least).any()
        if not of_zero:
            assert sizes.max() > AREA_CHUNK
        first = np.arange(h * w).reshape(h, w)
        assert any(len(np.unique(first[c == v] // AREA_CHUNK)) > 1 for c in canon for v in np.unique(c)[1:][:40])
        target = TT.dev(before[idx], offset=1)
        labels = TT.raw_label(target, conn, of_zero)
        assert np.array_equal(labels.cpu().numpy(), canon[idx]), (conn, of_zero)
        got, wide = TT.raw_area_filter(labels, target, least, value, wide=True)
        assert np.array_equal(got != 0, want[idx]), (regime, conn, of_zero, least)
        assert set(np.unique(got)) <= {0, 1} and wide.dtype == np.int32 and np.array_equal(wide, (got != 0).astype(np.int32))
        before = want.astype(np.uint8)
    hand = want[PERIOD - 1]
    assert hand[15, 14:26].all() and not hand[30, 33:44].any() and not hand[45, 10:16].any() and hand[50, 10:15].all()
    assert poisoned_alloc.check() > 0


# ------------------------------------------------------------------------------------------- class map, counts, scores
def judge_predict(key, offsets, seed, with_scores=True, fine=True):
    """cae_seg_predict on the case `key` of GRIDS: class map and counts equal to numpy's on the same logits, scores within
    4 E + 2^-24 of float64, and the same decisions without the score stores; the oracle once for all offsets"""
    _, _, S, _, _ = _mods()
    _, n, c, hw, _, _ = (GRIDS.get(key) or UNCAPPED[key])
    assert hw == (HW4 if 1 < c <= 16 else HW)
    logits, target = draw(n, c, hw, seed, fine=fine)
    cls, counts = np.empty((n, hw), dtype=np.uint8), np.empty((n, 6), dtype=np.int64)

    def part(a):  # in slices: the oracle's temporaries are several times the logits; numpy runs them side by side
        cls[a:a + 128], counts[a:a + 128] = TP.oracle(logits[a:a + 128], target[a:a + 128], np.float32(0), 5)
    with ThreadPoolExecutor(4) as pool:
        list(pool.map(part, range(0, n, 128)))
    if with_scores:
        f64 = TP.scores_f64(logits)
        # test_seg_predict.score_bound, 4 E + 2^-24 with E of torch's CPU float32 op, on the float64 scores made above
        x = torch.from_numpy(logits)
        ref = (torch.sigmoid(x) if c == 1 else torch.softmax(x, dim=1)).numpy()
        bound = 4.0 * float(np.abs(ref - f64).max()) + 2.0 ** -24
        assert TP.score_bound(logits[:1]) <= bound  # (the rule itself on one plane: a maximum over fewer pixels)
        del x, ref
    for offset in offsets:
        lg, tg = TP.on_device(logits, offset), TP.on_device(target, 0)
        if with_scores:
            got = S.predict(lg, tg, scores=True)
            torch.cuda.synchronize()
            assert np.array_equal(got['cls'].cpu().numpy(), cls), (key, offset)
            assert np.array_equal(got['counts'].cpu().numpy(), counts), (key, offset)
            sc = got['scores'].cpu().numpy()
            err = float(np.abs(sc.astype(np.float64) - f64).max())
            print(f'{key} offset {offset}: score error {err:.3e}, bound {bound:.3e}')
            assert np.isfinite(sc).all() and err <= bound, (key, offset, err, bound)
            del got, sc
        plain = S.predict(lg, tg, scores=False)
        torch.cuda.synchronize()
        assert plain['scores'] is None and np.array_equal(plain['cls'].cpu().numpy(), cls), (key, offset)
        assert np.array_equal(plain['counts'].cpu().numpy(), counts), (key, offset)
        bare = S.predict(lg, None, scores=False)  # no target: no tallies, no workspace
        assert bare['counts'] is None and np.array_equal(bare['cls'].cpu().numpy(), cls), (key, offset)
    assert counts[:, 0].min() > 0 and (counts[:, 5] > counts[:, 0]).any() == (c > 1)


@gpu
@pytest.mark.parametrize('regime', ['A', 'C'])
def test_predict_one_class(regime, poisoned_alloc):  # noqa: F811
    """65 x 67 planes: every plane at another offset within 16 bytes, so heads and tails of up to three single pixels
    beside 1088 groups of four; A: five turns of the one block; C: three blocks, two turns, partials merged"""
    judge_predict(('predict c=1', regime), (0, 1), 11)
    assert poisoned_alloc.check() > 0


@gpu
@pytest.mark.parametrize('regime', ['A', 'C'])
def test_predict_three_classes_in_registers(regime, poisoned_alloc):  # noqa: F811
    """64 x 68 planes (hw % 4 == 0: the 16-byte path for several classes); offset 1 adds the scalar head and tail, byte
    stores of the class map and scalar score stores"""
    judge_predict(('predict c=3', regime), (0, 1), 13)
    assert poisoned_alloc.check() > 0


@gpu
def test_predict_streamed_classes_with_six_hundred_planes(poisoned_alloc):  # noqa: F811
    """c = 17, the first streamed count, with scores and without: five blocks per plane (the cap of 6 does not bind this
    grid, see UNCAPPED), four turns of single pixels, the partials of the five merged per plane"""
    judge_predict(('predict c=17', 'B'), (1,), 17)
    assert poisoned_alloc.check() > 0


@gpu
def test_predict_streamed_classes_with_more_planes_than_blocks(poisoned_alloc):  # noqa: F811
    """c = 17 and 4100 planes, one block each: 18 turns of single pixels.  303 M logits: multiples of 4 only (cheap to
    draw, ties of the maximum and across the top-k border everywhere), class map and counts with and without a target;
    the scores of the streamed path are judged at 600 planes"""
    judge_predict(('predict c=17', 'A'), (0,), 19, with_scores=False, fine=False)
    assert poisoned_alloc.check() > 0


# -------------------------------------------------------------------------------------------- objects: cover, counts
COVER_NAMES = ('b10', 'rings', 'empty', 'b40', 'spiral', 'grid', 'b60', 'comb', 'full', 'antidiagonal', 'rows')


def cover_extents():
    h, w = ODD
    return [(h, w), (h - 2, w - 3), (h, w), (h // 2 + 1, w), (h, w - 1), (h, w), (h + 10, w + 10), (h, w), (h - 1, w),
            (h, w // 2), (h, w)]


@gpu
@pytest.mark.parametrize('regime', ['A', 'B'])
def test_object_cover(regime, poisoned_alloc):  # noqa: F811
    """obj_box_init, obj_box and obj_corner walk a plane in 18 turns of one block (A) or three turns of six (B); labels,
    numbers and cover of the patterns of test_seg_objects with whole and ragged extents"""
    _, _, S, _, _ = _mods()
    n = planes_of(('cover', regime))
    h, w = ODD
    assert len(COVER_NAMES) == PERIOD == len(cover_extents())
    idx = np.arange(n) % PERIOD
    truth = [TO.truth(k, h, w, False, e) for k, e in zip(COVER_NAMES, cover_extents())]
    target = np.stack([TO.plane(k, h, w) for k in COVER_NAMES])[idx]
    extent = np.array(cover_extents())[idx]
    labels, count, cover = TO.run_objects(S, target, extent, offset=1)
    assert np.array_equal(labels, np.stack([t[0] for t in truth])[idx])
    assert np.array_equal(count, np.array([t[1] for t in truth])[idx])
    assert np.array_equal(cover, np.stack([t[3] for t in truth])[idx])
    assert cover.max() >= 4 and count.max() > 100 and count.min() == 0
    assert poisoned_alloc.check() > 0


def weighted_record(logits, target, cover, t, top_k):
    """(n, c, hw) fp32, (n, hw) uint8, (n, hw) integer weights -> (n, 6) int64: the statements of seg_objects_oracle.record
    with every pixel counted `cover` times (what seg_objects_oracle.weighted_counts gets by repeating pixels, plane by
    plane), all planes at once"""
    n, c, hw = logits.shape
    cv = cover.astype(np.int64)
    if c == 1:
        on, pos = logits[:, 0] > np.float32(t), target > 0
        tp, tn = (cv * (on & pos)).sum(1), (cv * (~on & ~pos)).sum(1)
        fp, fn = (cv * (on & ~pos)).sum(1), (cv * (~on & pos)).sum(1)
        return np.stack([tp, tn, fp, fn, (cv * pos).sum(1), tp], axis=1)
    best, idx = logits[:, 0].copy(), np.zeros((n, hw), dtype=np.int64)
    for j in range(1, c):
        wins = logits[:, j] > best
        best, idx = np.where(wins, logits[:, j], best), np.where(wins, j, idx)
    tgt = target.astype(np.int64)
    lt = np.take_along_axis(logits, np.minimum(tgt, c - 1)[:, None, :], axis=1)
    below = np.arange(c)[None, :, None] < tgt[:, None, :]
    rank = (logits > lt).sum(1) + ((logits == lt) & below).sum(1)
    tp = (cv * (idx == tgt)).sum(1)
    top = (cv * ((tgt < c) & (rank < min(top_k, c)))).sum(1)
    full = cv.sum(1)
    return np.stack([tp, 0 * tp, full - tp, full - tp, full, top], axis=1)


@gpu
@pytest.mark.parametrize('c', [1, 3])
@pytest.mark.parametrize('regime', ['A', 'B'])
def test_object_counts(regime, c, poisoned_alloc):  # noqa: F811
    """obj_tally_kernel (one class, and the streamed decisions of several) over 18 turns of one block or three of six,
    the six partials merged per plane: logits and targets of each plane's own, the cover that of the patterns (zeros are
    skipped, no pixel counts twice) with 65535 planted at pixels of the last turn"""
    _, _, S, _, _ = _mods()
    n = planes_of(('object counts', regime))
    h, w = ODD
    idx = np.arange(n) % PERIOD
    cover = np.stack([TO.truth(k, h, w)[3] for k in COVER_NAMES]).astype(np.uint16)[idx].reshape(n, -1)
    cover[::7, -1], cover[3::7, -1300] = 65535, 65535
    logits, target = draw(n, c, h * w, 23 + c)
    thr, top_k = 0.8, 2  # neither is the default
    t = np.float32(S.threshold_logit(thr))
    want = weighted_record(logits, target, cover, t, top_k)
    few = slice(0, 2 * PERIOD, 3)  # the restatement as it stands on some planes, for the weights up to 9
    assert np.array_equal(want[few], OO.weighted_counts(logits[few], target[few], np.minimum(cover[few], 9), t, top_k)
                          + weighted_record(logits[few], target[few], cover[few] - np.minimum(cover[few], 9), t, top_k))
    got = S.object_counts(TO.dev(logits, 1), TO.dev(target, 1), TO.dev(cover), threshold=thr, top_k=top_k)
    torch.cuda.synchronize()
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), (regime, c)
    assert want[:, 4].max() > 65535 and (want[2::PERIOD, 4] <= 2 * 65535).all()  # (the empty pattern: planted only)
    assert poisoned_alloc.check() > 0


# --------------------------------------------------------------------------------------- distances and the weight map
@functools.lru_cache(maxsize=None)
def weight_planes():
    """11 distinct 65 x 67 planes: no object, one, and blobs with several"""
    h, w = ODD
    one = np.zeros((h, w), dtype=np.uint8)
    one[20:30, 40:60] = 1
    planes = [np.zeros((h, w), dtype=np.uint8), one]
    planes += [WO.blobs(h, w, d, 200 + i) for i, d in enumerate((0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.4, 0.5, 0.6))]
    planes = np.stack(planes)
    assert len(planes) == PERIOD
    planes.setflags(write=False)
    return planes


@functools.lru_cache(maxsize=None)
def weight_oracle(sigma):
    return [WO.weight_map(p, [0.75, 3.0], sigma=sigma, w_0=10) for p in weight_planes()]


@gpu
@pytest.mark.parametrize('regime', ['A', 'B'])
def test_distances_within_and_weight_map(regime, poisoned_alloc):  # noqa: F811
    """wd_map_kernel walks a plane in 18 turns of one block (A) or three of six (B); the squared distances it reads are
    equal to scipy's, the disk test on them is scipy's dilation, and the three maps of test_seg_weight_map (exponential
    part, class weights, both) hold that file's bound per pixel; planes without, with one and with several objects, which
    take different forms of the weight, side by side"""
    _, _, S, _, sampler = _mods()
    n = planes_of(('weight map', regime))
    sigma = 5
    distinct, oracle = weight_planes(), weight_oracle(sigma)
    idx = np.arange(n) % PERIOD
    counts = np.array([o['count'] for o in oracle])
    assert counts[0] == 0 and counts[1] == 1 and (counts[2:] > 1).all()
    planes = distinct[idx]
    labels, count = S.components(TO.dev(planes))
    d2 = S.object_distances(labels)
    torch.cuda.synchronize()
    assert np.array_equal(count.cpu().numpy(), counts[idx])
    assert np.array_equal(d2.cpu().numpy(), np.stack([o['d2'] for o in oracle])[idx])
    for radius in (0, 3):
        want = np.stack([R.dilate(p != 0, radius) for p in distinct])
        assert np.array_equal(raw_within(d2, radius * radius) != 0, want[idx]), radius
    del d2, labels
    # the maps
    t = TO.dev(planes.astype(np.float32))[:, None]
    wd = sampler.WeightsDistances
    e_dev = wd([0.0, 0.0], sigma=sigma, w_0=1)(t).cpu().numpy()
    cw_dev = wd([0.75, 3.0], sigma=sigma, w_0=0)(t).cpu().numpy()
    full_dev = wd([0.75, 3.0], sigma=sigma, w_0=10)(t).cpu().numpy()
    cw = np.where(distinct > 0, np.float32(3.0), np.float32(0.75))
    assert np.array_equal(cw_dev[:, 0], cw[idx])
    for got in (e_dev, cw_dev, full_dev):
        assert np.array_equal(got[:, 1], planes.astype(np.float32))
    # per distinct plane: the oracle's values and what may lie between; a plane without objects is exact (bound 0)
    e = np.stack([o['e'] for o in oracle])
    w64 = np.stack([o['w64'] for o in oracle])
    tol = np.stack([np.zeros(ODD) if o['count'] == 0 else WO.bound(o['arg'], o['e']) for o in oracle])
    tol_full = 10.0 * tol + 2.0 ** -23 * w64 * (1.0 + 2.0 ** -10)
    tol_full[0] = 0.0
    assert np.array_equal(w64[0], cw[0].astype(np.float64)) and not e[0].any()
    err = np.abs(e_dev[:, 0].astype(np.float64) - e[idx])
    print(f'{regime}: worst exponential error / bound {float((err[idx != 0] / tol[idx][idx != 0]).max()):.3f}')
    assert (err <= tol[idx]).all()
    assert (np.abs(full_dev[:, 0].astype(np.float64) - w64[idx]) <= tol_full[idx]).all()
    assert poisoned_alloc.check() > 0


# --------------------------------------------------------------------------------------------------------- histograms
def hist_inputs(n, h, w, seed):
    """logits (n, 1, h, w) of each plane's own with +-inf, NaN and -0 planted, a uint8 target with many non-zero values,
    ragged extents: whole, empty both ways, beyond the plane, and random"""
    rng = np.random.default_rng(seed)
    logits = draw(n, 1, h * w, seed)[0]
    flat = logits.reshape(-1)
    flat[::1009], flat[1::2003], flat[2::3001], flat[3::4001], flat[4::5003] = np.inf, -np.inf, np.nan, -0.0, -np.nan
    target = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    target[target < 179] = 0  # 30 % positives, of 77 values
    extent = np.stack([rng.integers(0, h + 2, n), rng.integers(0, w + 2, n)], axis=1)
    extent[::3] = (h, w)
    extent[1], extent[2], extent[4] = (0, w), (h, 0), (h + 10, w - 1)
    return logits.reshape(n, 1, h, w), target, extent


@gpu
@pytest.mark.parametrize('bits', [8, 14])
def test_roc_histograms_with_more_planes_than_blocks(bits, poisoned_alloc):  # noqa: F811
    """1025 planes at 8 bits, 257 at 14: one block takes the 8281 pixels that two share below the cap; per image and
    summed over the batch, logits on and off the 16-byte grid"""
    _, _, S, _, _ = _mods()
    n, h, w = HISTS['roc', bits]
    logits, target, extent = hist_inputs(n, h, w, bits)
    want = RO.histogram(logits, target, bits, extent, per_image=True)
    assert want[1].sum() == 0 and want[2].sum() == 0 and want[0].sum() == h * w and want[4].sum() == h * (w - 1)
    for offset in (0, 1):
        lg, tg = TO.dev(logits, offset), TO.dev(target, 1)
        got = S.roc_histogram(lg, tg, extent=extent, bits=bits, per_image=True)
        total = S.roc_histogram(lg, tg, extent=extent, bits=bits)
        torch.cuda.synchronize()
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), (bits, offset)
        assert np.array_equal(total.cpu().numpy(), want.sum(axis=0)), (bits, offset)
    assert poisoned_alloc.check() > 0


def weighted_histogram(logits, target, weight, bits, extent):
    """seg_objects_oracle.weighted_histogram per image (the bin of seg_roc_oracle, integer weights, the extent), all
    planes in one numpy.bincount per row instead of one numpy.add.at per plane: sums below 2^53 are exact in its float64"""
    n, _, h, w = logits.shape
    B = 1 << bits
    rows = np.clip(extent[:, 0], 0, h)[:, None, None]
    cols = np.clip(extent[:, 1], 0, w)[:, None, None]
    counted = (np.arange(h)[None, :, None] < rows) & (np.arange(w)[None, None, :] < cols)
    word = np.arange(n)[:, None, None] * (2 * B) + np.where(target > 0, B, 0) + RO.bin_of(logits[:, 0], bits)
    wt = np.where(counted, weight, 0).astype(np.float64)
    assert wt.sum() < 2.0 ** 53
    return np.bincount(word.reshape(-1), weights=wt.reshape(-1), minlength=n * 2 * B).astype(np.int64).reshape(n, 2, B)


@gpu
@pytest.mark.parametrize('bits', [8, 14])
def test_object_roc_histograms_with_more_planes_than_blocks(bits, poisoned_alloc):  # noqa: F811
    """211 x 311 = 65621 pixels, 85 more than a block's chunk: one block where two are launched below the cap, which
    flushes its 32-bit words once on the way; any uint16 weights, 65535 among them"""
    _, _, S, _, _ = _mods()
    n, h, w = HISTS['object roc', bits]
    logits, target, extent = hist_inputs(n, h, w, 40 + bits)
    rng = np.random.default_rng(bits)
    cover = rng.integers(0, 4, (n, h, w), dtype=np.uint16)
    cover.reshape(-1)[::4099] = 65535
    cover[:, -1, -1], logits[:, 0, -1, -1] = 65535, 1.5  # the last pixel of every plane: behind the flush
    want = weighted_histogram(logits, target, cover, bits, extent)
    few = slice(0, 5)  # the restatement as it stands, on the planes with the planted extents
    assert np.array_equal(want[few], OO.weighted_histogram(logits[few], target[few], cover[few], bits, extent[few], per_image=True))
    assert want[0].sum() > 65535 and want[1].sum() == 0 and want[2].sum() == 0
    lg, tg, cv = TO.dev(logits, 1), TO.dev(target, 1), TO.dev(cover)
    got = S.object_roc_histogram(lg, tg, cv, extent=extent, bits=bits, per_image=True)
    total = S.object_roc_histogram(lg, tg, cv, extent=extent, bits=bits)
    torch.cuda.synchronize()
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), bits
    assert np.array_equal(total.cpu().numpy(), want.sum(axis=0)), bits
    assert poisoned_alloc.check() > 0
