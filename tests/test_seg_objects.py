"""The object-level entry points on the GPU (csrc/cae_seg_objects.hip) and what is built on them: segmenters.components,
object_cover, object_counts, object_roc_histogram, SlideCoder.segment_batches(object_level=True),
zarrio.segment_image(object_level=True).

Everything is an integer and is compared for equality with the restatement (tests/seg_objects_oracle.py), which makes the
object-level record and histogram as the reference does: from the concatenated pixels of the boxes, without a cover.
NaN and +-inf logits are planted for every class count, at pixels the cover counts.  For several classes the record comes
from seg_objects_oracle.record, which states the contract's strict-greater argmax (a NaN never wins; numpy's argmax, which
test_seg_predict's oracle uses, returns the first NaN), and with cover 1 from cae_seg_predict itself.
"""
import functools

import numpy as np
import pytest
import torch

import seg_objects_oracle as OO
import seg_roc_oracle as RO
import test_seg_predict as TP
from residue import poisoned_alloc  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 2), (7, 9), (16, 16), (33, 65), (65, 130), (264, 265)]  # the last: several blocks both ways
PATTERNS = ('empty', 'full', 'grid', 'spiral', 'comb', 'antidiagonal', 'rings', 'rows', 'b10', 'b40', 'b60', 'b90')


def _seg():
    from cnn_autoencoder_amd import segmenters
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return segmenters


# ------------------------------------------------------------------------------------------------------ patterns
def _spiral(h, w):
    """a one-pixel-wide path that winds inwards with one pixel of background between its turns: one object"""
    a = np.zeros((h, w), dtype=bool)
    y = x = 0
    dy, dx = 0, 1
    a[0, 0] = True
    free = lambda yy, xx: not (0 <= yy < h and 0 <= xx < w) or not a[yy, xx]  # noqa: E731
    while True:
        for _ in range(2):
            ny, nx = y + dy, x + dx
            if 0 <= ny < h and 0 <= nx < w and not a[ny, nx] and free(ny + dy, nx + dx):
                break
            dy, dx = dx, -dy  # turn right
        else:
            return a
        y, x = ny, nx
        a[y, x] = True


@functools.lru_cache(maxsize=None)
def plane(name, h, w):
    a = np.zeros((h, w), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    if name == 'full':
        a[:] = 1
    elif name == 'grid':  # isolated pixels on the even grid: the most objects a plane holds
        a[::2, ::2] = 1
    elif name == 'spiral':
        a[_spiral(h, w)] = 1
    elif name == 'comb':  # teeth that join only along the far edge
        a[:, ::2] = 1
        a[h - 1, :] = 1
    elif name == 'antidiagonal':  # lines that hold together by corners only
        a[(yy + xx) % 3 == 0] = 1
    elif name == 'rings':  # nested boxes, a high cover in the middle
        a[np.minimum(np.minimum(yy, xx), np.minimum(h - 1 - yy, w - 1 - xx)) % 2 == 0] = 1
    elif name == 'rows':
        a[::2, :] = 1
    elif name.startswith('b'):
        rng = np.random.default_rng(h * 1000 + w + int(name[1:]))
        a[rng.random((h, w)) < int(name[1:]) / 100.0] = 200
    elif name.startswith('v'):  # values for by_value
        rng = np.random.default_rng(h * 1000 + w + int(name[1:]))
        a[:] = rng.choice(np.array([0, 1, 2, 255], dtype=np.uint8), (h, w), p=[1 - int(name[1:]) / 100.0] + [int(name[1:]) / 300.0] * 3)
    else:
        assert name == 'empty', name
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def truth(name, h, w, by_value=False, extent=None):
    """the restatement of one plane, computed once: (labels (H,W), n_objects, boxes, cover (H,W))"""
    ext = None if extent is None else [extent]
    labels, count, boxes = OO.components(plane(name, h, w)[None], extent=ext, by_value=by_value)
    return labels[0], int(count[0]), boxes[0], OO.cover(boxes, h, w)[0]


def dev(arr, offset=0):
    return TP.on_device(np.ascontiguousarray(arr), offset)


def run_objects(S, target, extent=None, by_value=False, offset=0):
    labels, count = S.components(dev(target, offset), extent=extent, by_value=by_value)
    cover = S.object_cover(labels, extent=extent)
    torch.cuda.synchronize()
    assert labels.dtype == torch.int32 and count.dtype == torch.int64 and cover.dtype == torch.uint16
    return labels.cpu().numpy(), count.cpu().numpy(), cover.cpu().numpy()


def judge_objects(S, names, h, w, by_value=False, extents=None, offset=0):
    n = len(names)
    target = np.stack([plane(k, h, w) for k in names])
    want = [truth(k, h, w, by_value, None if extents is None else tuple(int(v) for v in extents[i])) for i, k in enumerate(names)]
    labels, count, cover = run_objects(S, target, None if extents is None else np.asarray(extents), by_value, offset)
    what = (names, h, w, by_value, extents, offset)
    assert labels.shape == (n, h, w) and count.shape == (n,) and cover.shape == (n, h, w)
    for i in range(n):
        assert np.array_equal(labels[i], want[i][0]), (what, i)
        assert count[i] == want[i][1], (what, i, count[i], want[i][1])
        assert np.array_equal(cover[i], want[i][3]), (what, i)
    return labels, count, cover


# ------------------------------------------------------------------------------------------ labels, numbers, cover
@pytest.mark.parametrize('shape', SHAPES)
def test_labels_numbers_and_cover_of_the_patterns(shape):
    """every pattern alone (N = 1) and three at a time (N = 3), targets at byte offsets 0 and 1"""
    S = _seg()
    h, w = shape
    for i, name in enumerate(PATTERNS):
        judge_objects(S, [name], h, w, offset=i % 2)
    for i in range(0, len(PATTERNS), 3):
        judge_objects(S, list(PATTERNS[i:i + 3]), h, w, offset=(i // 3 + 1) % 2)
    assert truth('grid', h, w)[1] == -(-h // 2) * -(-w // 2)
    assert truth('spiral', h, w)[1] == 1 and truth('comb', h, w)[1] == 1 and truth('full', h, w)[1] == 1
    if min(h, w) >= 16:
        assert truth('antidiagonal', h, w)[1] > 1 and truth('rings', h, w)[3].max() >= 4


@pytest.mark.parametrize('shape', SHAPES)
def test_objects_by_value(shape):
    """labels {0, 1, 2, 255}: neighbours of different values stay apart; the same planes without by_value for comparison"""
    S = _seg()
    h, w = shape
    names = ['v30', 'v60', 'v90']
    _, by_value, _ = judge_objects(S, names, h, w, by_value=True, offset=1)
    _, merged, _ = judge_objects(S, names, h, w, by_value=False)
    assert (by_value >= merged).all()
    judge_objects(S, ['v60'], h, w, by_value=True)
    if h * w > 100:
        assert (by_value > merged).any()


@pytest.mark.parametrize('shape', [(7, 9), (33, 65), (264, 265)])
def test_extents(shape):
    """full, ragged, empty, per image and out of range: a pixel outside the extent is background, boxes stop at it"""
    S = _seg()
    h, w = shape
    for names in (['b40', 'rings', 'full'], ['spiral', 'comb', 'b60']):
        for extents in ([(h, w)] * 3, [(h - 2, w - 3)] * 3, [(0, w), (h, 0), (0, 0)], [(h, w - 1), (h // 2, w), (1, 1)],
                        [(h + 10, w + 10), (-4, w), (2 ** 31 - 1, -2 ** 31)], [(h // 2 + 1, w // 2 + 1), (h, 1), (1, w)]):
            judge_objects(S, names, h, w, extents=extents)
            judge_objects(S, names, h, w, by_value=True, extents=extents, offset=1)
    empty = run_objects(S, np.stack([plane('full', h, w)] * 2), extent=np.array([(0, w), (h, 0)]))
    assert not empty[0].any() and not empty[1].any() and not empty[2].any()


def test_results_do_not_depend_on_what_the_buffers_held(poisoned_alloc):  # noqa: F811
    """outputs and workspaces come poisoned from torch.empty; nothing is written outside them"""
    S = _seg()
    for (h, w), names in (((33, 65), ['b40', 'rings', 'empty']), ((264, 265), ['b10', 'spiral', 'grid'])):
        labels, count, cover = judge_objects(S, names, h, w, extents=[(h, w), (h - 1, w - 2), (h, w)])
        rng = np.random.default_rng(h)
        target = np.stack([plane(k, h, w) for k in names])
        logits = (3 * rng.standard_normal((3, 1, h, w))).astype(np.float32)
        boxes = [truth(k, h, w, False, e)[2] for k, e in zip(names, [(h, w), (h - 1, w - 2), (h, w)])]
        got = S.object_counts(dev(logits), dev(target), dev(cover.astype(np.uint16)))
        hist = S.object_roc_histogram(dev(logits), dev(target), dev(cover.astype(np.uint16)), bits=14, per_image=True)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), OO.object_counts(logits, target, boxes, np.float32(0), 5))
        assert np.array_equal(hist.cpu().numpy(), OO.object_histogram(logits, target, boxes, 14, per_image=True))
    assert poisoned_alloc.check() > 0


def _raw(S, target, labels, count, cover, ws, by_value=0):
    """cae_seg_components and cae_seg_object_cover on the caller's own buffers"""
    from cnn_autoencoder_amd import _lib
    L = _lib.lib()
    n, h, w = target.shape
    assert ws.numel() * 8 >= max(L.cae_seg_components_workspace(n, h, w), L.cae_seg_object_cover_workspace(n, h, w))
    _lib.check(L.cae_seg_components(target.data_ptr(), None, n, h, w, by_value, labels.data_ptr(), count.data_ptr(),
                                    ws.data_ptr(), ws.numel() * 8, _lib.stream_ptr()))
    _lib.check(L.cae_seg_object_cover(labels.data_ptr(), None, n, h, w, cover.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                      _lib.stream_ptr()))
    torch.cuda.synchronize()
    k = n * h * w
    return (labels.view(-1)[:k].view(n, h, w).cpu().numpy(), count[:n].cpu().numpy(), cover.view(-1)[:k].view(n, h, w).cpu().numpy())


def test_a_small_call_after_a_large_one_on_the_same_buffers_and_two_equal_runs():
    S = _seg()
    big, small = (3, 264, 265), (2, 7, 9)
    k = big[0] * big[1] * big[2]
    labels = torch.zeros(k, dtype=torch.int32, device='cuda')
    count = torch.zeros(big[0], dtype=torch.int64, device='cuda')
    cover = torch.zeros(k, dtype=torch.uint16, device='cuda')
    ws = torch.zeros(2 * k + 64, dtype=torch.int64, device='cuda')
    first = None
    for names, (n, h, w) in ((['b40', 'spiral', 'grid'], big), (['b40', 'rings'], small), (['b40', 'spiral', 'grid'], big),
                             (['b40', 'rings'], small)):
        target = dev(np.stack([plane(name, h, w) for name in names]))
        got = _raw(S, target, labels, count, cover, ws)
        for i, name in enumerate(names):
            want = truth(name, h, w)
            assert np.array_equal(got[0][i], want[0]) and got[1][i] == want[1] and np.array_equal(got[2][i], want[3]), (name, h, w)
        if (n, h, w) == big:
            if first is None:
                first = got
            else:  # the same call again: the same bits
                assert all(np.array_equal(a, b) for a, b in zip(first, got))


# ---------------------------------------------------------------------------------------- counts and histograms
SPOTS = 10  # pixels of every plane that get a planted value


def _logits(n, c, h, w, seed, target=None, cover=None):
    """logits (n,c,h,w) with ties (TP.draw) and, in every plane of at least SPOTS pixels, planted +-inf and NaN at the
    first SPOTS pixels that the cover counts (the first pixels of the plane where it counts fewer): +inf and -inf in single
    classes, every class +inf; one class: NaN of both signs; several: a whole pixel of NaN, NaN in class 0, in the last
    class, in class 1, in the target's class, in class 0 and the target's class, and in every class but the last"""
    x, _ = TP.draw(n, c, h * w, seed)
    flat = x.reshape(n, c, -1)
    for i in range(n if h * w >= SPOTS else 0):
        s = np.flatnonzero(np.asarray(cover[i]).reshape(-1))[:SPOTS] if cover is not None else np.arange(SPOTS)
        s = s if s.size == SPOTS else np.arange(SPOTS)
        tc = [int(v) if v < c else 0 for v in (np.asarray(target[i]).reshape(-1)[s] if target is not None else np.zeros(SPOTS))]
        flat[i, 0, s[0]], flat[i, c - 1, s[1]], flat[i, :, s[2]] = np.inf, -np.inf, np.inf
        if c == 1:
            flat[i, 0, s[3]], flat[i, 0, s[4]] = np.nan, -np.nan
        else:
            flat[i, :, s[3]], flat[i, 0, s[4]], flat[i, c - 1, s[5]], flat[i, 1, s[6]] = np.nan, np.nan, np.nan, -np.nan
            flat[i, tc[7], s[7]] = np.nan
            flat[i, 0, s[8]], flat[i, tc[8], s[8]] = np.nan, np.nan
            flat[i, :c - 1, s[9]] = np.nan
    return x.reshape(n, c, h, w)


@pytest.mark.parametrize('offset', [0, 3])
@pytest.mark.parametrize('c', [1, 3, 17])
def test_object_counts_are_the_record_of_the_concatenated_boxes(c, offset):
    S = _seg()
    for (h, w), names in (((7, 9), ['v30', 'rings', 'grid']), ((33, 65), ['v60', 'b40', 'rings']), ((264, 265), ['b10', 'v30', 'rows'])):
        n = len(names)
        by_value = c > 1
        target = np.stack([plane(k, h, w) for k in names])
        if c > 1:
            target = np.where(target > 0, (target.astype(np.int64) + np.arange(h * w).reshape(h, w) % 3) % (c + 2), 0).astype(np.uint8)
        labels, count, boxes = OO.components(target, by_value=by_value)
        cover = OO.cover(boxes, h, w)
        logits = _logits(n, c, h, w, 7 * c + h, target, cover)
        if h * w > 100:  # the planted values are where the cover counts them
            assert all(int(np.isnan(logits[i]).any(axis=0)[cover[i] > 0].sum()) >= (2 if c == 1 else 6) for i in range(n))
        for thr, top_k in ((0.5, 5), (0.8, 2)):
            t = np.float32(S.threshold_logit(thr))
            got = S.object_counts(dev(logits, offset), dev(target, 1), dev(cover.astype(np.uint16)), threshold=thr, top_k=top_k)
            torch.cuda.synchronize()
            want = OO.object_counts(logits, target, boxes, t, top_k)
            assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), (c, h, w, thr, got.cpu().numpy(), want)
        # the device's own cover gives the same record
        lab_d, _ = S.components(dev(target), by_value=by_value)
        own = S.object_counts(dev(logits), dev(target), S.object_cover(lab_d))
        torch.cuda.synchronize()
        assert np.array_equal(own.cpu().numpy(), OO.object_counts(logits, target, boxes, np.float32(0), 5))
        # cover 1 everywhere: the record of cae_seg_predict
        ones = dev(np.ones((n, h, w), dtype=np.uint16))
        for top_k in (5, 1):
            plain = S.predict(dev(logits), dev(target), top_k=top_k)['counts']
            same = S.object_counts(dev(logits), dev(target), ones, top_k=top_k)
            torch.cuda.synchronize()
            assert torch.equal(plain, same)
            assert np.array_equal(same.cpu().numpy(), OO.record(logits.reshape(n, c, -1), target.reshape(n, -1), np.float32(0), top_k))


@pytest.mark.parametrize('offset', [0, 3])
@pytest.mark.parametrize('bits', [8, 14])
def test_object_histograms_are_those_of_the_concatenated_boxes(bits, offset):
    S = _seg()
    for (h, w), names in (((7, 9), ['b40', 'rings', 'grid']), ((33, 65), ['b60', 'b40', 'rings']), ((264, 265), ['b10', 'rows', 'rings'])):
        n = len(names)
        target = np.stack([plane(k, h, w) for k in names])
        logits = _logits(n, 1, h, w, bits + h, target, target)  # planted on the objects: inside every cover below
        for extents in (None, [(h, w), (h - 1, w - 2), (h // 2, w)]):
            _, _, boxes = OO.components(target, extent=extents)
            cover = OO.cover(boxes, h, w).astype(np.uint16)
            for per_image in (False, True):
                got = S.object_roc_histogram(dev(logits, offset), dev(target, 1), dev(cover), extent=extents, bits=bits,
                                             per_image=per_image)
                torch.cuda.synchronize()
                assert got.dtype == torch.int64 and got.shape == ((n, 2, 1 << bits) if per_image else (2, 1 << bits))
                assert np.array_equal(got.cpu().numpy(), OO.object_histogram(logits, target, boxes, bits, per_image=per_image))
            # weights outside the extent are not counted
            noisy = cover.copy()
            if extents is not None:
                noisy[1, h - 1:, :], noisy[1, :, w - 2:] = 9, 9
                got = S.object_roc_histogram(dev(logits), dev(target), dev(noisy), extent=extents, bits=bits)
                torch.cuda.synchronize()
                assert np.array_equal(got.cpu().numpy(), OO.object_histogram(logits, target, boxes, bits))
        # cover 1 everywhere: the histogram of cae_seg_roc_hist
        ones = dev(np.ones((n, h, w), dtype=np.uint16))
        ext = [(h, w - 1), (h - 3, w), (h, w)]
        plain = S.roc_histogram(dev(logits), dev(target), extent=ext, bits=bits, per_image=True)
        same = S.object_roc_histogram(dev(logits), dev(target), ones, extent=ext, bits=bits, per_image=True)
        torch.cuda.synchronize()
        assert torch.equal(plain, same)


def test_object_histograms_merge_more_partials_than_the_merge_kernel_has_waves():
    """5 planes of 264 x 265 are two blocks each: 10 sources of 64-bit words when summed over the batch (the merge
    kernel has 8 waves, so two of them take a second source) and 2 per image"""
    S = _seg()
    names, h, w, bits = ['b10', 'rows', 'rings', 'b40', 'grid'], 264, 265, 8
    n = len(names)
    from cnn_autoencoder_amd import _lib
    assert _lib.lib().cae_seg_object_roc_workspace(n, h, w, bits) == n * 2 * (2 << bits) * 8  # two partials a plane
    target = np.stack([plane(k, h, w) for k in names])
    logits = _logits(n, 1, h, w, bits + h, target, target)
    _, _, boxes = OO.components(target)
    cover = OO.cover(boxes, h, w).astype(np.uint16)
    for per_image in (False, True):
        got = S.object_roc_histogram(dev(logits), dev(target), dev(cover), bits=bits, per_image=per_image)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), OO.object_histogram(logits, target, boxes, bits, per_image=per_image))


def test_sums_beyond_32_bits_are_exact():
    """cover 65535 on every pixel of a (264, 265) plane whose logits are one value: 69 960 x 65 535 > 2^32 in one bin"""
    S = _seg()
    n, h, w = 2, 264, 265
    total = h * w * 65535
    assert total > 2 ** 32
    logits = np.full((n, 1, h, w), 1.5, dtype=np.float32)
    target = np.ones((n, h, w), dtype=np.uint8)
    target[1] = 0
    cover = np.full((n, h, w), 65535, dtype=np.uint16)
    for bits in (8, 14):
        hist = S.object_roc_histogram(dev(logits), dev(target), dev(cover), bits=bits, per_image=True).cpu().numpy()
        b = int(RO.bin_of(np.float32(1.5), bits))
        want = np.zeros((n, 2, 1 << bits), dtype=np.int64)
        want[0, 1, b] = want[1, 0, b] = total
        assert np.array_equal(hist, want), (bits, hist[0, 1, b], hist[1, 0, b], total)
        assert np.array_equal(S.object_roc_histogram(dev(logits), dev(target), dev(cover), bits=bits).cpu().numpy(), want.sum(axis=0))
    counts = S.object_counts(dev(logits), dev(target), dev(cover), threshold=0.5).cpu().numpy()
    assert counts.tolist() == [[total, 0, 0, 0, total, total], [0, 0, total, 0, 0, 0]]
    # several classes: class 2 wins everywhere, the target names it on the first plane only
    logits3 = np.stack([np.full((n, h, w), v, dtype=np.float32) for v in (0.0, -1.0, 2.0)], axis=1)
    target3 = np.full((n, h, w), 2, dtype=np.uint8)
    target3[1] = 1
    counts = S.object_counts(dev(logits3), dev(target3), dev(cover), top_k=2).cpu().numpy()
    assert counts.tolist() == [[total, 0, 0, 0, total, total], [0, 0, total, total, total, 0]]


def test_a_caller_made_cover():
    """any uint16 weights are summed exactly: 65535 at three pixels of one bin, small weights elsewhere"""
    S = _seg()
    n, h, w = 2, 33, 65
    rng = np.random.default_rng(11)
    logits = _logits(n, 1, h, w, 3)
    target = plane('b40', h, w)[None].repeat(n, axis=0).copy()
    cover = rng.integers(0, 4, (n, h, w)).astype(np.uint16)
    spots = [(0, 5, 7), (0, 20, 64), (1, 32, 0)]
    for i, y, x in spots:
        logits[i, 0, y, x], target[i, y, x], cover[i, y, x] = -2.25, 3, 65535
    for bits in (8, 14):
        got = S.object_roc_histogram(dev(logits), dev(target), dev(cover), bits=bits).cpu().numpy()
        want = OO.weighted_histogram(logits, target, cover, bits)
        assert np.array_equal(got, want) and got[1, int(RO.bin_of(np.float32(-2.25), bits))] >= 3 * 65535
    got = S.object_counts(dev(logits), dev(target), dev(cover), threshold=0.0, threshold_on='logits').cpu().numpy()
    on, pos, cv = logits[:, 0] > 0, target > 0, cover.astype(np.int64)
    want = np.stack([(cv * (on & pos)).sum((1, 2)), (cv * (~on & ~pos)).sum((1, 2)), (cv * (on & ~pos)).sum((1, 2)),
                     (cv * (~on & pos)).sum((1, 2)), (cv * pos).sum((1, 2)), (cv * (on & pos)).sum((1, 2))], axis=1)
    assert np.array_equal(got, want) and want[0, 3] >= 2 * 65535


def test_python_surface_on_the_device():
    S = _seg()
    lab, cnt = S.components(torch.zeros((0, 4, 6), dtype=torch.uint8, device='cuda'))
    assert lab.shape == (0, 4, 6) and cnt.shape == (0,) and S.object_cover(lab).shape == (0, 4, 6)
    t = torch.zeros((2, 4, 6), dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError):
        S.components(t.cpu())
    with pytest.raises(ValueError):
        S.components(t, extent=[(4, 6)])
    with pytest.raises(ValueError):
        S.components(t, extent=np.array([(4.0, 6.0)] * 2))
    lab, _ = S.components(t)
    with pytest.raises(ValueError):
        S.object_cover(lab.cpu())
    lg = torch.zeros((2, 1, 4, 6), device='cuda')
    cv = S.object_cover(lab)
    with pytest.raises(ValueError):
        S.object_counts(lg, t, torch.zeros((2, 4, 6), dtype=torch.int32, device='cuda'))
    with pytest.raises(ValueError):
        S.object_counts(lg, t, cv[:1])
    with pytest.raises(ValueError):
        S.object_roc_histogram(torch.zeros((2, 3, 4, 6), device='cuda'), t, cv)
    with pytest.raises(ValueError):
        S.object_roc_histogram(lg, t, torch.zeros((2, 4, 6), dtype=torch.int32, device='cuda'))
    assert S.object_counts(lg[:0], t[:0], cv[:0]).shape == (0, 6)
    assert S.object_roc_histogram(lg[:0], t[:0], cv[:0], bits=8).shape == (2, 256)


# ------------------------------------------------------------------------------------------------------ driver
def _blobs(n, size, classes, seed=0):
    """label maps with a few objects: squares of values 1..classes on background"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, size, size), dtype=np.uint8)
    for i in range(n):
        for _ in range(6):
            y, x, s = rng.integers(0, size - 4), rng.integers(0, size - 4), rng.integers(1, 12)
            out[i, y:y + s, x:x + s] = rng.integers(1, max(classes, 2) + 1)
    return out


@pytest.mark.parametrize('classes', [1, 5])
def test_segment_batches_object_level(classes):
    """5 tiles in batches of 2 + 2 + 1: the object-level results equal the entry points called by hand on the batch's own
    logits, on both coders and with to_host; plain calls return the keys they returned before"""
    from cnn_autoencoder_amd import slide
    S = _seg()
    codec = TP._codec()
    _, seg = TP._head(True, classes)
    tiles, labels = TP._tiles(), _blobs(5, 64, classes)
    bufs = codec.encode_batch(tiles)
    extents = [np.array([(64, 64), (61, 59)]), np.array([(0, 64), (64, 1)]), np.array([(33, 64)])]
    bits = 11 if classes == 1 else None
    keys = {'cls', 'scores', 'counts', 'logits', 'n_objects', 'object_counts'} | ({'roc_hist', 'object_roc_hist'} if bits else set())
    sc = slide.SlideCoder(codec)
    want = []
    for r, lab, ext in zip(sc.segment_batches(TP._groups(bufs), 64, 64, seg, targets=TP._groups(labels), keep_logits=True,
                                              roc_bits=bits, extents=extents, object_level=True, threshold=0.6, top_k=2),
                           TP._groups(labels), extents):
        assert set(r) == keys
        tgt = torch.from_numpy(lab).cuda()
        lab_d, count = S.components(tgt, extent=ext, by_value=classes > 1)
        cover = S.object_cover(lab_d, extent=ext)
        assert torch.equal(r['n_objects'], count)
        assert torch.equal(r['object_counts'], S.object_counts(r['logits'], tgt, cover, threshold=0.6, top_k=2))
        if bits:
            assert r['object_roc_hist'].is_cuda
            assert torch.equal(r['object_roc_hist'], S.object_roc_histogram(r['logits'], tgt, cover, extent=ext, bits=bits))
        # and the restatement on the same logits
        _, count_o, boxes = OO.components(lab, extent=ext, by_value=classes > 1)
        assert np.array_equal(count.cpu().numpy(), count_o)
        t = np.float32(S.threshold_logit(0.6))
        assert np.array_equal(r['object_counts'].cpu().numpy(), OO.object_counts(r['logits'].cpu().numpy(), lab, boxes, t, 2))
        want.append({k: r[k].cpu().numpy().copy() for k in keys - {'cls', 'scores', 'logits', 'counts'}})
    assert len(want) == 3 and want[0]['n_objects'].sum() > 0 and not want[1]['n_objects'][0] and want[0]['object_counts'].sum() > 0
    for kw in (dict(coder='device'), dict()):
        sc2 = slide.SlideCoder(codec, **kw)
        to_host = 'coder' not in kw
        got = []
        for r in sc2.segment_batches(TP._groups(bufs), 64, 64, seg, targets=TP._groups(labels), roc_bits=bits, extents=extents,
                                     object_level=True, threshold=0.6, top_k=2, to_host=to_host):
            assert set(r) == keys
            if to_host:
                assert isinstance(r['n_objects'], np.ndarray) and isinstance(r['object_counts'], np.ndarray)
                assert not bits or r['object_roc_hist'].is_cuda
            got.append({k: r[k].cpu().numpy() if isinstance(r[k], torch.Tensor) else np.array(r[k]) for k in want[0]})
        assert len(got) == 3 and all(np.array_equal(a[k], b[k]) for a, b in zip(got, want) for k in a)
    # extents with object_level alone; plain calls carry the old keys
    alone = list(sc.segment_batches(TP._groups(bufs), 64, 64, seg, targets=TP._groups(labels), extents=extents,
                                    object_level=True, threshold=0.6, top_k=2))
    assert all(set(r) == {'cls', 'scores', 'counts', 'logits', 'n_objects', 'object_counts'} for r in alone)
    assert all(np.array_equal(r['object_counts'].cpu().numpy(), b['object_counts']) for r, b in zip(alone, want))
    plain = list(sc.segment_batches(TP._groups(bufs), 64, 64, seg, targets=TP._groups(labels)))
    assert all(set(r) == {'cls', 'scores', 'counts', 'logits'} for r in plain)
    with pytest.raises(ValueError, match='targets'):
        sc.segment_batches(TP._groups(bufs), 64, 64, seg, object_level=True)
    with pytest.raises(ValueError, match='roc_bits'):
        sc.segment_batches(TP._groups(bufs), 64, 64, seg, targets=TP._groups(labels), extents=extents)


@pytest.mark.parametrize('classes', [1, 3])
def test_segment_image_object_level(tmp_path, classes):
    """a 2 x 3-tile image whose size is no multiple of the patch: the object-level record is the restatement's over the
    real pixels of every tile; the curve is on disk; everything else is what the call without object_level gives"""
    import os
    from cnn_autoencoder_amd import synth, zarrio
    S = _seg()
    ckpt = TP._codec(tmp_path)
    _, seg = TP._head(True, classes)
    H, W, patch = 100, 170, 64
    img = np.ascontiguousarray(synth.histo_tile(192, 1)[:H, :W])
    store, out_store, plain_store = str(tmp_path / 'slide.zarr'), str(tmp_path / 'pred.zarr'), str(tmp_path / 'pred2.zarr')
    z = zarrio.compress_image('CAE', ckpt, img, store, patch_size=patch, batch_tiles=4)
    labels = np.concatenate([_blobs(1, H, classes, seed=4)[0], _blobs(1, H, classes, seed=5)[0, :, :W - H]], axis=1)
    labels[60:70, 120:140] = 1  # an object cut by tile borders: one object per tile
    zarrio.ZarrArray.create(store, 'labels/0', (H, W), (patch, patch), np.uint8, codec=zarrio.Zlib(1))[:] = labels
    bits = 14 if classes == 1 else None
    got = zarrio.segment_image(store, seg, out_store, target_group='labels/0', batch_tiles=4, roc_bits=bits, object_level=True)
    plain = zarrio.segment_image(store, seg, plain_store, target_group='labels/0', batch_tiles=4, roc_bits=bits)
    tiles = z.chunk_indices()
    logits = S.segment_compressed([z.read_chunk_bytes(i) for i in tiles], z.codec, seg).cpu().numpy()
    records, numbers, hist = [], 0, np.zeros((2, 1 << 14), dtype=np.int64)
    for (i, j, _), lg in zip(tiles, logits):
        ch, cw = min(patch, H - i * patch), min(patch, W - j * patch)
        lab = labels[i * patch:i * patch + ch, j * patch:j * patch + cw][None]
        _, count, boxes = OO.components(lab, by_value=classes > 1)
        records.append(OO.object_counts(lg[None, :, :ch, :cw], lab, boxes, np.float32(0), 5)[0])
        numbers += int(count[0])
        if bits:
            hist += OO.object_histogram(lg[None, :, :ch, :cw], lab, boxes, 14)
    obj = got['object_level']
    assert np.array_equal(obj['records'], np.stack(records)) and obj['n_objects'] == numbers and numbers > 4
    want = S.class_metrics(np.stack(records).sum(axis=0), multiclass=classes > 1)
    assert all(obj[k] == want[k] or (np.isnan(obj[k]) and np.isnan(want[k])) for k in want) and obj['p'] > 0
    if bits:
        roc = S.roc_from_histogram(hist)
        assert obj['auc'] == roc['auc'] and obj['auc_slack'] == roc['auc_slack'] and obj['roc']['p'] == roc['p'] > 0
        for name, key in (('fpr', 'fpr'), ('tpr', 'tpr'), ('thrsh', 'score_thresholds'), ('thrsh_logit', 'thresholds')):
            za = zarrio.ZarrArray.open(out_store, f'object_level/{name}')
            assert za.dtype == np.float32 and np.array_equal(za[:], roc[key].astype(np.float32), equal_nan=True), name
            a, b = (os.path.join(s, 'image_level', name, '0') for s in (out_store, plain_store))
            assert open(a, 'rb').read() == open(b, 'rb').read(), name
    else:
        assert 'auc' not in obj and not os.path.exists(os.path.join(out_store, 'object_level'))
    assert not os.path.exists(os.path.join(plain_store, 'object_level'))
    assert set(got) == set(plain) | {'object_level'}
    for k in plain:
        if k == 'roc':
            assert all(np.array_equal(got[k][m], plain[k][m], equal_nan=True) for m in plain[k])
        else:
            assert np.array_equal(got[k], plain[k], equal_nan=True), k
    assert np.array_equal(zarrio.ZarrArray.open(out_store, 'class/0/0')[:], zarrio.ZarrArray.open(plain_store, 'class/0/0')[:])
