"""The object-level restatement (tests/seg_objects_oracle.py) against hand-worked planes and against its own identities,
and the device-free part of the new ground: the ABI's refusals and workspace queries, the Python functions' argument
errors, the drivers' argument errors."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import seg_objects_oracle as OO
import seg_roc_oracle as RO
from test_seg_predict import oracle as predict_oracle


def _seg():
    from cnn_autoencoder_amd import segmenters
    return segmenters


def _plane(rows):
    return np.array([[int(c) for c in r] for r in rows], dtype=np.uint8)[None]


# ------------------------------------------------------------------------------------------- hand-worked planes
def test_a_corner_pixel_has_a_clipped_box():
    t = np.zeros((1, 4, 5), dtype=np.uint8)
    t[0, 0, 0] = 7
    labels, count, boxes = OO.components(t)
    assert count.tolist() == [1] and labels[0, 0, 0] == 1 and labels.sum() == 1
    assert boxes == [[(0, 2, 0, 2)]]
    cover = OO.cover(boxes, 4, 5)
    assert cover.sum() == 4 and (cover[0, :2, :2] == 1).all()
    t[0, 0, 0], t[0, 3, 4] = 0, 1  # the opposite corner: label 1 + 19
    labels, count, boxes = OO.components(t)
    assert labels[0, 3, 4] == 20 and boxes == [[(2, 4, 3, 5)]]
    # with an extent that cuts the widened box
    t[0, 3, 4], t[0, 1, 1] = 0, 1
    labels, count, boxes = OO.components(t, extent=[(2, 2)])
    assert labels[0, 1, 1] == 7 and boxes == [[(0, 2, 0, 2)]]


def test_two_diagonal_pixels_are_one_object():
    t = _plane(['0100', '1000', '0000'])
    labels, count, boxes = OO.components(t)
    assert count.tolist() == [1] and labels[0, 0, 1] == 2 and labels[0, 1, 0] == 2
    assert boxes == [[(0, 3, 0, 3)]]


def test_two_pixels_two_apart_overlap_in_the_pixel_between():
    t = _plane(['00000', '01010', '00000'])
    labels, count, boxes = OO.components(t)
    assert count.tolist() == [2] and labels[0, 1, 1] == 7 and labels[0, 1, 3] == 9
    cover = OO.cover(boxes, 3, 5)
    assert cover[0].tolist() == [[1, 1, 2, 1, 1]] * 3


def test_nested_rings():
    t = np.zeros((1, 9, 9), dtype=np.uint8)
    t[0, 0, :], t[0, 8, :], t[0, :, 0], t[0, :, 8] = 1, 1, 1, 1   # the outer ring
    t[0, 2, 2:7], t[0, 6, 2:7], t[0, 2:7, 2], t[0, 2:7, 6] = 1, 1, 1, 1  # a ring inside, one pixel of background between
    t[0, 4, 4] = 1  # and a pixel in the middle
    labels, count, boxes = OO.components(t)
    assert count.tolist() == [3]
    assert labels[0, 0, 0] == 1 and labels[0, 8, 8] == 1 and labels[0, 2, 2] == 21 and labels[0, 6, 6] == 21 and labels[0, 4, 4] == 41
    assert sorted(boxes[0]) == [(0, 9, 0, 9), (1, 8, 1, 8), (3, 6, 3, 6)]
    cover = OO.cover(boxes, 9, 9)
    assert cover[0, 0, 0] == 1 and cover[0, 1, 1] == 2 and cover[0, 4, 4] == 3 and cover[0, 2, 2] == 2 and cover[0, 3, 3] == 3


def test_by_value_keeps_touching_regions_of_different_values_apart():
    t = _plane(['1122', '1122', '0033'])
    labels, count, _ = OO.components(t, by_value=False)
    assert count.tolist() == [1] and (labels[0][t[0] > 0] == 1).all()
    labels, count, boxes = OO.components(t, by_value=True)
    assert count.tolist() == [3]
    assert labels[0].tolist() == [[1, 1, 3, 3], [1, 1, 3, 3], [0, 0, 11, 11]]
    assert sorted(boxes[0]) == [(0, 3, 0, 3), (0, 3, 1, 4), (1, 3, 1, 4)]
    # equal values that do not touch are objects of their own
    t = _plane(['505', '000', '505'])
    assert OO.components(t, by_value=True)[1].tolist() == [4]


def test_labels_give_back_their_boxes():
    rng = np.random.default_rng(0)
    t = (rng.random((3, 17, 23)) < 0.3).astype(np.uint8) * rng.integers(1, 4, (3, 17, 23)).astype(np.uint8)
    ext = [(17, 23), (9, 30), (20, 11)]
    for by_value in (False, True):
        labels, _, boxes = OO.components(t, extent=ext, by_value=by_value)
        again = OO.boxes_of_labels(labels, extent=ext)
        assert [sorted(b) for b in again] == [sorted(b) for b in boxes]


# ------------------------------------------------------------------------------------------------- identities
def test_the_cover_stays_below_three_times_the_short_side():
    rng = np.random.default_rng(1)
    worst = 0.0
    for k in range(200):
        h, w = (int(v) for v in rng.integers(1, 24, 2))
        density = rng.choice([0.05, 0.2, 0.4, 0.6])
        t = (rng.random((1, h, w)) < density).astype(np.uint8)
        if k % 4 == 0:  # the densest packing of objects: isolated pixels on the even grid
            t[:] = 0
            t[0, ::2, ::2] = 1
        _, count, boxes = OO.components(t, by_value=bool(k % 2))
        cover = OO.cover(boxes, h, w)
        assert cover.max() <= 3 * min(h, w), (h, w)
        worst = max(worst, cover.max() / (3 * min(h, w)))
        if k % 4 == 0:
            assert count[0] == -(-h // 2) * -(-w // 2)
    assert worst > 0.3  # the planes come near enough to the bound to say something


@pytest.mark.parametrize('c', [1, 3])
def test_the_concatenated_record_is_the_cover_weighted_record(c):
    rng = np.random.default_rng(2 + c)
    n, h, w = 2, 13, 19
    t = (rng.random((n, h, w)) < 0.25).astype(np.uint8) * rng.integers(1, 4, (n, h, w)).astype(np.uint8)
    logits = np.round(rng.standard_normal((n, c, h, w)) * 2).astype(np.float32)  # with ties
    ext = [(13, 19), (10, 12)]
    _, _, boxes = OO.components(t, extent=ext, by_value=c > 1)
    cover = OO.cover(boxes, h, w)
    assert cover.max() >= 2
    got = OO.object_counts(logits, t, boxes, np.float32(0.5), 2)
    # every pixel repeated cover times, and for one class summed by hand
    assert np.array_equal(got, OO.weighted_counts(logits.reshape(n, c, -1), t.reshape(n, -1), cover.reshape(n, -1), np.float32(0.5), 2))
    if c == 1:
        on, pos = logits[:, 0] > 0.5, t > 0
        by_hand = [(cover * (on & pos)).sum((1, 2)), (cover * (~on & ~pos)).sum((1, 2)), (cover * (on & ~pos)).sum((1, 2)),
                   (cover * (~on & pos)).sum((1, 2)), (cover * pos).sum((1, 2)), (cover * (on & pos)).sum((1, 2))]
        assert np.array_equal(got, np.stack(by_hand, axis=1))
    else:
        assert np.array_equal(got[:, 4], cover.sum((1, 2))) and np.array_equal(got[:, 2], got[:, 4] - got[:, 0])


def test_the_concatenated_histogram_is_the_cover_weighted_histogram():
    rng = np.random.default_rng(5)
    n, h, w = 2, 13, 19
    t = (rng.random((n, h, w)) < 0.25).astype(np.uint8)
    logits = (3 * rng.standard_normal((n, 1, h, w))).astype(np.float32)
    logits[0, 0, 0, :3] = [np.nan, np.inf, -np.inf]
    ext = [(13, 19), (10, 12)]
    _, _, boxes = OO.components(t, extent=ext)
    cover = OO.cover(boxes, h, w)
    for per_image in (False, True):
        got = OO.object_histogram(logits, t, boxes, 8, per_image=per_image)
        assert np.array_equal(got, OO.weighted_histogram(logits, t, cover, 8, per_image=per_image))
    assert OO.object_histogram(logits, t, boxes, 8).sum() == cover.sum()
    # weight 1 everywhere is the plain histogram
    ones = np.ones((n, h, w), dtype=np.int64)
    assert np.array_equal(OO.weighted_histogram(logits, t, ones, 11, extent=ext), RO.histogram(logits, t, 11, extent=ext))
    assert np.array_equal(OO.weighted_counts(logits.reshape(n, 1, -1), t.reshape(n, -1), ones.reshape(n, -1), np.float32(0), 5),
                          predict_oracle(logits.reshape(n, 1, -1), t.reshape(n, -1), np.float32(0), 5)[1])


def test_the_strict_record_is_the_plain_one_without_nan_and_the_contracts_with():
    """seg_objects_oracle.record against test_seg_predict's oracle on logits with ties and +-inf, and by hand on NaN"""
    rng = np.random.default_rng(8)
    for c in (1, 2, 3, 17):
        logits = np.round(2 * rng.standard_normal((3, c, 500))).astype(np.float32)
        logits[0, 0, :3], logits[1, c - 1, 3:6], logits[2, :, 6] = np.inf, -np.inf, np.inf
        target = rng.integers(0, c + 2, (3, 500)).astype(np.uint8)
        for top_k in (1, 2, 5):
            assert np.array_equal(OO.record(logits, target, np.float32(0), top_k), predict_oracle(logits, target, np.float32(0), top_k)[1])
    nan = np.nan
    # pixels:        all NaN   NaN at 0      NaN at 2      NaN at the target (1)   NaN everywhere but class 2
    lg = np.array([[nan,       nan,          1.0,          3.0,                    nan],
                   [nan,       5.0,          2.0,          nan,                    nan],
                   [nan,       7.0,          nan,          1.0,                    0.5]], dtype=np.float32)[None]
    # class by the strict compare: 0 (nothing beats a NaN at class 0), 0, 1, 0, 0
    # tp_top at top_k = 1 counts rank 0: no logit above the target's, none equal in a lower class; all false against a NaN
    for tgt, tp, top1 in (([0, 0, 1, 0, 0], 5, 5),   # every pixel's class named
                          ([1, 1, 1, 1, 1], 1, 4),   # pixel 1: 7 > 5, rank 1; the NaN targets of pixels 0, 3, 4 rank first
                          ([2, 2, 2, 2, 2], 0, 4),   # pixel 3: 3 > 1, rank 1; pixel 1: 7 is the largest; NaN targets rank first
                          ([3, 9, 255, 3, 3], 0, 0)):  # targets outside the classes are wrong
        got = OO.record(lg, np.array([tgt], dtype=np.uint8), np.float32(0), 1)[0]
        assert got.tolist() == [tp, 0, 5 - tp, 5 - tp, 5, top1], (tgt, got)


# ------------------------------------------------------------------------------------------------------ the ABI
NEW_SYMBOLS = ('cae_seg_components', 'cae_seg_components_workspace', 'cae_seg_object_cover', 'cae_seg_object_cover_workspace',
               'cae_seg_object_counts', 'cae_seg_object_counts_workspace', 'cae_seg_object_roc_hist',
               'cae_seg_object_roc_workspace')


def test_the_new_symbols_are_bound(built_lib):
    from cnn_autoencoder_amd import _lib
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is not None, name


def test_workspace_queries(built_lib):
    from cnn_autoencoder_amd import _lib
    L = _lib.lib()
    bad_planes = ((0, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, 0), (1, -3, 4), (1, 21846, 21846), (1, 30000, 70000),
                  (1, 3, 1 << 30))  # the last: 3 min(h, w) is fine, h w does not fit a label
    for n, h, w in bad_planes:
        assert L.cae_seg_components_workspace(n, h, w) == 0 and L.cae_seg_object_cover_workspace(n, h, w) == 0, (n, h, w)
    for n, h, w in ((1, 1, 1), (3, 7, 9), (3, 264, 265), (4, 1024, 1024), (32, 256, 256), (1, 21845, 21845), (1, 2, 1 << 29)):
        assert L.cae_seg_components_workspace(n, h, w) >= 8 * n and L.cae_seg_components_workspace(n, h, w) % 8 == 0
        assert L.cae_seg_object_cover_workspace(n, h, w) == 16 * n * h * w
    for n, c, hw in ((0, 1, 10), (1, 0, 10), (1, 257, 10), (1, 1, 0), (-2, 3, 10)):
        assert L.cae_seg_object_counts_workspace(n, c, hw) == 0
    for n, c, hw in ((1, 1, 1), (3, 17, 264 * 265), (4, 1, 1 << 20), (5000, 256, 64)):
        need = L.cae_seg_object_counts_workspace(n, c, hw)
        assert need >= 32 * n and need % 32 == 0
    for n, h, w, bits in ((1, 4, 4, 7), (1, 4, 4, 15), (1, 0, 4, 8), (1, 4, 0, 8), (0, 4, 4, 8), (-1, 4, 4, 8)):
        assert L.cae_seg_object_roc_workspace(n, h, w, bits) == 0
    for bits in (8, 11, 14):
        for n, h, w in ((1, 1, 1), (3, 264, 265), (4, 1024, 1024), (5000, 64, 64)):
            need = L.cae_seg_object_roc_workspace(n, h, w, bits)
            assert need >= n * 2 * (1 << bits) * 8 and need % (2 * (1 << bits) * 8) == 0
    assert L.cae_seg_object_roc_workspace(3, 264, 265, 14) == 3 * 2 * 2 * (1 << 14) * 8  # two spans of 65536 pixels an image


def test_abi_refuses_without_a_device(built_lib):
    """bad arguments are refused before anything touches a device; n == 0 is nothing to do"""
    from cnn_autoencoder_amd import _lib
    L = _lib.lib()
    p = 1 << 20  # a pointer-like value that is aligned to everything; never dereferenced: every call here is refused
    big = 1 << 40
    comp = lambda target=p, extent=None, n=1, h=4, w=4, labels=p, count=p, ws=p, nbytes=big: L.cae_seg_components(  # noqa: E731
        target, extent, n, h, w, 0, labels, count, ws, nbytes, None)
    assert comp(n=0) == 0 and comp(n=0, target=None, labels=None, count=None, ws=None, nbytes=0) == 0
    for kw in (dict(n=-1), dict(h=0), dict(w=0), dict(h=21846, w=21846), dict(h=3, w=1 << 30), dict(target=None),
               dict(labels=None), dict(count=None), dict(ws=None), dict(nbytes=0), dict(labels=p + 2), dict(count=p + 4),
               dict(ws=p + 4), dict(extent=p + 1)):
        assert comp(**kw) == -1, kw
    assert comp(n=0, h=0) == -1  # a bad shape is a bad shape with no images too
    cov = lambda labels=p, extent=None, n=1, h=4, w=4, cover=p, ws=p, nbytes=big: L.cae_seg_object_cover(  # noqa: E731
        labels, extent, n, h, w, cover, ws, nbytes, None)
    assert cov(n=0) == 0
    for kw in (dict(n=-1), dict(h=0), dict(w=-1), dict(h=21846, w=21846), dict(labels=None), dict(cover=None), dict(ws=None),
               dict(nbytes=16 * 16 - 1), dict(labels=p + 1), dict(cover=p + 1), dict(ws=p + 2), dict(extent=p + 2)):
        assert cov(**kw) == -1, kw
    cnt = lambda logits=p, target=p, cover=p, n=1, c=3, hw=16, k=5, counts=p, ws=p, nbytes=big: L.cae_seg_object_counts(  # noqa: E731
        logits, target, cover, n, c, hw, 0.0, k, counts, ws, nbytes, None)
    assert cnt(n=0) == 0
    for kw in (dict(n=-1), dict(c=0), dict(c=257), dict(hw=0), dict(k=0), dict(logits=None), dict(target=None), dict(cover=None),
               dict(counts=None), dict(ws=None), dict(nbytes=31), dict(logits=p + 2), dict(cover=p + 1), dict(counts=p + 4),
               dict(ws=p + 4)):
        assert cnt(**kw) == -1, kw
    roc = lambda logits=p, target=p, cover=p, extent=None, n=1, h=4, w=4, bits=8, hist=p, ws=p, nbytes=big: L.cae_seg_object_roc_hist(  # noqa: E731
        logits, target, cover, extent, n, h, w, bits, 0, hist, ws, nbytes, None)
    assert roc(n=0) == 0
    for kw in (dict(n=-1), dict(h=0), dict(w=0), dict(bits=7), dict(bits=15), dict(logits=None), dict(target=None),
               dict(cover=None), dict(hist=None), dict(ws=None), dict(nbytes=2 * 256 * 8 - 1), dict(logits=p + 1),
               dict(cover=p + 1), dict(hist=p + 4), dict(ws=p + 4), dict(extent=p + 2)):
        assert roc(**kw) == -1, kw


def test_the_new_kernels_use_no_scratch(built_lib):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import scratch_check
    table = {k: v for k, v in scratch_check.kernel_table(built_lib).items() if ('obj_' in k and '_kernel' in k) or 'seg_record_kernel' in k}
    # 4 of the labelling, 5 of the cover, 3 of the counts (2 + the shared record kernel), 1 of the histogram (its merge
    # kernel is shared too: tests/test_seg_roc_host.py)
    assert len(table) == 13, sorted(table)
    assert all(v == (0, 0) for v in table.values()), table


# -------------------------------------------------------------------------------------------------- Python surface
def test_python_functions_refuse_bad_arguments():
    S = _seg()
    u8 = torch.zeros((2, 4, 6), dtype=torch.uint8)
    with pytest.raises(ValueError, match='uint8'):
        S.components(u8.float())
    with pytest.raises(ValueError, match='uint8'):
        S.components(u8[0])
    with pytest.raises(ValueError, match='uint8'):
        S.components(u8.numpy())
    with pytest.raises(ValueError, match='too large'):
        S.components(torch.zeros((1, 21846, 21846), dtype=torch.uint8, device='meta'))
    with pytest.raises(ValueError, match='int32'):
        S.object_cover(u8)
    with pytest.raises(ValueError, match='int32'):
        S.object_cover(torch.zeros((4, 6), dtype=torch.int32))
    lg, cv = torch.zeros((2, 1, 4, 6)), torch.zeros((2, 4, 6), dtype=torch.uint16)
    with pytest.raises(ValueError, match='threshold'):
        S.object_counts(lg, u8, cv, threshold=1.0)
    with pytest.raises(ValueError, match='threshold_on'):
        S.object_counts(lg, u8, cv, threshold_on='probabilities')
    with pytest.raises(ValueError, match='top_k'):
        S.object_counts(lg, u8, cv, top_k=0)
    for bits in (7, 15, 8.5, True):
        with pytest.raises(ValueError, match='bits'):
            S.object_roc_histogram(lg, u8, cv, bits=bits)


def test_without_a_device_the_functions_say_so(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)  # (so on a machine that has one, too)
    S = _seg()
    u8 = torch.zeros((2, 4, 6), dtype=torch.uint8)
    lg, cv = torch.zeros((2, 1, 4, 6)), torch.zeros((2, 4, 6), dtype=torch.uint16)
    for call in (lambda: S.components(u8), lambda: S.object_cover(u8.to(torch.int32)), lambda: S.object_counts(lg, u8, cv),
                 lambda: S.object_roc_histogram(lg, u8, cv)):
        with pytest.raises(RuntimeError, match='no HIP device'):
            call()


def _bare_coder(channels=16, level=3):
    """a SlideCoder as far as segment_batches' argument checks look at it"""
    from cnn_autoencoder_amd import slide
    sc = object.__new__(slide.SlideCoder)
    sc.eb, sc.level = types.SimpleNamespace(channels=channels), level
    return sc


def test_segment_batches_argument_errors():
    sc = _bare_coder()
    seg = types.SimpleNamespace(training=False, _channels_bn=16, _num_classes=1)
    with pytest.raises(ValueError, match='object_level needs targets'):
        sc.segment_batches([[b'']], 64, 64, seg, object_level=True)
    with pytest.raises(ValueError, match='roc_bits'):  # as before: extents alone bound nothing
        sc.segment_batches([[b'']], 64, 64, seg, targets=[None], extents=[[(64, 64)]])
    with pytest.raises(ValueError, match='object_level'):
        sc.segment_batches([[b'']], 64, 64, seg, targets=[None], extents=[[(64, 64)]])
    with pytest.raises(ValueError, match='too large'):
        sc.segment_batches([[b'']], 21848, 21848, seg, targets=[None], object_level=True)
    with pytest.raises(ValueError, match='roc_bits needs targets'):
        sc.segment_batches([[b'']], 64, 64, seg, roc_bits=11, object_level=False)


def test_segment_image_needs_a_target_for_objects(tmp_path):
    from cnn_autoencoder_amd import zarrio
    with pytest.raises(ValueError, match='object_level needs a target_group'):
        zarrio.segment_image(str(tmp_path / 'none.zarr'), None, str(tmp_path / 'out.zarr'), object_level=True)
