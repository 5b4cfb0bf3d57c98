"""The host half of the slide ROC (segmenters.roc_bin_edges, roc_from_histogram) and the device-free part of the ABI,
against the numpy restatement of the contract (tests/seg_roc_oracle.py) and, where it is installed, sklearn."""
import os
import sys

import numpy as np
import pytest

import seg_roc_oracle as RO

BITS = [8, 11, 14]


def _seg():
    from cnn_autoencoder_amd import segmenters
    return segmenters


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.mark.parametrize('bits', BITS)
def test_bin_edges_are_the_restatements(bits):
    S = _seg()
    e, want = S.roc_bin_edges(bits), RO.edges(bits)
    assert e.dtype == np.float32 and e.shape == (1 << bits,)
    assert np.array_equal(np.isnan(e), np.isnan(want))
    ok = ~np.isnan(e)
    assert _same(e[ok], want[ok])
    # every edge opens its bin: bin(e_j) == j and the fp32 value below it lies in the bin below (the next non-empty one)
    j = np.flatnonzero(ok)
    assert np.array_equal(RO.bin_of(e[ok], bits), j)
    inner = ok & np.isfinite(e)  # (-inf has no predecessor)
    with np.errstate(over='ignore'):  # the most negative finite edge steps to -inf
        below = np.nextafter(e[inner], np.float32(-np.inf))
    assert np.array_equal(RO.bin_of(below, bits), np.flatnonzero(inner) - 1)
    assert (np.diff(e[ok]) > 0).all()
    # NaN-only bins: below -inf's and above +inf's
    assert np.isnan(e[:j[0]]).all() and np.isnan(e[j[-1] + 1:]).all() and j.size == j[-1] - j[0] + 1
    assert e[j[0]] == -np.inf and RO.bin_of(np.float32(np.inf), bits) == j[-1]


@pytest.mark.parametrize('bits', BITS)
def test_special_values_land_as_the_contract_says(bits):
    S = _seg()
    e = S.roc_bin_edges(bits)
    B = 1 << bits
    f = lambda v: int(RO.bin_of(np.float32(v), bits))
    assert f(0.0) == f(-0.0) == B // 2 and _same(e[B // 2], np.float32(0.0))  # one bin, opened by +0
    tiny = np.float32(1e-45)  # the smallest denormal
    assert f(tiny) == B // 2 and f(-tiny) == B // 2 - 1
    assert f(np.nan) == 0 and f(-np.nan) == 0
    assert f(-np.inf) == int(np.flatnonzero(~np.isnan(e))[0]) and f(np.inf) == int(np.flatnonzero(~np.isnan(e))[-1])
    assert f(-np.inf) <= f(-3e38) <= f(-1.0) < f(-tiny) < f(0.0) <= f(tiny) < f(1.0) <= f(3e38) <= f(np.inf)
    if bits > 8:
        assert f(np.nan) < f(-np.inf)  # NaN alone in bin 0


def test_bad_bits_are_refused():
    S = _seg()
    for bits in (7, 15, 0, -1, 8.5, True):
        with pytest.raises(ValueError):
            S.roc_bin_edges(bits)
    with pytest.raises(ValueError):
        S.roc_from_histogram(np.zeros((2, 100), dtype=np.int64))
    with pytest.raises(ValueError):
        S.roc_from_histogram(np.zeros((3, 256), dtype=np.int64))
    with pytest.raises(ValueError):
        S.roc_from_histogram(np.zeros((2, 256), dtype=np.float64))


def _draw(n, seed, sigma=3.0):
    rng = np.random.default_rng(seed)
    x = (sigma * rng.standard_normal(n)).astype(np.float32)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-x.astype(np.float64) + 1.0))).astype(np.uint8)  # informative labels
    return x, y


def _quantise(x, bits, S):
    return S.roc_bin_edges(bits)[RO.bin_of(x, bits)]


@pytest.mark.parametrize('bits', BITS)
def test_curve_and_auc_equal_sklearn_on_logits_that_sit_on_edges(bits):
    skm = pytest.importorskip('sklearn.metrics')
    S = _seg()
    x, y = _draw(5000, bits)
    x[:6] = [0.0, -0.0, 1e30, -1e30, 1e-40, -1e-40]  # (sklearn takes no infinite score)
    q = _quantise(x, bits, S)
    assert not np.isnan(q).any() and _same(_quantise(q, bits, S), q)
    roc = S.roc_from_histogram(RO.histogram(q.reshape(1, 1, 50, 100), y.reshape(1, 50, 100), bits))
    fpr, tpr, thr = skm.roc_curve(y, q.astype(np.float64), drop_intermediate=False)
    for k in ('fpr', 'tpr', 'thresholds', 'score_thresholds'):
        assert roc[k].dtype == np.float64 and roc[k].shape == fpr.shape, k
    assert np.array_equal(roc['fpr'], fpr) and np.array_equal(roc['tpr'], tpr)
    assert np.array_equal(roc['thresholds'], thr)
    assert roc['score_thresholds'][0] == np.inf
    with np.errstate(over='ignore'):
        assert np.array_equal(roc['score_thresholds'][1:], 1.0 / (1.0 + np.exp(-thr[1:])))
    # one division of exact integers against sklearn's float64 trapezoid sum over len(fpr) terms
    assert abs(roc['auc'] - skm.roc_auc_score(y, q.astype(np.float64))) <= len(fpr) * 2.0 ** -52
    assert roc['auc'] == RO.exact_auc(q, y)
    assert roc['p'] == int(y.sum()) and roc['n'] == int((1 - y).sum())


@pytest.mark.parametrize('bits', BITS)
def test_the_exact_auc_lies_inside_the_slack(bits):
    S = _seg()
    for seed, sigma in ((1, 3.0), (2, 0.01), (3, 1e-3)):  # narrow logits: many ties inside a bin, a wide slack
        x, y = _draw(4000, seed, sigma)
        roc = S.roc_from_histogram(RO.histogram(x.reshape(1, 1, 40, 100), y.reshape(1, 40, 100), bits))
        exact = RO.exact_auc(x, y)
        assert 0.0 <= roc['auc_slack'] <= 0.5
        # (one ulp of a number below 1 for the two divisions)
        assert roc['auc'] - roc['auc_slack'] - 2.0 ** -52 <= exact <= roc['auc'] + roc['auc_slack'] + 2.0 ** -52, \
            (bits, seed, roc['auc'], roc['auc_slack'], exact)
    x, y = _draw(4000, 4)
    q = _quantise(x, bits, S)
    roc = S.roc_from_histogram(RO.histogram(q.reshape(1, 1, 40, 100), y.reshape(1, 40, 100), bits))
    assert roc['auc'] == RO.exact_auc(q, y)  # on the edges the curve's area is the AUC itself


def test_hand_counted_histogram():
    S = _seg()
    h = np.zeros((2, 256), dtype=np.int64)
    h[0, [10, 20, 30]] = [3, 1, 2]  # negatives
    h[1, [20, 30, 40]] = [2, 1, 4]  # positives
    roc = S.roc_from_histogram(h)
    assert roc['p'] == 7 and roc['n'] == 6
    assert np.array_equal(roc['fpr'], np.array([0, 0, 2, 3, 6]) / 6) and np.array_equal(roc['tpr'], np.array([0, 4, 5, 7, 7]) / 7)
    e = S.roc_bin_edges(8)
    assert np.array_equal(roc['thresholds'][1:], e[[40, 30, 20, 10]].astype(np.float64))
    # pairs: the 4 at 40 beat all 6; the 1 at 30 beats 4 and ties 2; the 2 at 20 beat 3 and tie 1
    assert roc['auc'] == (2 * (4 * 6 + 1 * 4 + 2 * 3) + (1 * 2 + 2 * 1)) / (2 * 7 * 6)
    assert roc['auc_slack'] == (1 * 2 + 2 * 1) / (2 * 7 * 6)
    big = h * (1 << 40)  # a slide's counts: products beyond 64 bits
    assert S.roc_from_histogram(big)['auc'] == roc['auc']


def test_one_class_only_gives_nan():
    S = _seg()
    x, y = _draw(500, 5)
    for fill in (0, 1):
        roc = S.roc_from_histogram(RO.histogram(x.reshape(1, 1, 20, 25), np.full((1, 20, 25), fill, np.uint8), 11))
        assert np.isnan(roc['auc']) and np.isnan(roc['auc_slack'])
        assert roc['p'] == 500 * fill and roc['n'] == 500 * (1 - fill)
        assert np.isnan(roc['tpr' if fill == 0 else 'fpr']).all() and roc['fpr' if fill == 0 else 'tpr'][-1] == 1.0
    empty = S.roc_from_histogram(np.zeros((2, 1 << 11), dtype=np.int64))
    assert np.isnan(empty['auc']) and empty['fpr'].shape == (1,) and empty['thresholds'][0] == np.inf


def test_a_stack_of_histograms_equals_its_sum():
    import torch
    S = _seg()
    x, y = _draw(3 * 600, 6)
    per = RO.histogram(x.reshape(3, 1, 20, 30), y.reshape(3, 20, 30), 11, per_image=True)
    assert per.shape == (3, 2, 1 << 11)
    a, b = S.roc_from_histogram(per), S.roc_from_histogram(per.sum(axis=0))
    c = S.roc_from_histogram(torch.from_numpy(per))
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True) and np.array_equal(a[k], c[k], equal_nan=True), k


def test_the_restatement_counts_an_extent():
    x, y = _draw(2 * 42, 7)
    x, y = x.reshape(2, 1, 6, 7), y.reshape(2, 6, 7)
    h = RO.histogram(x, y, 8, extent=[(4, 2), (9, -1)], per_image=True)
    assert h[0].sum() == 8 and h[1].sum() == 0
    assert np.array_equal(h[0], RO.histogram(x[:1, :, :4, :2], y[:1, :4, :2], 8))


def test_abi_refuses_without_a_device(built_lib):
    from cnn_autoencoder_amd import _lib
    L = _lib.lib()
    for n, h, w, bits in ((1, 4, 4, 7), (1, 4, 4, 15), (1, 0, 4, 8), (1, 4, 0, 8), (0, 4, 4, 8), (-1, 4, 4, 8), (1, -3, 4, 14)):
        assert L.cae_seg_roc_workspace(n, h, w, bits) == 0 and L.cae_seg_roc_blocks(n, h, w, bits) == 0
    for bits in (8, 11, 14):
        for n, h, w in ((1, 1, 1), (3, 50, 100), (3, 264, 265), (4, 1024, 1024), (5000, 64, 64)):
            bx = L.cae_seg_roc_blocks(n, h, w, bits)
            assert bx >= 1 and L.cae_seg_roc_workspace(n, h, w, bits) == n * bx * 2 * (1 << bits) * 4
    assert L.cae_seg_roc_blocks(3, 264, 265, 14) >= 2
    # bad arguments are refused before anything touches a device
    assert L.cae_seg_roc_hist(None, None, None, 1, 4, 4, 7, 0, None, None, 0, None) == -1
    assert L.cae_seg_roc_hist(None, None, None, 1, 0, 4, 8, 0, None, None, 0, None) == -1
    assert L.cae_seg_roc_hist(None, None, None, 1, 4, 4, 8, 0, None, None, 0, None) == -1  # NULL pointers
    assert L.cae_seg_roc_hist(None, None, None, 0, 4, 4, 8, 0, None, None, 0, None) == 0   # n == 0: nothing to do


def test_the_new_kernels_use_no_scratch(built_lib):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import scratch_check
    table = {k: v for k, v in scratch_check.kernel_table(built_lib).items() if 'roc_hist_kernel' in k or 'seg_histsum_kernel' in k}
    assert len(table) == 3, sorted(table)  # the histogram; the merge of 32-bit and of 64-bit partials
    assert all(v == (0, 0) for v in table.values()), table


def test_reduce_histogram_is_the_identity_in_one_process():
    import torch
    from cnn_autoencoder_amd import slide
    h = torch.arange(2 * 256, dtype=torch.int64).view(2, 256)
    assert slide.reduce_histogram(h) is h
    with pytest.raises(ValueError, match='int64'):
        slide.reduce_histogram(h.to(torch.int32))
