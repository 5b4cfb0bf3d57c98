"""The host half of the slide's average precision (segmenters.score_bin_edges, ap_from_histogram and the argument checks
that need no device) against the numpy restatement (tests/seg_ap_oracle.py) and, where it is installed, sklearn.

Bounds.  ap_from_histogram divides its terms in Python integers and adds them with math.fsum; ap_sorted does the same.
Either is within 2^-51 of its exact value (lo, with its logarithm, within 2^-49), so equal quantities agree within
SUM = 2^-49 -- inside the 2^bits 2^-50 of a plain float64 summation over the bins -- and an inequality between exact
values holds between the computed ones within the same SUM.  sklearn sums in float64 over the distinct scores in order:
its result is compared within 2^-52 times the number of its terms.
"""
import numpy as np
import pytest

import seg_ap_oracle as AO

SUM = 2.0 ** -49
BITS = [8, 11, 14]


def _seg():
    from cnn_autoencoder_amd import segmenters
    return segmenters


def one_hot(target, c):
    """target (...,) -> (labelled pixels, c) booleans, and the mask of the labelled pixels"""
    t = np.asarray(target).reshape(-1)
    keep = t < c
    return t[keep][:, None] == np.arange(c)[None], keep


def pixels_by_class(scores, keep):
    """scores (N,C,H,W) -> (labelled pixels, C)"""
    c = scores.shape[1]
    return np.moveaxis(scores, 1, -1).reshape(-1, c)[keep]


def cases():
    """(name, scores (N,C,H,W) float32, target (N,H,W)): sharp and flat logits, C in 2..6, heavily tied scores"""
    out = []
    for seed, c in enumerate((2, 3, 4, 5, 6, 3)):
        logits, target = AO.draw(2, c, 24, 31, 100 + seed)
        s = AO.softmax32(logits)
        out.append((f'softmax C={c}', s, target))
        if seed % 2 == 0:
            out.append((f'tied C={c}', (np.round(s * 8) / 8).astype(np.float32), target))
    rng = np.random.default_rng(7)
    flat = AO.softmax32((0.01 * rng.standard_normal((1, 4, 20, 20))).astype(np.float32))
    out.append(('flat', flat, rng.integers(0, 4, (1, 20, 20)).astype(np.uint8)))
    sharp = AO.softmax32((40 * rng.standard_normal((1, 3, 20, 20))).astype(np.float32))
    out.append(('sharp', sharp, rng.integers(0, 3, (1, 20, 20)).astype(np.uint8)))
    return out


CASES = cases()


# ------------------------------------------------------------------------------------------------------ the bin
@pytest.mark.parametrize('bits', BITS)
def test_bin_edges_equal_the_search(bits):
    S = _seg()
    e, want = S.score_bin_edges(bits), AO.edges(bits)
    assert e.dtype == np.float32 and e.shape == (1 << bits,)
    assert np.array_equal(e, want, equal_nan=True)
    ok = np.flatnonzero(~np.isnan(e))
    assert e[0] == 0 and e[ok[-1]] == 1 and ok[-1] == (1 << bits) - 1 and (np.diff(e[ok]) > 0).all()
    # the smallest score of its bin: the edge is in bin j, its predecessor below
    assert np.array_equal(AO.score_bin(e[ok], bits), ok)
    assert (AO.score_bin(np.nextafter(e[ok[1:]], np.float32(-1)), bits) < ok[1:]).all()
    # bin(s) >= j exactly when s >= e_j, for every special value in [0, 1] and every reached bin
    v = AO.special_values(bits)
    v = v[(v >= 0) & (v <= 1)]
    b = AO.score_bin(v, bits)
    js = ok[:: max(1, ok.size // 97)]
    assert np.array_equal(b[:, None] >= js[None], v[:, None] >= e[js][None])


def test_the_bins_the_contract_names():
    x = np.array([0.25, np.nextafter(np.float32(0.5), np.float32(0)), 0.5, np.nextafter(np.float32(1), np.float32(0)), 1.0,
                  0.0, -0.0, np.nan, -1.0, 1e-45, 2.0, np.inf, -np.inf], dtype=np.float32)
    assert AO.score_bin(x, 14).tolist() == [8000, 8063, 8319, 9791, 16383, 0, 0, 0, 0, 0, 16383, 16383, 0]
    e = _seg().score_bin_edges(14)
    assert np.isnan(e[8064:8319]).all() and not np.isnan(e[[8063, 8319]]).any()


@pytest.mark.parametrize('bits', BITS)
def test_the_bin_is_monotone(bits):
    rng = np.random.default_rng(bits)
    s = np.concatenate([rng.random(50_000), rng.random(25_000) ** 8, 1 - rng.random(25_000) ** 8]).astype(np.float32)
    s = np.sort(np.concatenate([s, np.array([0, 0.5, 1], dtype=np.float32)]))
    b = AO.score_bin(s, bits)
    assert (np.diff(b) >= 0).all() and b.min() == 0 and b.max() == (1 << bits) - 1
    # and the bin of a score is that of the largest edge at or below it
    e = _seg().score_bin_edges(bits)
    ok = np.flatnonzero(~np.isnan(e))
    assert np.array_equal(ok[np.searchsorted(e[ok], s, side='right') - 1], b)


# ------------------------------------------------------------------------------------------- average precision
@pytest.mark.parametrize('bits', [8, 14])
@pytest.mark.parametrize('name,scores,target', CASES, ids=[c[0] for c in CASES])
def test_average_precision_and_its_bounds(name, scores, target, bits):
    S = _seg()
    c = scores.shape[1]
    hist = AO.score_hist(scores, target, bits)
    r = S.ap_from_histogram(hist.sum(axis=(0, 1)))
    oh, keep = one_hot(target, c)
    sc = pixels_by_class(scores, keep)
    assert r['p'] == oh.sum() and r['n'] == (~oh).sum()
    snapped = AO.ap_sorted(oh, AO.score_bin(sc, bits))
    assert abs(r['avg_prec'] - snapped) <= SUM <= (1 << bits) * 2.0 ** -50
    exact = AO.ap_sorted(oh, sc)
    assert r['avg_prec_lo'] - SUM <= exact <= r['avg_prec_hi'] + SUM, (r['avg_prec_lo'], exact, r['avg_prec_hi'])
    assert r['avg_prec_lo'] - SUM <= r['avg_prec'] <= r['avg_prec_hi'] + SUM
    # (M, 2, B) is summed; a torch tensor is taken too
    again = S.ap_from_histogram(hist.reshape(-1, 2, 1 << bits))
    assert all(again[k] == r[k] for k in ('avg_prec', 'avg_prec_lo', 'avg_prec_hi', 'p', 'n'))
    # per class: every class's own histogram against its own sorted scores
    for k in range(c):
        rk = S.ap_from_histogram(hist[:, k])
        assert abs(rk['avg_prec'] - AO.ap_sorted(oh[:, k], AO.score_bin(sc[:, k], bits))) <= SUM
        assert rk['avg_prec_lo'] - SUM <= AO.ap_sorted(oh[:, k], sc[:, k]) <= rk['avg_prec_hi'] + SUM
    # the curve: one point per non-empty bin, rising thresholds, the end point (1, 0)
    full = np.flatnonzero(hist.sum(axis=(0, 1, 2)))
    assert r['thresholds'].shape == (full.size,) and r['precision'].shape == r['recall'].shape == (full.size + 1,)
    assert np.array_equal(r['thresholds'], S.score_bin_edges(bits)[full].astype(np.float64))
    assert r['precision'][-1] == 1 and r['recall'][-1] == 0 and r['recall'][0] == 1 and (np.diff(r['recall']) <= 0).all()
    assert r['precision'][0] == r['p'] / (r['p'] + r['n'])
    steps = -np.diff(r['recall']) * r['precision'][:-1]  # sklearn's own sum over its curve
    assert abs(steps.sum() - r['avg_prec']) <= full.size * 2.0 ** -50


@pytest.mark.parametrize('bits', [8, 14])
@pytest.mark.parametrize('name,scores,target', CASES, ids=[c[0] for c in CASES])
def test_against_sklearn(name, scores, target, bits):
    metrics = pytest.importorskip('sklearn.metrics')
    S = _seg()
    c = scores.shape[1]
    hist = AO.score_hist(scores, target, bits)
    oh, keep = one_hot(target, c)
    sc = pixels_by_class(scores, keep)
    tol = oh.size * 2.0 ** -52
    r = S.ap_from_histogram(hist.sum(axis=(0, 1)))
    b = AO.score_bin(sc, bits).astype(np.float64)
    assert abs(r['avg_prec'] - metrics.average_precision_score(oh, b, average='micro')) <= tol
    micro = metrics.average_precision_score(oh, sc, average='micro')
    assert abs(micro - AO.ap_sorted(oh, sc)) <= tol
    assert r['avg_prec_lo'] - tol <= micro <= r['avg_prec_hi'] + tol
    per_class = metrics.average_precision_score(oh, sc, average=None)
    snapped = metrics.average_precision_score(oh, b, average=None)
    for k in range(c):
        rk = S.ap_from_histogram(hist[:, k])
        assert abs(rk['avg_prec'] - snapped[k]) <= tol
        assert rk['avg_prec_lo'] - tol <= per_class[k] <= rk['avg_prec_hi'] + tol
    pr, rc, th = metrics.precision_recall_curve(oh.reshape(-1), b.reshape(-1))
    if pr.size == r['precision'].size:  # (sklearn before 1.1 cut the curve where the recall reaches 1)
        assert np.allclose(pr, r['precision'], rtol=0, atol=2.0 ** -50) and np.allclose(rc, r['recall'], rtol=0, atol=2.0 ** -50)
        assert np.array_equal(th, np.flatnonzero(hist.sum(axis=(0, 1, 2))).astype(np.float64))


def test_separated_classes_give_a_point():
    """every positive above every negative: the interval is the point 1, at any bin width, ties inside bins or not"""
    S = _seg()
    rng = np.random.default_rng(0)
    target = rng.integers(0, 3, (2, 16, 16)).astype(np.uint8)
    oh = target[:, None] == np.arange(3)[None, :, None, None]
    scores = np.where(oh, 0.8 + 0.2 * rng.random(oh.shape), 0.1 * rng.random(oh.shape)).astype(np.float32)
    for bits in (8, 14):
        r = S.ap_from_histogram(AO.score_hist(scores, target, bits).sum(axis=(0, 1)))
        assert r['avg_prec'] == r['avg_prec_lo'] == r['avg_prec_hi'] == 1.0
    # no bin with both kinds, negatives above some positives: hi is the snapped value, lo at most that
    hist = np.zeros((2, 256), dtype=np.int64)
    hist[1, [200, 100]] = (5, 7)
    hist[0, [150, 50]] = (4, 9)
    r = S.ap_from_histogram(hist)
    assert r['avg_prec'] == r['avg_prec_hi'] == (5 * 5 / 5 + 7 * 12 / 16) / 12 and r['avg_prec_lo'] < r['avg_prec']
    # the lowest any order inside the bins can give (one positive per threshold) is not below lo
    assert r['avg_prec_lo'] <= (5 + sum((5 + i) / (9 + i) for i in range(1, 8))) / 12 + SUM


def test_no_positives_is_nan_and_no_negatives_is_one():
    S = _seg()
    hist = np.zeros((2, 256), dtype=np.int64)
    hist[0, [3, 77]] = (5, 6)
    r = S.ap_from_histogram(hist)
    assert all(np.isnan(r[k]) for k in ('avg_prec', 'avg_prec_lo', 'avg_prec_hi')) and r['p'] == 0 and r['n'] == 11
    assert np.isnan(r['precision']).all() and np.isnan(r['recall']).all() and r['thresholds'].shape == (2,)
    empty = S.ap_from_histogram(np.zeros((2, 256), dtype=np.int64))
    assert np.isnan(empty['avg_prec']) and empty['thresholds'].shape == (0,) and empty['precision'].shape == (1,)
    only = S.ap_from_histogram(hist[::-1])
    assert only['avg_prec'] == only['avg_prec_lo'] == only['avg_prec_hi'] == 1.0 and only['n'] == 0
    # counts beyond 2^32 per bin: Python integers, no overflow
    big = np.zeros((2, 256), dtype=np.int64)
    big[1, 200], big[0, 200], big[1, 10], big[0, 10] = 3 << 40, 1 << 40, 1 << 40, 5 << 40
    r = S.ap_from_histogram(big)
    assert abs(r['avg_prec'] - (3 * 0.75 + 1 * 0.4) / 4) <= SUM and r['avg_prec_lo'] <= r['avg_prec'] <= r['avg_prec_hi']


def test_logit_key_reads_a_roc_histogram():
    """a one-class case: the logit histogram of seg_roc_oracle, its average precision that of the sigmoid scores"""
    import seg_roc_oracle as RO
    S = _seg()
    rng = np.random.default_rng(3)
    target = (rng.random((2, 30, 41)) < 0.3).astype(np.uint8) * rng.integers(1, 4, (2, 30, 41)).astype(np.uint8)
    logits = (2 * rng.standard_normal((2, 1, 30, 41)) + 1.5 * (target[:, None] > 0)).astype(np.float32)
    for bits in (8, 14):
        hist = RO.histogram(logits, target, bits)
        r = S.ap_from_histogram(hist, key='logit')
        y = target.reshape(-1) > 0
        assert abs(r['avg_prec'] - AO.ap_sorted(y, RO.bin_of(logits, bits).reshape(-1))) <= SUM
        exact = AO.ap_sorted(y, logits.reshape(-1))
        assert r['avg_prec_lo'] - SUM <= exact <= r['avg_prec_hi'] + SUM
        sig = 1 / (1 + np.exp(-logits.astype(np.float64).reshape(-1)))  # monotone: the same order, the same value
        assert abs(AO.ap_sorted(y, sig) - exact) <= SUM
        full = np.flatnonzero(hist.sum(axis=0))
        assert np.array_equal(r['thresholds'], S.roc_bin_edges(bits)[full].astype(np.float64))
        assert r['p'] == y.sum() and r['n'] == (~y).sum()


# ------------------------------------------------------------------------------------------- arguments, no device
def test_argument_errors_without_a_device():
    import torch
    S = _seg()
    assert S.AP_BITS == 14 and S.AP_BITS_RANGE == (8, 14)
    for bad in (7, 15, 8.5, True):
        with pytest.raises(ValueError, match='bits'):
            S.score_bin_edges(bad)
        with pytest.raises(ValueError, match='bits'):
            S.score_histogram(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8), bits=bad)
    tg = torch.zeros(1, 4, 4, dtype=torch.uint8)
    for scores in (torch.zeros(1, 1, 4, 4), torch.zeros(1, 256, 4, 4), torch.zeros(1, 2, 16), torch.zeros(1, 2, 4, 4).double(),
                   np.zeros((1, 2, 4, 4), np.float32), torch.zeros(1, 2, 0, 4)):
        with pytest.raises(ValueError):
            S.score_histogram(scores, tg)
    with pytest.raises(ValueError, match='one-class'):
        S.score_histogram(torch.zeros(1, 1, 4, 4), tg)
    good = np.zeros((2, 256), dtype=np.int64)
    for hist in (good.astype(np.float64), good[:1], good[:, :255], np.zeros((2, 128), np.int64), good - 1,
                 np.zeros((2, 1 << 15), np.int64), np.zeros((2, 2, 2, 256), np.int64)):
        with pytest.raises(ValueError):
            S.ap_from_histogram(hist)
    with pytest.raises(ValueError, match='key'):
        S.ap_from_histogram(good, key='sigmoid')


def test_abi_refuses_without_a_device(built_lib):
    from cnn_autoencoder_amd import _lib
    L = _lib.lib()
    for args in ((1, 2, 4, 4, 7), (1, 2, 4, 4, 15), (1, 1, 4, 4, 8), (1, 256, 4, 4, 8), (1, 2, 0, 4, 8), (1, 2, 4, 0, 8),
                 (0, 2, 4, 4, 8), (-1, 2, 4, 4, 8), (1, 2, 1 << 16, 1 << 15, 8)):
        assert L.cae_seg_score_workspace(*args) == 0, args
        assert L.cae_seg_score_hist(None, None, None, *args, 0, 0, None, None, 0, None) == -1, args
    assert L.cae_seg_score_hist(None, None, None, 1, 2, 4, 4, 8, 0, 0, None, None, 0, None) == -1  # NULL pointers
    assert b'NULL' in L.cae_last_error()
    table = 2 * 4  # bytes of a partial per bin
    for bits in (8, 11, 14):
        cap = 256 if bits > 12 else 1024
        for n, c, h, w in ((1, 2, 1, 1), (1, 2, 96, 100), (2, 17, 8, 12), (4, 16, 1024, 1024), (40, 255, 64, 64)):
            blocks = min(-(-h * w // 8192), max(1, cap // (n * c)))
            assert L.cae_seg_score_workspace(n, c, h, w, bits) == n * c * blocks * (table << bits)
    assert L.cae_seg_score_workspace(4, 16, 1024, 1024, 14) == 32 << 20  # DESIGN's 32 MiB of partials


def test_the_new_kernel_uses_no_scratch(built_lib):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import scratch_check
    table = {k: v for k, v in scratch_check.kernel_table(built_lib).items() if 'score_hist_kernel' in k}
    assert len(table) == 1 and all(v == (0, 0) for v in table.values()), table


# ------------------------------------------------------------------------------------------------ the judge case
def test_the_gpu_inputs_tell_wrong_kernels_apart():
    """on every input of tests/test_seg_ap.py (the host's softmax of the same logits): a bin that is linear in the score
    and the positive rule target > 0 both give another histogram than the contract's, and so does counting unlabelled
    pixels or ignoring the extent where there is one"""
    for bits in (8, 14):
        for seed, shape in enumerate(AO.SHAPES):
            logits, target = AO.draw(*shape, seed)
            scores, extent = AO.softmax32(logits), AO.EXTENTS.get(shape)
            want = AO.score_hist(scores, target, bits, extent)
            assert want.sum() == sum(int((target[i, :r, :c] < shape[1]).sum()) * shape[1] for i, (r, c) in enumerate(
                extent or [(shape[2], shape[3])] * shape[0]))
            assert not np.array_equal(AO.score_hist(scores, target, bits, extent, bin_of=AO.linear_bin), want)
            assert not np.array_equal(AO.score_hist(scores, target, bits, extent, positive=lambda t, k: t > 0), want)
            relabelled = np.where(target >= shape[1], 0, target).astype(np.uint8)
            assert (target >= shape[1]).any() and not np.array_equal(AO.score_hist(scores, relabelled, bits, extent), want)
            if extent is not None:
                assert not np.array_equal(AO.score_hist(scores, target, bits), want)
            assert not np.array_equal(want[:, 0], want[:, 1])  # classes differ: a kernel that reads one plane is seen
