"""cae_seg_roc_hist on the GPU (csrc/cae_seg_hist.hip) and what is built on it: segmenters.roc_histogram,
SlideCoder.segment_batches(roc_bits=...), zarrio.segment_image(roc_bits=...).

The oracle is the numpy restatement of the contract (tests/seg_roc_oracle.py) on the SAME logits.  Histograms are
integers and must be equal, entry for entry; curve and AUC are roc_from_histogram of equal integers and must be equal too.
"""
import numpy as np
import pytest
import torch

import seg_roc_oracle as RO
import test_seg_predict as TP  # its tiny codec, head, tiles and batch split
from residue import poisoned_alloc  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (7, 9), (16, 16), (50, 100), (264, 265)]  # the last: several blocks per image
BITS = [8, 11, 14]


def _seg():
    from cnn_autoencoder_amd import segmenters
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return segmenters


def on_device(arr, offset):
    """`arr` on the device as a view that starts `offset` elements into a larger buffer"""
    flat = torch.from_numpy(np.ascontiguousarray(arr)).reshape(-1)
    buf = torch.zeros(flat.numel() + offset + 8, dtype=flat.dtype, device='cuda')
    view = buf[offset:offset + flat.numel()]
    view.copy_(flat)
    return view.view(arr.shape)


def draw(n, h, w, seed, sigma=3.0):
    """logits (n,1,h,w) with a share of exact ties (halves) and a few special values, targets 0 (half of them), 1, 2, 255"""
    rng = np.random.default_rng(seed)
    x = (sigma * rng.standard_normal((n, 1, h, w))).astype(np.float32)
    x = np.where(rng.random(x.shape) < 0.3, np.round(x * 2) / 2, x).astype(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-41, -1e-41], dtype=np.float32)
    x = np.where(rng.random(x.shape) < 0.02, rng.choice(special, x.shape), x).astype(np.float32)
    target = rng.choice(np.array([0, 0, 0, 1, 2, 255], dtype=np.uint8), (n, h, w))
    return x, target


def run(S, logits, target, bits, extent=None, per_image=False, offsets=(0, 0)):
    out = S.roc_histogram(on_device(logits, offsets[0]), on_device(target, offsets[1]), extent=extent, bits=bits,
                          per_image=per_image)
    torch.cuda.synchronize()
    assert out.dtype == torch.int64 and out.is_cuda
    return out.cpu().numpy()


def judge(S, logits, target, bits, extent=None, offsets=(0, 0), what=''):
    want = RO.histogram(logits, target, bits, extent=extent, per_image=True)
    per = run(S, logits, target, bits, extent, True, offsets)
    assert per.shape == want.shape and np.array_equal(per, want), (what, np.argwhere(per != want)[:5])
    batch = run(S, logits, target, bits, extent, False, offsets)
    assert batch.shape == want.shape[1:] and np.array_equal(batch, want.sum(axis=0)), what
    return batch


def extents_of(n, h, w):
    """full, ragged, no rows, different per image, out of range (clamped)"""
    return [None, [(h - 3, w - 5)] * n, [(0, w)] * n, [(max(h - i, 0), max(w - 2 * i, 0)) for i in range(n)],
            [((h + 7) * (-1) ** i, w + 100) for i in range(n)], [(h, 0)] * n]


# ---------------------------------------------------------------------------------------------------- the histogram
@pytest.mark.parametrize('bits', BITS)
@pytest.mark.parametrize('n', [1, 3])
def test_histograms_equal_the_oracle(n, bits):
    """every shape at logit offsets 0, 1, 3 (plane starts off the 16-byte grid: one to three pixels in front of the first
    aligned one) and target offsets 0, 1 (byte loads), with every extent"""
    from cnn_autoencoder_amd import _lib
    S = _seg()
    assert _lib.lib().cae_seg_roc_blocks(n, 264, 265, bits) >= 2
    for h, w in SHAPES:
        logits, target = draw(n, h, w, 1000 * bits + 10 * h + n)
        for offsets in ((0, 0), (1, 1), (3, 0), (0, 1)):
            for extent in extents_of(n, h, w):
                judge(S, logits, target, bits, extent, offsets, what=f'n={n} bits={bits} {h}x{w} {offsets} {extent}')


@pytest.mark.parametrize('bits', BITS)
def test_planted_values(bits):
    """edges with their fp32 predecessors, both zeros, infinities, NaNs of both signs, denormals: each in the bin the
    contract names, through the 16-byte path and through the single pixels"""
    S = _seg()
    e = S.roc_bin_edges(bits)
    ok = np.flatnonzero(~np.isnan(e))
    js = [ok[0] + 1, ok[len(ok) // 3], (1 << bits) // 2 - 1, (1 << bits) // 2, (1 << bits) // 2 + 1, ok[-1]]
    with np.errstate(over='ignore'):
        planted = np.concatenate([e[js], np.nextafter(e[js], np.float32(-np.inf)),
                                  np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1e-45, -1e-45, 1e-39, -1e-39],
                                           dtype=np.float32)]).astype(np.float32)
    want_bins = RO.bin_of(planted, bits)
    assert np.array_equal(want_bins[:6], js) and np.array_equal(want_bins[6:12], np.array(js) - 1)
    assert want_bins[12] == want_bins[13] == (1 << bits) // 2 and want_bins[16] == want_bins[17] == 0
    for h, w in ((1, planted.size), (2, planted.size), (11, 2 * planted.size + 1)):
        x = np.resize(planted, (2, 1, h, w)).copy()
        target = (np.arange(2 * h * w).reshape(2, h, w) % 3).astype(np.uint8)
        for offsets in ((0, 0), (1, 1)):
            got = judge(S, x, target, bits, None, offsets, what=f'planted {h}x{w}')
        assert got.sum() == 2 * h * w
        if (h, w) == (1, planted.size):  # each value once per image and class of (index % 3 > 0)
            one = run(S, x[:1], np.zeros((1, h, w), np.uint8), bits)
            assert np.array_equal(one[0], np.bincount(want_bins, minlength=1 << bits)) and not one[1].any()


@pytest.mark.parametrize('bits', [8, 14])
def test_all_pixels_at_one_value(bits):
    """the contention case: every lane of every wave adds to one of two words"""
    S = _seg()
    for n, h, w, v in ((3, 264, 265, -4.25), (1, 50, 100, 0.0), (2, 7, 9, np.nan)):
        x = np.full((n, 1, h, w), v, dtype=np.float32)
        target = draw(n, h, w, 3)[1]
        got = judge(S, x, target, bits, None, (1, 0), what=f'one value {v}')
        b = int(RO.bin_of(np.float32(v), bits))
        assert got[1, b] == (target > 0).sum() and got[0, b] == (target == 0).sum() and got.sum() == n * h * w
        judge(S, x, target, bits, [(h - 3, w - 5)] * n, (0, 1), what=f'one value {v}, ragged')
    # 99 % of the pixels at one value, the others spread
    x, target = draw(2, 264, 265, 4)
    x = np.where(np.random.default_rng(5).random(x.shape) < 0.99, np.float32(-6.0), x).astype(np.float32)
    judge(S, x, target, bits, None, (0, 0), what='concentrated')


def test_targets_of_one_class_and_label_values():
    S = _seg()
    x, _ = draw(3, 50, 100, 6)
    for fill in (0, 1, 2, 255):
        got = judge(S, x, np.full((3, 50, 100), fill, dtype=np.uint8), 11, what=f'fill {fill}')
        assert got[1 if fill == 0 else 0].sum() == 0 and got.sum() == 3 * 50 * 100
    a = run(S, x, np.full((3, 50, 100), 1, dtype=np.uint8), 11)
    for fill in (2, 255):
        assert np.array_equal(run(S, x, np.full((3, 50, 100), fill, dtype=np.uint8), 11), a)  # positive is target > 0


# ---------------------------------------------------------------------------------------- residue, call order
@pytest.mark.parametrize('per_image', [False, True])
def test_results_do_not_depend_on_what_the_buffers_held(per_image, request):
    """histogram and workspace come from torch.empty: poisoned (0x7F bytes) and fenced they give the same integers, and no
    guard band is touched"""
    S = _seg()
    x, target = draw(3, 264, 265, 7)
    dl, dt = on_device(x, 1), on_device(target, 1)
    ext = [(264, 265), (100, 7), (261, 260)]
    want = S.roc_histogram(dl, dt, extent=ext, bits=14, per_image=per_image).cpu()
    pa = request.getfixturevalue('poisoned_alloc')
    out = S.roc_histogram(dl, dt, extent=ext, bits=14, per_image=per_image)
    assert pa.check(release=False) >= 2  # histogram, workspace
    assert torch.equal(out.cpu(), want)
    assert np.array_equal(want.numpy(), RO.histogram(x, target, 14, extent=ext, per_image=per_image))


def test_a_small_call_after_a_large_one_on_the_same_buffers():
    """the ABI itself, histogram and workspace of the large call handed to the small one as they are"""
    from cnn_autoencoder_amd import _lib
    _seg()
    L = _lib.lib()
    bits = 14
    big, small = draw(3, 264, 265, 8), draw(1, 7, 9, 9)
    ws = torch.empty(L.cae_seg_roc_workspace(3, 264, 265, bits) // 8, dtype=torch.int64, device='cuda')
    hist = torch.empty((3, 2, 1 << bits), dtype=torch.int64, device='cuda')
    assert L.cae_seg_roc_workspace(1, 7, 9, bits) < ws.numel() * 8

    def call(pair, n, h, w, per_image):
        dl, dt = on_device(pair[0], 0), on_device(pair[1], 0)
        _lib.check(L.cae_seg_roc_hist(dl.data_ptr(), dt.data_ptr(), None, n, h, w, bits, per_image, hist.data_ptr(),
                                      ws.data_ptr(), ws.numel() * 8, _lib.stream_ptr()))
        torch.cuda.synchronize()
        return hist.cpu().numpy().copy()

    first = call(big, 3, 264, 265, 1)
    assert np.array_equal(first, RO.histogram(*big, bits, per_image=True))
    got = call(small, 1, 7, 9, 0)
    assert np.array_equal(got[0], RO.histogram(*small, bits))
    assert np.array_equal(got[1:], first[1:])  # M = 1: the other entries are not this call's
    # a short workspace, a misaligned one and a missing target are refused before any launch
    dl, dt = on_device(big[0], 0), on_device(big[1], 0)
    with pytest.raises(ValueError, match='workspace'):
        _lib.check(L.cae_seg_roc_hist(dl.data_ptr(), dt.data_ptr(), None, 3, 264, 265, bits, 0, hist.data_ptr(),
                                      ws.data_ptr(), L.cae_seg_roc_workspace(3, 264, 265, bits) - 1, _lib.stream_ptr()))
    with pytest.raises(ValueError, match='aligned'):
        _lib.check(L.cae_seg_roc_hist(dl.data_ptr(), dt.data_ptr(), None, 1, 7, 9, bits, 0, hist.data_ptr(),
                                      ws.data_ptr() + 8, ws.numel() * 8 - 8, _lib.stream_ptr()))
    with pytest.raises(ValueError, match='NULL'):
        _lib.check(L.cae_seg_roc_hist(dl.data_ptr(), None, None, 1, 7, 9, bits, 0, hist.data_ptr(), ws.data_ptr(),
                                      ws.numel() * 8, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert np.array_equal(hist.cpu().numpy(), got)  # nothing was launched


def test_curve_points_are_the_confusion_counts_of_predict():
    """for several j: predict at the fp32 value below e_j gives tp = P_j and fp = N_j"""
    S = _seg()
    x, target = draw(2, 50, 100, 10)
    dl, dt = on_device(x, 1), on_device(target, 0)
    for bits in BITS:
        hist = S.roc_histogram(dl, dt, bits=bits).cpu().numpy()
        e = S.roc_bin_edges(bits)
        full = np.flatnonzero(hist.sum(axis=0))
        full = full[np.isfinite(e[full])]  # (a finite threshold for predict)
        for j in (full[0], full[len(full) // 4], full[len(full) // 2], full[-2], full[-1]):
            t = np.nextafter(e[j], np.float32(-np.inf))
            counts = S.predict(dl, dt, threshold=float(t), threshold_on='logits')['counts'].cpu().numpy().sum(axis=0)
            assert counts[0] == hist[1, j:].sum() and counts[2] == hist[0, j:].sum(), (bits, j)


def test_empty_batches_and_refusals():
    S = _seg()
    lg = torch.zeros(2, 1, 4, 6, device='cuda')
    tg = torch.zeros(2, 4, 6, dtype=torch.uint8, device='cuda')
    assert S.roc_histogram(lg, tg, bits=8).shape == (2, 256)
    assert S.roc_histogram(lg, tg, bits=8, per_image=True).shape == (2, 2, 256)
    empty = S.roc_histogram(lg[:0], tg[:0], bits=8)
    assert empty.shape == (2, 256) and empty.dtype == torch.int64 and not empty.any()
    assert S.roc_histogram(lg[:0], tg[:0], bits=8, per_image=True).shape == (0, 2, 256)
    assert int(S.roc_histogram(lg, tg, extent=torch.tensor([[4, 6], [1, 2]]), bits=8).sum()) == 26
    for bad in (dict(bits=7), dict(bits=15), dict(bits=8.5), dict(extent=[(1, 2)]), dict(extent=[(1.0, 2.0), (1.0, 2.0)])):
        with pytest.raises(ValueError):
            S.roc_histogram(lg, tg, **bad)
    with pytest.raises(ValueError, match='one-class'):
        S.roc_histogram(torch.zeros(2, 3, 4, 6, device='cuda'), tg)
    with pytest.raises(ValueError):
        S.roc_histogram(lg.double(), tg)
    with pytest.raises(ValueError):
        S.roc_histogram(lg.view(2, 1, 24), tg)
    with pytest.raises(ValueError):
        S.roc_histogram(lg, tg.float())
    with pytest.raises(ValueError):
        S.roc_histogram(lg, tg[:1])


# ------------------------------------------------------------------------------------------------------ driver
def test_segment_batches_with_roc_bits():
    """5 tiles in batches of 2 + 2 + 1: 'roc_hist' is the oracle's histogram of the batch's own logits inside its extents,
    on both coders and with to_host; without roc_bits the results carry the keys they carried before"""
    from cnn_autoencoder_amd import slide
    codec = TP._codec()
    _, seg = TP._head(True, 1)
    tiles, labels = TP._tiles(), TP._labels(5, 64, 1)
    bufs = codec.encode_batch(tiles)
    extents = [np.array([(64, 64), (61, 59)]), np.array([(0, 64), (64, 1)]), np.array([(33, 64)])]
    sc = slide.SlideCoder(codec)
    want = []
    for r, lab, ext in zip(sc.segment_batches(TP._groups(bufs), 64, 64, seg, targets=TP._groups(labels), keep_logits=True,
                                              roc_bits=11, extents=extents), TP._groups(labels), extents):
        assert set(r) == {'cls', 'scores', 'counts', 'logits', 'roc_hist'}
        assert r['roc_hist'].is_cuda and r['roc_hist'].dtype == torch.int64 and r['roc_hist'].shape == (2, 1 << 11)
        want.append(RO.histogram(r['logits'].cpu().numpy(), lab, 11, extent=ext))
        assert np.array_equal(r['roc_hist'].cpu().numpy(), want[-1])
    assert len(want) == 3 and want[1].sum() == 64 and want[2].sum() == 33 * 64
    for kw in (dict(coder='device'), dict()):
        sc2 = slide.SlideCoder(codec, **kw)
        got = [r['roc_hist'].cpu().numpy().copy()
               for r in sc2.segment_batches(TP._groups(bufs), 64, 64, seg, targets=TP._groups(labels), roc_bits=11,
                                            extents=extents, to_host='coder' not in kw)]
        assert len(got) == 3 and all(np.array_equal(a, b) for a, b in zip(got, want))
    # whole tiles without extents
    whole = [r['roc_hist'].cpu().numpy() for r in sc.segment_batches(TP._groups(bufs), 64, 64, seg,
                                                                     targets=TP._groups(labels), roc_bits=8)]
    assert [int(v.sum()) for v in whole] == [2 * 4096, 2 * 4096, 4096]
    plain = list(sc.segment_batches(TP._groups(bufs), 64, 64, seg, targets=TP._groups(labels)))
    assert all(set(r) == {'cls', 'scores', 'counts', 'logits'} for r in plain)


def test_segment_batches_roc_refusals():
    from cnn_autoencoder_amd import slide
    codec = TP._codec()
    _, seg = TP._head(True, 1)
    _, seg5 = TP._head(True, 5)
    sc = slide.SlideCoder(codec)
    bufs, labels = codec.encode_batch(TP._tiles(2)), TP._labels(2, 64, 1)
    with pytest.raises(ValueError, match='targets'):
        sc.segment_batches([bufs], 64, 64, seg, roc_bits=11)
    with pytest.raises(ValueError, match='one-class'):
        sc.segment_batches([bufs], 64, 64, seg5, targets=[labels], roc_bits=11)
    for bits in (7, 15, 9.5):
        with pytest.raises(ValueError, match='bits'):
            sc.segment_batches([bufs], 64, 64, seg, targets=[labels], roc_bits=bits)
    with pytest.raises(ValueError, match='roc_bits'):
        sc.segment_batches([bufs], 64, 64, seg, targets=[labels], extents=[[(64, 64)] * 2])
    assert torch.equal(slide.reduce_histogram(torch.arange(6).view(2, 3)), torch.arange(6).view(2, 3))  # one process


def test_segment_image_with_roc_bits(tmp_path):
    """a 2 x 3-tile image whose size is no multiple of the patch: auc, fpr and tpr are roc_from_histogram of the oracle's
    histogram over the image's real pixels; the four curve arrays are on disk"""
    from cnn_autoencoder_amd import synth, zarrio
    S = _seg()
    ckpt = TP._codec(tmp_path)
    _, seg = TP._head(True, 1)
    H, W, patch = 100, 170, 64
    img = np.ascontiguousarray(synth.histo_tile(192, 1)[:H, :W])
    store, out_store = str(tmp_path / 'slide.zarr'), str(tmp_path / 'pred.zarr')
    z = zarrio.compress_image('CAE', ckpt, img, store, patch_size=patch, batch_tiles=4)
    labels = np.random.default_rng(5).integers(0, 3, (H, W)).astype(np.uint8)
    zarrio.ZarrArray.create(store, 'labels/0', (H, W), (patch, patch), np.uint8, codec=zarrio.Zlib(1))[:] = labels
    got = zarrio.segment_image(store, seg, out_store, target_group='labels/0', batch_tiles=4, roc_bits=14)
    tiles = z.chunk_indices()
    logits = S.segment_compressed([z.read_chunk_bytes(i) for i in tiles], z.codec, seg).cpu().numpy()
    mosaic = np.zeros((2 * patch, 3 * patch), dtype=np.float32)
    for (i, j, _), lg in zip(tiles, logits):
        mosaic[i * patch:(i + 1) * patch, j * patch:(j + 1) * patch] = lg[0]
    want = S.roc_from_histogram(RO.histogram(mosaic[None, None, :H, :W], labels[None], 14))
    assert want['p'] + want['n'] == H * W and got['roc']['p'] == want['p'] and got['roc']['n'] == want['n']
    assert got['auc'] == want['auc'] and got['auc_slack'] == want['auc_slack'] and 0.0 <= got['auc'] <= 1.0
    exact = RO.exact_auc(mosaic[:H, :W], labels)
    assert abs(exact - got['auc']) <= got['auc_slack'] + 2.0 ** -52
    for k in ('fpr', 'tpr', 'thresholds', 'score_thresholds'):
        assert np.array_equal(got['roc'][k], want[k]), k
    for name, key in (('fpr', 'fpr'), ('tpr', 'tpr'), ('thrsh', 'score_thresholds'), ('thrsh_logit', 'thresholds')):
        za = zarrio.ZarrArray.open(out_store, f'image_level/{name}')
        assert za.dtype == np.float32 and za.shape == want[key].shape and za.meta['compressor'] == dict(id='zlib', level=9)
        assert np.array_equal(za[:], want[key].astype(np.float32)), name
    assert got['tiles'] == 6 and 'acc' in got  # beside the metrics of the threshold, which are what they were
    plain = zarrio.segment_image(store, seg, str(tmp_path / 'pred2.zarr'), target_group='labels/0', batch_tiles=4)
    assert 'auc' not in plain and 'roc' not in plain and all(plain[k] == got[k] for k in ('tp', 'tn', 'fp', 'fn', 'acc'))
    import os
    assert not os.path.exists(os.path.join(str(tmp_path / 'pred2.zarr'), 'image_level'))
    with pytest.raises(ValueError, match='roc_bits'):
        zarrio.segment_image(store, seg, str(tmp_path / 'pred3.zarr'), batch_tiles=4, roc_bits=14)
