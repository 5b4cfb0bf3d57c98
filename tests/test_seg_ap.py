"""cae_seg_score_hist on the GPU (csrc/cae_seg_hist.hip) and what is built on it: segmenters.score_histogram,
SlideCoder.segment_batches(ap_bits=...), zarrio.segment_image(ap_bits=...).

The oracle is the numpy restatement of the contract (tests/seg_ap_oracle.py) on the SAME scores, bit for bit: those that
cae_seg_predict wrote, copied back.  Histograms are integers and must be equal, entry for entry; the average precision is
ap_from_histogram of equal integers and must be equal too.  tests/test_seg_ap_host.py shows that these inputs tell a
linear bin and the positive rule target > 0 from the contract.
"""
import numpy as np
import pytest
import torch

import seg_ap_oracle as AO
import seg_roc_oracle as RO
import test_seg_predict as TP  # its tiny codec, head, tiles and batch split
from residue import poisoned_alloc  # noqa: F401  (the fixture)
from test_seg_roc import on_device

pytestmark = pytest.mark.gpu

BITS = [8, 14]


def _seg():
    from cnn_autoencoder_amd import segmenters
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return segmenters


_made = {}


def scores_of(shape, seed):
    """(scores (N,C,H,W) float32 as predict(scores=True) wrote them, target): made once per shape and only read"""
    if shape not in _made:
        S = _seg()
        logits, target = AO.draw(*shape, seed)
        sc = S.predict(torch.from_numpy(logits).cuda(), scores=True)['scores'].cpu().numpy()
        _made[shape] = (sc, target)
    return _made[shape]


def run(S, scores, target, bits, extent=None, per_image=False, per_class=False, offsets=(0, 0)):
    out = S.score_histogram(on_device(scores, offsets[0]), on_device(target, offsets[1]), extent=extent, bits=bits,
                            per_image=per_image, per_class=per_class)
    torch.cuda.synchronize()
    assert out.dtype == torch.int64 and out.is_cuda
    return out.cpu()


def judge(S, scores, target, bits, extent=None, offsets=(0, 0), what=''):
    """all four layouts against the restatement; -> the micro histogram"""
    want = torch.from_numpy(AO.score_hist(scores, target, bits, extent))  # (N, C, 2, B)
    n, c = want.shape[:2]
    both = run(S, scores, target, bits, extent, True, True, offsets)
    assert both.shape == want.shape and torch.equal(both, want), (what, torch.nonzero(both != want)[:5])
    per_class = run(S, scores, target, bits, extent, False, True, offsets)
    assert per_class.shape == (c, 2, 1 << bits) and torch.equal(per_class, want.sum(dim=0)), what
    per_image = run(S, scores, target, bits, extent, True, False, offsets)
    assert per_image.shape == (n, 2, 1 << bits) and torch.equal(per_image, want.sum(dim=1)), what
    micro = run(S, scores, target, bits, extent, False, False, offsets)
    assert micro.shape == (2, 1 << bits) and torch.equal(micro, want.sum(dim=(0, 1))), what
    assert torch.equal(per_class.sum(dim=0), micro)  # the class sum is the micro histogram
    return micro.numpy()


# ---------------------------------------------------------------------------------------------------- the histogram
@pytest.mark.parametrize('bits', BITS)
@pytest.mark.parametrize('shape', AO.SHAPES, ids=['x'.join(map(str, s)) for s in AO.SHAPES])
def test_histograms_equal_the_oracle(shape, bits):
    """the scores of predict(scores=True) on random logits; score offsets 0, 1, 3 put the planes at every alignment (with
    37 x 45 pixels every plane starts at another one anyway), target offset 1 takes the byte loads"""
    from cnn_autoencoder_amd import _lib
    S = _seg()
    n, c, h, w = shape
    scores, target = scores_of(shape, AO.SHAPES.index(shape))
    assert (target >= c).any() and scores.min() >= 0 and scores.max() <= 1
    blocks = _lib.lib().cae_seg_score_workspace(n, c, h, w, bits) // (n * c * (8 << bits))
    assert blocks == (2 if h * w > 8192 else 1)  # 96 x 100: several blocks per plane, and a merge of them
    extent = AO.EXTENTS.get(shape)
    for offsets in ((0, 0), (1, 1), (3, 0)):
        got = judge(S, scores, target, bits, extent, offsets, what=f'{shape} bits={bits} {offsets}')
    labelled = [(target[i, :r, :k] < c).sum() for i, (r, k) in enumerate(extent or [(h, w)] * n)]
    assert got[1].sum() == sum(labelled) and got[0].sum() == (c - 1) * sum(labelled)
    if extent is None:  # out of range values are clamped, no columns is no pixel
        judge(S, scores, target, bits, [((h + 7) * (-1) ** i, w + 100) for i in range(n)], what='clamped')
        judge(S, scores, target, bits, [(h - 3, w - 5)] * n, (1, 0), what='ragged')
        assert not judge(S, scores, target, bits, [(h, 0)] * n, what='no columns').any()


@pytest.mark.parametrize('bits', BITS)
def test_planted_values(bits):
    """hand-made planes that hold every edge with its neighbours, zeros, denormals, 0.5 +- 1 ulp, 1, NaN, negatives and
    values above 1: each in the bin the contract names, through the 16-byte path and through the single pixels"""
    S = _seg()
    planted = AO.special_values(bits)
    want_bins = AO.score_bin(planted, bits)
    for h, w in ((1, planted.size), (3, planted.size + 1)):
        x = np.resize(planted, (2, 2, h, w)).copy()
        x[:, 1] = x[:, 1, ::-1, ::-1]  # another value per class at a pixel
        target = (np.arange(2 * h * w).reshape(2, h, w) % 3).astype(np.uint8)  # label 2: unlabelled
        for offsets in ((0, 0), (1, 1)):
            got = judge(S, x, target, bits, None, offsets, what=f'planted {h}x{w}')
        assert got.sum() == 2 * (target < 2).sum()  # two classes per labelled pixel
    one = run(S, np.resize(planted, (1, 2, 1, planted.size)), np.zeros((1, 1, planted.size), np.uint8), bits, per_class=True)
    count = torch.from_numpy(np.bincount(want_bins, minlength=1 << bits))
    assert torch.equal(one[0, 1], count) and torch.equal(one[1, 0], count) and not one[0, 0].any() and not one[1, 1].any()


def test_all_pixels_at_one_value():
    """the contention case: every lane of every wave adds to one of two words"""
    S = _seg()
    target = AO.draw(1, 2, 96, 100, 5)[1]
    for v in (0.0, 1.0, 0.5, np.nan):
        x = np.full((1, 2, 96, 100), v, dtype=np.float32)
        got = judge(S, x, target, 14, None, (1, 0), what=f'one value {v}')
        b = int(AO.score_bin(np.float32(v), 14))
        assert got[1, b] == (target < 2).sum() == got[0, b] and got.sum() == 2 * (target < 2).sum()


# ---------------------------------------------------------------------------------- residue, streams, arguments
def test_results_do_not_depend_on_what_the_buffers_held(request):
    """histogram and workspace come from torch.empty: poisoned (0x7F bytes) and fenced they give the same integers, and no
    guard band is touched"""
    S = _seg()
    shape = (1, 2, 96, 100)
    scores, target = scores_of(shape, 1)
    ds, dt = on_device(scores, 1), on_device(target, 1)
    ext = [(93, 97)]
    want = S.score_histogram(ds, dt, extent=ext, bits=14, per_class=True).cpu()
    pa = request.getfixturevalue('poisoned_alloc')
    out = S.score_histogram(ds, dt, extent=ext, bits=14, per_class=True)
    assert pa.check(release=False) >= 2  # histogram, workspace
    assert torch.equal(out.cpu(), want)
    assert torch.equal(want, torch.from_numpy(AO.score_hist(scores, target, 14, ext)[0]))


def test_the_call_is_asynchronous_on_the_current_stream():
    """on a side stream behind the kernel that makes the scores there: no synchronisation in between, the scores'
    histogram all the same; and twice the same integers"""
    S = _seg()
    shape = (2, 3, 37, 45)
    scores, target = scores_of(shape, 0)
    logits = torch.from_numpy(AO.draw(*shape, 0)[0]).cuda()
    dt = torch.from_numpy(target).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        made = S.predict(logits, scores=True)['scores']
        a = S.score_histogram(made, dt, bits=14)
        b = S.score_histogram(made, dt, bits=14)
    side.synchronize()
    want = torch.from_numpy(AO.score_hist(scores, target, 14).sum(axis=(0, 1)))
    assert torch.equal(a.cpu(), want) and torch.equal(b.cpu(), want)


def test_views_that_are_not_contiguous():
    """as roc_histogram: read in place where contiguous, else through a contiguous copy -- the same integers"""
    S = _seg()
    shape = (3, 5, 16, 16)
    scores, target = scores_of(shape, 3)
    want = torch.from_numpy(AO.score_hist(scores, target, 8).sum(axis=(0, 1)))
    wide = torch.zeros(3, 5, 16, 32, device='cuda')
    wide[..., ::2] = torch.from_numpy(scores).cuda()
    tall = torch.zeros(3, 16, 16, 2, dtype=torch.uint8, device='cuda')
    tall[..., 0] = torch.from_numpy(target).cuda()
    assert not wide[..., ::2].is_contiguous() and not tall[..., 0].is_contiguous()
    assert torch.equal(S.score_histogram(wide[..., ::2], tall[..., 0], bits=8).cpu(), want)


def test_empty_batches_and_refusals():
    from cnn_autoencoder_amd import _lib
    S = _seg()
    sc = torch.full((2, 3, 4, 6), 0.25, device='cuda')
    tg = torch.zeros(2, 4, 6, dtype=torch.uint8, device='cuda')
    for per_image, per_class, shape in ((False, False, (2, 256)), (False, True, (3, 2, 256)), (True, False, (2, 2, 256)),
                                        (True, True, (2, 3, 2, 256))):
        assert S.score_histogram(sc, tg, bits=8, per_image=per_image, per_class=per_class).shape == shape
        empty = S.score_histogram(sc[:0], tg[:0], bits=8, per_image=per_image, per_class=per_class)
        assert empty.shape == ((0,) + shape[1:] if per_image else shape) and empty.dtype == torch.int64 and not empty.any()
    assert int(S.score_histogram(sc, tg, extent=torch.tensor([[4, 6], [1, 2]]), bits=8).sum()) == 3 * 26
    for bad in (dict(bits=7), dict(bits=15), dict(bits=8.5), dict(extent=[(1, 2)]), dict(extent=[(1.0, 2.0), (1.0, 2.0)])):
        with pytest.raises(ValueError):
            S.score_histogram(sc, tg, **bad)
    for scores, target in ((sc[:, :1], tg), (sc.double(), tg), (sc.view(2, 3, 24), tg), (sc, tg.float()), (sc, tg[:1]),
                           (sc.cpu(), tg), (torch.zeros(1, 256, 2, 2, device='cuda'), tg[:1, :2, :2])):
        with pytest.raises(ValueError):
            S.score_histogram(scores, target)
    # the ABI itself: refused before any launch, with a message
    L = _lib.lib()
    hist = torch.full((2, 256), -7, dtype=torch.int64, device='cuda')
    ws = torch.empty(L.cae_seg_score_workspace(2, 3, 4, 6, 8) // 8, dtype=torch.int64, device='cuda')
    assert ws.numel() * 8 == 2 * 3 * 1 * 2 * 256 * 4

    def call(scores=sc.data_ptr(), target=tg.data_ptr(), n=2, c=3, h=4, w=6, bits=8, out=hist.data_ptr(),
             work=ws.data_ptr(), size=ws.numel() * 8):
        return L.cae_seg_score_hist(scores, target, None, n, c, h, w, bits, 0, 0, out, work, size, _lib.stream_ptr())

    for kw, word in ((dict(scores=None), 'NULL'), (dict(target=None), 'NULL'), (dict(out=None), 'NULL'),
                     (dict(bits=7), 'bits'), (dict(bits=15), 'bits'), (dict(c=1), 'classes'), (dict(c=256), 'classes'),
                     (dict(n=0), 'shape'), (dict(h=0), 'shape'), (dict(w=-1), 'shape'), (dict(h=1 << 16, w=1 << 15), 'large'),
                     (dict(work=None), 'workspace'), (dict(size=ws.numel() * 8 - 1), 'workspace'),
                     (dict(work=ws.data_ptr() + 8, size=ws.numel() * 8 - 8, n=1), 'aligned'),
                     (dict(scores=sc.data_ptr() + 2), 'aligned')):
        with pytest.raises(ValueError, match=word):
            _lib.check(call(**kw))
    for args in ((0, 3, 4, 6, 8), (2, 1, 4, 6, 8), (2, 256, 4, 6, 8), (2, 3, 0, 6, 8), (2, 3, 4, 6, 15), (1, 2, 1 << 16, 1 << 15, 8)):
        assert L.cae_seg_score_workspace(*args) == 0
    torch.cuda.synchronize()
    assert (hist == -7).all()  # nothing was launched
    _lib.check(call())
    torch.cuda.synchronize()
    assert int(hist.sum()) == 3 * 48


# ------------------------------------------------------------------------------------------------------ drivers
def test_segment_batches_with_ap_bits():
    """5 tiles in batches of 2 + 2 + 1, a head of 5 classes: 'ap_hist' is the restated micro histogram of the batch's own
    scores inside its extents, asked for or not, on both coders and with to_host; a one-class head gets its logit
    histogram, the ROC one itself at equal bits; without ap_bits the results carry the keys they carried before"""
    from cnn_autoencoder_amd import slide
    codec = TP._codec()
    _, seg = TP._head(True, 5)
    tiles, labels = TP._tiles(), TP._labels(5, 64, 5)
    assert (labels >= 5).any()
    bufs = codec.encode_batch(tiles)
    extents = [np.array([(64, 64), (61, 59)]), np.array([(0, 64), (64, 1)]), np.array([(33, 64)])]
    sc = slide.SlideCoder(codec)
    want = []
    for r, lab, ext in zip(sc.segment_batches(TP._groups(bufs), 64, 64, seg, targets=TP._groups(labels), scores=True,
                                              ap_bits=11, extents=extents), TP._groups(labels), extents):
        assert set(r) == {'cls', 'scores', 'counts', 'logits', 'ap_hist'}
        assert r['ap_hist'].is_cuda and r['ap_hist'].dtype == torch.int64 and r['ap_hist'].shape == (2, 1 << 11)
        want.append(torch.from_numpy(AO.score_hist(r['scores'].cpu().numpy(), lab, 11, ext).sum(axis=(0, 1))))
        assert torch.equal(r['ap_hist'].cpu(), want[-1])
    assert len(want) == 3 and want[1][1].sum() == (labels[3, :, :1] < 5).sum()
    for kw in (dict(coder='device'), dict()):
        sc2 = slide.SlideCoder(codec, **kw)
        got = list(sc2.segment_batches(TP._groups(bufs), 64, 64, seg, targets=TP._groups(labels), ap_bits=11,
                                       extents=extents, to_host='coder' not in kw))
        assert all(r['scores'] is None and r['ap_hist'].is_cuda for r in got)  # made for the histogram, not handed out
        assert len(got) == 3 and all(torch.equal(r['ap_hist'].cpu(), b) for r, b in zip(got, want))
    plain = list(sc.segment_batches(TP._groups(bufs), 64, 64, seg, targets=TP._groups(labels)))
    assert all(set(r) == {'cls', 'scores', 'counts', 'logits'} for r in plain)
    # one class: the logit histogram at ap_bits
    _, seg1 = TP._head(True, 1)
    lab1 = TP._labels(5, 64, 1)
    for r, lab, ext in zip(sc.segment_batches(TP._groups(bufs), 64, 64, seg1, targets=TP._groups(lab1), keep_logits=True,
                                              roc_bits=11, ap_bits=9, extents=extents), TP._groups(lab1), extents):
        lg = r['logits'].cpu().numpy()
        assert np.array_equal(r['ap_hist'].cpu().numpy(), RO.histogram(lg, lab, 9, extent=ext))
        assert np.array_equal(r['roc_hist'].cpu().numpy(), RO.histogram(lg, lab, 11, extent=ext))
    for r in sc.segment_batches(TP._groups(bufs), 64, 64, seg1, targets=TP._groups(lab1), roc_bits=11, ap_bits=11):
        assert r['ap_hist'] is r['roc_hist'] and int(r['ap_hist'].sum()) == r['cls'].numel()
    with pytest.raises(ValueError, match='targets'):
        sc.segment_batches([bufs[:2]], 64, 64, seg, ap_bits=11)
    for bits in (7, 15, 9.5):
        with pytest.raises(ValueError, match='bits'):
            sc.segment_batches([bufs[:2]], 64, 64, seg, targets=[labels[:2]], ap_bits=bits)


def test_a_repeated_batch_counts_its_repeated_scores():
    """a batch that leaves the head's f16x3 range runs again on the fp32 head: its histogram is that of the scores it
    hands out, which are those of the repeated logits"""
    import struct
    from cnn_autoencoder_amd import slide
    from cnn_autoencoder_amd.codec import _module
    codec = TP._codec()
    _, seg = TP._head(True, 5)
    enc, eb = (_module(codec._model[k]) for k in ('encoder', 'fact_ent'))
    with torch.no_grad():
        sym = enc.forward_u8_symbols(torch.from_numpy(TP._tiles(2)).cuda(), eb)
    sym[1, 0, 0, 0] = 72000  # (the recipe of test_seg_predict: one symbol outside the f16 range)
    bufs = [struct.pack('>QQ', 64, 64) + p for p in eb.encode_symbols(sym.reshape(2, sym.size(1), -1).cpu().numpy())]
    labels = TP._labels(2, 64, 5)
    sc = slide.SlideCoder(codec)
    res = list(sc.segment_batches([bufs], 64, 64, seg, targets=[labels], scores=True, keep_logits=True, ap_bits=14))
    assert sc.timers['head_fp32_repeats'] == 1 and len(res) == 1
    assert torch.equal(res[0]['scores'], _seg().predict(res[0]['logits'], scores=True)['scores'])
    want = AO.score_hist(res[0]['scores'].cpu().numpy(), labels, 14).sum(axis=(0, 1))
    assert np.array_equal(res[0]['ap_hist'].cpu().numpy(), want)


def test_segment_image_with_ap_bits(tmp_path):
    """a 2 x 2-tile image with a ragged edge and a head of 5 classes: avg_prec and its bounds are ap_from_histogram of the
    restated histogram of the scores the same call wrote; the three curve arrays are in the store; a sparse store raises"""
    from cnn_autoencoder_amd import synth, zarrio
    S = _seg()
    ckpt = TP._codec(tmp_path)
    _, seg = TP._head(True, 5)
    H, W, patch = 100, 110, 64
    img = np.ascontiguousarray(synth.histo_tile(128, 1)[:H, :W])
    store, out_store = str(tmp_path / 'slide.zarr'), str(tmp_path / 'pred.zarr')
    zarrio.compress_image('CAE', ckpt, img, store, patch_size=patch, batch_tiles=4)
    labels = np.random.default_rng(5).integers(0, 6, (H, W)).astype(np.uint8)  # label 5: unlabelled
    zarrio.ZarrArray.create(store, 'labels/0', (H, W), (patch, patch), np.uint8, codec=zarrio.Zlib(1))[:] = labels
    got = zarrio.segment_image(store, seg, out_store, target_group='labels/0', batch_tiles=3, scores=True, ap_bits=14)
    scores = zarrio.ZarrArray.open(out_store, 'scores/0/0')[:]
    assert scores.shape == (5, H, W) and got['tiles'] == 4
    hist = AO.score_hist(scores[None], labels[None], 14).sum(axis=(0, 1))
    want = S.ap_from_histogram(hist)
    assert want['p'] == (labels < 5).sum() == got['pr']['p'] and got['pr']['n'] == 4 * want['p']
    for k in ('avg_prec', 'avg_prec_lo', 'avg_prec_hi'):
        assert got[k] == want[k] == got['pr'][k], k
    assert 0 < got['avg_prec_lo'] <= got['avg_prec'] <= got['avg_prec_hi'] <= 1
    oh = labels.reshape(-1)[:, None] == np.arange(5)[None]
    keep = labels.reshape(-1) < 5
    exact = AO.ap_sorted(oh[keep], scores.reshape(5, -1).T[keep])
    assert got['avg_prec_lo'] - 2.0 ** -49 <= exact <= got['avg_prec_hi'] + 2.0 ** -49
    for name, key in (('precision', 'precision'), ('recall', 'recall'), ('pr_thrsh', 'thresholds')):
        assert np.array_equal(got['pr'][key], want[key]), key
        za = zarrio.ZarrArray.open(out_store, f'image_level/{name}')
        assert za.dtype == np.float32 and za.shape == want[key].shape and za.chunks == want[key].shape
        assert za.meta['compressor'] == dict(id='zlib', level=9) and np.array_equal(za[:], want[key].astype(np.float32)), name
    # without scores=True the same numbers and no scores array; without ap_bits what there was before
    import os
    again = zarrio.segment_image(store, seg, str(tmp_path / 'pred2.zarr'), target_group='labels/0', batch_tiles=4,
                                 ap_bits=14, coder='device')
    assert all(again[k] == got[k] for k in ('avg_prec', 'avg_prec_lo', 'avg_prec_hi', 'tp', 'acc'))
    assert not os.path.exists(os.path.join(str(tmp_path / 'pred2.zarr'), 'scores'))
    plain = zarrio.segment_image(store, seg, str(tmp_path / 'pred3.zarr'), target_group='labels/0', batch_tiles=4)
    assert not {'avg_prec', 'avg_prec_lo', 'avg_prec_hi', 'pr'} & set(plain) and plain['tp'] == got['tp']
    assert not os.path.exists(os.path.join(str(tmp_path / 'pred3.zarr'), 'image_level'))
    with pytest.raises(ValueError, match='ap_bits'):
        zarrio.segment_image(store, seg, str(tmp_path / 'pred4.zarr'), batch_tiles=4, ap_bits=14)
    # a sparse store: a skipped chunk has no score
    blank = np.full((128, 128, 3), 240, dtype=np.uint8)
    blank[0:64, 0:64] = synth.histo_tile(64, 1)
    mask = np.zeros((4, 4), dtype=bool)
    mask[0:2, 0:2] = True
    sparse = str(tmp_path / 'sparse.zarr')
    zarrio.compress_image('CAE', ckpt, blank, sparse, patch_size=patch, batch_tiles=4, mask=mask, mask_scale=1 / 32)
    assert zarrio.ZarrArray.open(sparse, '0/0').is_sparse
    zarrio.ZarrArray.create(sparse, 'labels/0', (128, 128), (patch, patch), np.uint8, codec=zarrio.Zlib(1))[:] = np.ones(
        (128, 128), dtype=np.uint8)
    with pytest.raises(ValueError, match='sparse'):
        zarrio.segment_image(sparse, seg, str(tmp_path / 'pred5.zarr'), target_group='labels/0', ap_bits=14)


def test_segment_image_one_class_reads_the_logit_histogram(tmp_path):
    """a one-class head: avg_prec from the logit histogram, the ROC one's integers at equal bits"""
    from cnn_autoencoder_amd import synth, zarrio
    S = _seg()
    ckpt = TP._codec(tmp_path)
    _, seg = TP._head(True, 1)
    H, W, patch = 100, 110, 64
    img = np.ascontiguousarray(synth.histo_tile(128, 1)[:H, :W])
    store = str(tmp_path / 'slide.zarr')
    z = zarrio.compress_image('CAE', ckpt, img, store, patch_size=patch, batch_tiles=4)
    labels = np.random.default_rng(5).integers(0, 3, (H, W)).astype(np.uint8)
    zarrio.ZarrArray.create(store, 'labels/0', (H, W), (patch, patch), np.uint8, codec=zarrio.Zlib(1))[:] = labels
    got = zarrio.segment_image(store, seg, str(tmp_path / 'pred.zarr'), target_group='labels/0', roc_bits=14, ap_bits=14)
    tiles = z.chunk_indices()
    logits = S.segment_compressed([z.read_chunk_bytes(i) for i in tiles], z.codec, seg).cpu().numpy()
    mosaic = np.zeros((2 * patch, 2 * patch), dtype=np.float32)
    for (i, j, _), lg in zip(tiles, logits):
        mosaic[i * patch:(i + 1) * patch, j * patch:(j + 1) * patch] = lg[0]
    hist = RO.histogram(mosaic[None, None, :H, :W], labels[None], 14)
    want = S.ap_from_histogram(hist, key='logit')
    assert all(got[k] == want[k] for k in ('avg_prec', 'avg_prec_lo', 'avg_prec_hi')) and got['pr']['p'] == got['roc']['p']
    assert np.array_equal(got['pr']['thresholds'], want['thresholds']) and got['auc'] == S.roc_from_histogram(hist)['auc']
