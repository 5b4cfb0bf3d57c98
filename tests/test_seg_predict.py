"""cae_seg_predict on the GPU (csrc/cae_seg_predict.hip) and what is built on it: segmenters.predict,
SlideCoder.segment_batches, zarrio.segment_image.

The oracle is numpy on the SAME logits.  Class maps and counts are integers and must be equal.  Scores:
max|gpu - f64| <= 4 E + 2^-24, E = the largest error of torch's own CPU float32 sigmoid / softmax against float64 on
those logits (the reference op's error, a margin of 4 for another exp, one fp32 rounding).  The driver's logits are held to
the end-to-end rule of tests/test_segmenter.py (segmenter_restatement.e2e_bound).
"""
import struct

import numpy as np
import pytest
import torch

import segmenter_restatement as SR
from residue import poisoned_alloc  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

HWS = [1, 3, 63, 64, 65, 257, 8 * 16 + 5, 2 * 1024 + 7, 5000]  # the last two: several blocks per image


def _seg():
    from cnn_autoencoder_amd import segmenters
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return segmenters


# ------------------------------------------------------------------------------------------------------- the oracle
def oracle(logits, target, t, top_k):
    """logits (N,C,HW) float32, target (N,HW) uint8 | None, t np.float32 -> (cls (N,HW) uint8, counts (N,6) int64 | None)"""
    n, c, hw = logits.shape
    if c == 1:
        cls = logits[:, 0] > np.float32(t)
        if target is None:
            return cls.astype(np.uint8), None
        pos = target > 0
        tp, tn = (cls & pos).sum(1), (~cls & ~pos).sum(1)
        fp, fn = (cls & ~pos).sum(1), (~cls & pos).sum(1)
        return cls.astype(np.uint8), np.stack([tp, tn, fp, fn, pos.sum(1), tp], axis=1).astype(np.int64)
    cls = logits.argmax(axis=1)  # the first of equal maxima
    if target is None:
        return cls.astype(np.uint8), None
    tgt = target.astype(np.int64)
    tp = (cls == tgt).sum(1)
    lt = np.take_along_axis(logits, np.minimum(tgt, c - 1)[:, None, :], axis=1)
    below = np.arange(c)[None, :, None] < tgt[:, None, :]
    rank = (logits > lt).sum(1) + ((logits == lt) & below).sum(1)
    top = ((tgt < c) & (rank < min(top_k, c))).sum(1)
    full = np.full(n, hw)
    return cls.astype(np.uint8), np.stack([tp, 0 * tp, full - tp, full - tp, full, top], axis=1).astype(np.int64)


def scores_f64(logits):
    x = logits.astype(np.float64)
    with np.errstate(over='ignore'):
        if x.shape[1] == 1:
            return 1.0 / (1.0 + np.exp(-x))
        e = np.exp(x - x.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)


def score_bound(logits):
    """4 E + 2^-24 with E of torch's CPU float32 op on these logits"""
    x = torch.from_numpy(logits)
    ref = torch.sigmoid(x) if x.shape[1] == 1 else torch.softmax(x, dim=1)
    return 4.0 * float(np.abs(ref.numpy().astype(np.float64) - scores_f64(logits)).max()) + 2.0 ** -24


def on_device(arr, offset):
    """`arr` on the device as a view that starts `offset` elements into a larger buffer"""
    flat = torch.from_numpy(np.ascontiguousarray(arr)).reshape(-1)
    buf = torch.zeros(flat.numel() + offset + 8, dtype=flat.dtype, device='cuda')
    view = buf[offset:offset + flat.numel()]
    view.copy_(flat)
    return view.view(arr.shape)


def draw(n, c, hw, seed, sigma=5.0):
    """logits with frequent exact ties (half of the pixels are rounded to halves), targets that include values >= c"""
    rng = np.random.default_rng(seed)
    x = (sigma * rng.standard_normal((n, c, hw))).astype(np.float32)
    coarse = rng.random((n, 1, hw)) < 0.5
    x = np.where(coarse, np.round(x / 4) * 4 if c > 1 else np.round(x * 2) / 2, x).astype(np.float32)
    target = rng.integers(0, max(c, 2) + 2, (n, hw)).astype(np.uint8)
    return x, target


def run(S, logits, target, offset, **kw):
    out = S.predict(on_device(logits, offset), None if target is None else on_device(target, 0), **kw)
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def judge(S, logits, target, offset, thr=0.5, on='scores', top_k=5, what=''):
    t = np.float32(S.threshold_logit(thr, on))
    got = run(S, logits, target, offset, threshold=thr, threshold_on=on, top_k=top_k, scores=True)
    cls, counts = oracle(logits, target, t, top_k)
    assert got['cls'].dtype == np.uint8 and got['cls'].shape == cls.shape
    assert np.array_equal(got['cls'], cls), what
    if target is None:
        assert got['counts'] is None
    else:
        assert got['counts'].dtype == np.int64 and np.array_equal(got['counts'], counts), (what, got['counts'], counts)
    err, bound = float(np.abs(got['scores'].astype(np.float64) - scores_f64(logits)).max()), score_bound(logits)
    assert np.isfinite(got['scores']).all() and err <= bound, (what, err, bound)
    plain = run(S, logits, target, offset, threshold=thr, threshold_on=on, top_k=top_k, scores=False)
    assert plain['scores'] is None and np.array_equal(plain['cls'], cls)  # the same decisions without the score stores
    assert target is None or np.array_equal(plain['counts'], counts)
    return got


# ------------------------------------------------------------------------------------- class map, counts, scores
@pytest.mark.parametrize('offset', [0, 1, 3])
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('c', [1, 2, 3, 7])
def test_class_map_counts_and_scores(c, n, offset):
    """3 classes are below top_k = 5 and 7 above; offset 1 / 3: plane starts off the 16-byte grid (scalar heads, byte
    stores of the class map, scalar score stores); HW not a multiple of four: every plane at another offset"""
    S = _seg()
    for hw in HWS:
        logits, target = draw(n, c, hw, 100 * c + hw)
        judge(S, logits, target, offset, what=f'c={c} n={n} hw={hw} offset={offset}')
    judge(S, *draw(n, c, 257, 7)[:1], None, offset, what='no target')


@pytest.mark.parametrize('c', [8, 12, 16, 17, 40, 256])
def test_register_bound_and_streamed_classes(c):
    """8 and 16 fill their register instance, 12 leaves rows of it unused, 17 is the first streamed count"""
    S = _seg()
    for hw, offset in ((65, 1), (1024 + 36, 0)):
        logits, target = draw(2, c, hw, c + hw, sigma=3.0)
        target[0, :7] = [0, c - 1, 255, 254, min(c, 255), 1, 2]
        judge(S, logits, target, offset, top_k=5, what=f'c={c} hw={hw}')


@pytest.mark.parametrize('on', ['scores', 'logits'])
@pytest.mark.parametrize('thr', [0.5, 0.9])
def test_planted_binary_values(thr, on):
    """the threshold itself and its two fp32 neighbours, both zeros, all-background and all-foreground targets"""
    S = _seg()
    t = np.float32(S.threshold_logit(thr, on))
    if on == 'scores':
        assert t == np.float32(np.log(np.float64(thr) / (1.0 - np.float64(thr))))
    else:
        assert t == np.float32(thr)
    planted = np.array([t, np.nextafter(t, np.float32(np.inf)), np.nextafter(t, np.float32(-np.inf)), 0.0, -0.0,
                        np.float32(thr), 1e-30, -1e-30], dtype=np.float32)
    hw = 64 + 5
    logits = np.tile(planted, 3 * hw // planted.size + 1)[:3 * hw].reshape(3, 1, hw).copy()
    logits[2, 0, 40:] = draw(1, 1, hw - 40, 3)[0][0, 0]
    for fill in (0, 1, None):
        target = draw(3, 1, hw, 5)[1] if fill is None else np.full((3, hw), 200 * fill, dtype=np.uint8)
        for offset in (0, 1):
            got = judge(S, logits, target, offset, thr=thr, on=on, what=f'thr={thr} on={on} fill={fill}')
            if fill == 0:
                assert not got['counts'][:, [0, 3, 4]].any()  # tp fn p
            if fill == 1:
                assert not got['counts'][:, [1, 2]].any() and (got['counts'][:, 4] == hw).all()
    # the compare is the fp32 one: on at the upper neighbour only; +0 and -0 are equal, so neither exceeds t = 0
    got = run(S, planted.reshape(1, 1, -1), None, 0, threshold=thr, threshold_on=on)
    assert got['cls'][0, :3].tolist() == [0, 1, 0]
    if thr == 0.5 and on == 'scores':
        assert t == 0.0 and got['cls'][0, 3:5].tolist() == [0, 0] and got['cls'][0, 6:].tolist() == [1, 0]


def test_planted_ties_and_targets_outside_the_classes():
    """equal maxima: the lowest index; the target's logit tied across the top-k boundary: the ties below the target's index
    rank first; targets >= C are wrong in tp and tp_top"""
    S = _seg()
    c, k = 7, 3
    rows = [
        ([1, 5, 5, 0, 5, -1, 2], 2),   # maxima at 1, 2, 4 -> class 1; target 2 has rank 1: inside
        ([1, 5, 5, 0, 5, -1, 2], 4),   # rank 2: the last place inside
        ([5, 5, 5, 0, 5, -1, 2], 4),   # rank 3: the first outside, only through the tie rule
        ([5, 5, 5, 0, 5, -1, 2], 0),   # rank 0, tp
        ([0, 0, 0, 0, 0, 0, 0], 2),    # all equal: class 0; rank = the index: 2 inside
        ([0, 0, 0, 0, 0, 0, 0], 3),    # 3 outside
        ([9, 8, 7, 6, 5, 4, 3], 7),    # target == C
        ([9, 8, 7, 6, 5, 4, 3], 255),
        ([-3, -2, -1, -1, -2, -3, -1], 6),  # maxima at 2, 3, 6 -> class 2; target 6 has rank 2: inside
        ([3, 3, 1, 1, 1, 1, 1], 6),    # rank 2 + 4 ties below it = 6: outside
    ]
    logits = np.array([r for r, _ in rows], dtype=np.float32).T[None].copy()  # (1, 7, 10)
    target = np.array([[t for _, t in rows]], dtype=np.uint8)
    for offset in (0, 1):
        got = judge(S, logits, target, offset, top_k=k, what='planted ties')
        assert got['cls'][0].tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 2, 0]
        assert got['counts'][0].tolist() == [1, 0, 9, 9, 10, 5]
    wide = np.tile(logits, (2, 1, 300))  # the same through the 16-byte path and two images
    judge(S, wide, np.tile(target, (2, 300)), 0, top_k=k, what='planted ties, wide')
    got = run(S, wide, np.tile(target, (2, 300)), 0, top_k=100)  # top_k above C: every target inside the classes counts
    assert got['counts'][:, 5].tolist() == [8 * 300, 8 * 300]


@pytest.mark.parametrize('c', [1, 2, 7, 20])
def test_extreme_logits_give_clean_scores(c):
    """+-80 and +-1e4: scores of 0 or 1, no NaN, softmax rows that sum to 1, all inside the bound"""
    S = _seg()
    rng = np.random.default_rng(c)
    hw = 260
    logits = rng.choice(np.array([80, -80, 1e4, -1e4, 0.5, -3], dtype=np.float32), size=(2, c, hw))
    logits[0, :, :4] = 1e4
    logits[1, :, :4] = -1e4
    target = draw(2, c, hw, 1)[1]
    for offset in (0, 1):
        got = judge(S, logits, target, offset, what=f'extreme c={c}')
        s = got['scores'].astype(np.float64)
        assert (s >= 0).all() and (s <= 1).all()
        if c == 1:
            big = np.abs(logits) >= 80
            assert float(np.abs(s[big] - np.round(s[big])).max()) < 1e-30  # 0 or 1 (e^-80 is 2e-35)
        else:
            assert float(np.abs(s.sum(axis=1) - 1.0).max()) <= score_bound(logits)


def test_nan_logits_stay_inside_the_classes():
    S = _seg()
    for c in (1, 3, 20):
        logits = draw(2, c, 133, c)[0]
        logits[0, :, ::3] = np.nan
        logits[1, 0, 1::2] = np.nan
        got = run(S, logits, draw(2, c, 133, 2)[1], 1, scores=True)
        assert (got['cls'] < max(c, 2)).all()
        if c == 1:
            assert not got['cls'][np.isnan(logits[:, 0])].any()  # the compare is false
        clean = ~np.isnan(logits).any(axis=1)
        want = oracle(logits, None, np.float32(0), 5)[0]
        assert np.array_equal(got['cls'][clean], want[clean])


# ---------------------------------------------------------------------------------------- residue, call order
@pytest.mark.parametrize('c', [1, 5, 20])
def test_results_do_not_depend_on_what_the_buffers_held(c, request):
    """class map, scores, counts and the workspace of partials come from torch.empty: poisoned (NaN / 0x7F) and fenced
    they give the same bits, and no guard band is touched"""
    S = _seg()
    logits, target = draw(3, c, 2 * 1024 + 7, 40 + c)
    dl, dt = on_device(logits, 1), on_device(target, 0)
    want = {k: v.cpu() for k, v in S.predict(dl, dt, scores=True).items()}
    pa = request.getfixturevalue('poisoned_alloc')
    out = S.predict(dl, dt, scores=True)
    assert pa.check(release=False) >= 4  # class map, scores, counts, workspace
    for k in want:
        assert torch.equal(out[k].cpu().view(torch.uint8), want[k].view(torch.uint8)), k
    assert np.array_equal(want['counts'].numpy(), oracle(logits, target, np.float32(0), 5)[1])


def test_a_small_call_after_a_large_one_counts_alone():
    S = _seg()
    for c in (1, 5):
        big = draw(3, c, 300 * 1024, 50 + c)
        small = draw(1, c, 65, 60 + c)
        first = run(S, *big, 0)
        got = run(S, *small, 0)
        assert np.array_equal(first['counts'], oracle(*big, np.float32(0), 5)[1])
        assert np.array_equal(got['counts'], oracle(*small, np.float32(0), 5)[1])
        assert np.array_equal(got['cls'], oracle(*small, np.float32(0), 5)[0])


def test_4d_logits_and_refusals():
    S = _seg()
    logits, target = draw(2, 5, 12 * 20, 9)
    out = S.predict(torch.from_numpy(logits).cuda().view(2, 5, 12, 20), torch.from_numpy(target).cuda().view(2, 12, 20))
    assert out['cls'].shape == (2, 12, 20) and out['scores'] is None and out['counts'].shape == (2, 6)
    assert np.array_equal(out['cls'].cpu().numpy().reshape(2, -1), oracle(logits, target, np.float32(0), 5)[0])
    with pytest.raises(ValueError):
        S.predict(torch.zeros(2, 5, 8, device='cuda', dtype=torch.float64))
    with pytest.raises(ValueError):
        S.predict(torch.zeros(2, 300, 8, device='cuda'))
    with pytest.raises(ValueError):
        S.predict(torch.zeros(2, 5, 8, device='cuda'), torch.zeros(2, 7, dtype=torch.uint8, device='cuda'))
    empty = S.predict(torch.zeros(0, 5, 8, device='cuda'), torch.zeros(0, 8, dtype=torch.uint8, device='cuda'))
    assert empty['cls'].shape == (0, 8) and empty['counts'].shape == (0, 6)


# ------------------------------------------------------------------------------------------------------ driver
CODEC_CFG = dict(channels_net=24, channels_bn=16, compression_level=3)


def _codec(tmp_path=None, seed=3):
    import cnn_autoencoder_amd as cae
    from cnn_autoencoder_amd import synth
    state = synth.synthetic_state(dict(synth.CANONICAL, **CODEC_CFG), seed=seed)
    if tmp_path is None:
        return cae.ConvolutionalAutoencoder(checkpoint=state)
    path = str(tmp_path / 'ckpt.pth')
    torch.save(state, path)
    return path


def _head(concat, classes, seed=0):
    S = _seg()
    cfg = dict(CODEC_CFG, seg_channels_net=6, seg_channels_bn=20, num_classes=classes, concat_bridges=concat,
               batch_norm=True)
    torch.manual_seed(seed)
    m = S.JNet(**cfg)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.GroupNorm):
                mod.weight.copy_(1.0 + 0.5 * torch.randn(mod.weight.shape, generator=g))
                mod.bias.copy_(0.3 * torch.randn(mod.bias.shape, generator=g))
    return cfg, m.cuda().eval()


def _tiles(n=5, size=64):
    from cnn_autoencoder_amd import synth
    return np.stack([synth.histo_tile(size, i) for i in range(n)])


def _labels(n, size, classes, seed=0):
    return np.random.default_rng(seed).integers(0, max(classes, 2) + 1, (n, size, size)).astype(np.uint8)


def _groups(items):
    return [items[0:2], items[2:4], items[4:5]]


def _numpy_of(res, labels, t=np.float32(0), top_k=5):
    lg = res['logits']
    lg = (lg.cpu().numpy() if isinstance(lg, torch.Tensor) else lg)
    n, c = lg.shape[:2]
    return oracle(lg.reshape(n, c, -1), None if labels is None else labels.reshape(n, -1), t, top_k)


def _host(res):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else (None if v is None else np.array(v)))
            for k, v in res.items()}


@pytest.mark.parametrize('classes', [1, 5])
@pytest.mark.parametrize('concat', [False, True])
def test_segment_batches(concat, classes):
    """5 tiles of 64 x 64 in batches of 2 + 2 + 1: class maps and counts are numpy's on the driver's own logits, in input
    order; those logits are inside the head's end-to-end bound, as segment_compressed's are; host and device coder agree;
    to_host equals the device result"""
    from cnn_autoencoder_amd import slide
    from cnn_autoencoder_amd.codec import _module
    S = _seg()
    codec = _codec()
    cfg, seg = _head(concat, classes)
    tiles, labels = _tiles(), _labels(5, 64, classes)
    bufs = codec.encode_batch(tiles)
    sc = slide.SlideCoder(codec)
    out = [_host(r) for r in sc.segment_batches(_groups(bufs), 64, 64, seg, targets=_groups(labels), keep_logits=True,
                                                scores=True)]
    assert [r['cls'].shape[0] for r in out] == [2, 2, 1]
    assert sc.timers['head_fp32_repeats'] == 0 and sc.timers['head'] > 0
    for r, lab in zip(out, _groups(labels)):
        cls, counts = _numpy_of(r, lab)
        assert r['cls'].shape == lab.shape and np.array_equal(r['cls'].reshape(len(lab), -1), cls)
        assert np.array_equal(r['counts'], counts)
        lg = r['logits'].reshape(len(lab), classes, -1)
        assert float(np.abs(r['scores'].reshape(lg.shape).astype(np.float64) - scores_f64(lg)).max()) <= score_bound(lg)
    # the logits: the order is the input order, and the values are the head's
    logits = torch.from_numpy(np.concatenate([r['logits'] for r in out]))
    direct = S.segment_compressed(bufs, codec, seg).cpu()
    eb, dec = _module(codec._model['fact_ent']), _module(codec._model['decoder'])
    with torch.no_grad():
        y_q = eb.decompress([b[16:] for b in bufs], (8, 8))
        _, brg = dec(y_q)
    sd = {k: v.detach().cpu() for k, v in seg.state_dict().items()}
    brg = [b.cpu() for b in brg] if concat else None
    f64, _ = SR.jnet(sd, cfg, y_q.cpu(), brg, torch.float64)
    f32, _ = SR.jnet(sd, cfg, y_q.cpu(), brg, torch.float32)
    bound = SR.e2e_bound(f32, f64)
    assert logits.shape == direct.shape == (5, classes, 64, 64)
    assert float((logits.double() - f64).abs().max()) <= bound and float((direct.double() - f64).abs().max()) <= bound
    # the device coder, and the pinned ring of to_host
    dev = [_host(r) for r in slide.SlideCoder(codec, coder='device').segment_batches(_groups(bufs), 64, 64, seg,
                                                                                     targets=_groups(labels))]
    sc2 = slide.SlideCoder(codec)
    host = []
    for r in sc2.segment_batches(_groups(bufs), 64, 64, seg, targets=_groups(labels), to_host=True, scores=True,
                                 keep_logits=True):
        assert all(v is None or isinstance(v, np.ndarray) for v in r.values())
        host.append({k: None if v is None else v.copy() for k, v in r.items()})
    for a, b, c_ in zip(out, dev, host):
        assert np.array_equal(a['cls'], b['cls']) and np.array_equal(a['counts'], b['counts'])
        assert b['scores'] is None and b['logits'] is None
        for k in ('cls', 'counts', 'scores', 'logits'):
            assert np.array_equal(a[k], c_[k]), k
    # without targets: no counts
    plain = list(sc.segment_batches(_groups(bufs), 64, 64, seg))
    assert all(r['counts'] is None and r['scores'] is None and r['logits'] is None for r in plain)
    assert np.array_equal(np.concatenate([r['cls'].cpu().numpy() for r in plain]), np.concatenate([r['cls'] for r in out]))


def test_segment_batches_refusals():
    from cnn_autoencoder_amd import slide
    codec = _codec()
    _, seg = _head(True, 1)
    sc = slide.SlideCoder(codec)
    bufs = codec.encode_batch(_tiles(2)) + codec.encode_batch(_tiles(1, 32))
    with pytest.raises(ValueError, match='one tile size'):
        list(sc.segment_batches([bufs[:2], bufs[2:]], 64, 64, seg))
    seg.train()
    with pytest.raises(ValueError, match='eval'):
        sc.segment_batches([bufs[:2]], 64, 64, seg)
    seg.eval()
    other = _seg().JNet(**dict(CODEC_CFG, channels_bn=12, seg_channels_net=6, seg_channels_bn=20)).cuda().eval()
    with pytest.raises(ValueError, match='channels'):
        sc.segment_batches([bufs[:2]], 64, 64, other)
    with pytest.raises(ValueError, match='threshold'):
        sc.segment_batches([bufs[:2]], 64, 64, seg, threshold=1.0)


def test_a_batch_outside_the_f16_range_is_repeated_in_fp32():
    """one symbol of 72 000 in tile 2: the head's call of batch 1 leaves the f16x3 range; the generator completes, that
    batch comes from the head's fp32 torch ops, the timers count one repeat, batches 0 and 2 are what they are without it"""
    from cnn_autoencoder_amd import slide
    from cnn_autoencoder_amd.codec import _module
    codec = _codec()
    _, seg = _head(True, 5)
    enc, eb, dec = (_module(codec._model[k]) for k in ('encoder', 'fact_ent', 'decoder'))
    with torch.no_grad():
        sym = enc.forward_u8_symbols(torch.from_numpy(_tiles()).cuda(), eb)
    sym[2, 0, 0, 0] = 72000
    head = struct.pack('>QQ', 64, 64)
    bufs = [head + p for p in eb.encode_symbols(sym.reshape(5, sym.size(1), -1).cpu().numpy())]
    sc = slide.SlideCoder(codec)
    out = [_host(r) for r in sc.segment_batches(_groups(bufs), 64, 64, seg, keep_logits=True)]
    assert len(out) == 3 and sc.timers['head_fp32_repeats'] == 1
    with torch.no_grad():
        y_q = eb.dequantize_symbols(sym[2:4])
        assert float(y_q.abs().max()) > 65504.0
        _, brg = dec(y_q)
        with pytest.raises(FloatingPointError):
            seg(y_q, fx_brg=brg)
        seg.force_torch = True
        want = seg(y_q, fx_brg=brg)[0].cpu().numpy()
        seg.force_torch = False
    assert np.isfinite(want).all()
    assert np.array_equal(out[1]['cls'].reshape(2, -1), oracle(want.reshape(2, 5, -1), None, np.float32(0), 5)[0])
    assert np.array_equal(out[1]['cls'].reshape(2, -1), _numpy_of(out[1], None)[0])
    rest = [_host(r) for r in sc.segment_batches([bufs[0:2], bufs[4:5]], 64, 64, seg, keep_logits=True)]
    assert sc.timers['head_fp32_repeats'] == 0
    for a, b in zip((out[0], out[2]), rest):
        assert np.array_equal(a['cls'], b['cls']) and np.array_equal(a['logits'], b['logits'])


@pytest.mark.parametrize('classes', [1, 5])
def test_segment_image(tmp_path, classes):
    """a 2 x 3-tile image whose size is no multiple of the patch: class/0/0 (and scores/0/0) have the image's shape, every
    chunk is the tile's result cropped, the slide metrics are class_metrics of numpy's counts over the image's pixels"""
    from cnn_autoencoder_amd import synth, zarrio
    S = _seg()
    ckpt = _codec(tmp_path)
    _, seg = _head(True, classes)
    H, W, patch = 100, 170, 64
    img = np.ascontiguousarray(synth.histo_tile(192, 1)[:H, :W])
    store, out_store = str(tmp_path / 'slide.zarr'), str(tmp_path / 'pred.zarr')
    z = zarrio.compress_image('CAE', ckpt, img, store, patch_size=patch, batch_tiles=4)
    labels = np.random.default_rng(5).integers(0, max(classes, 2) + 1, (H, W)).astype(np.uint8)
    zarrio.ZarrArray.create(store, 'labels/0', (H, W), (patch, patch), np.uint8, codec=zarrio.Zlib(1))[:] = labels
    thr = 0.6
    got = zarrio.segment_image(store, seg, out_store, target_group='labels/0', batch_tiles=4, threshold=thr, scores=True)
    # per tile, by the unpipelined path
    tiles = z.chunk_indices()
    assert len(tiles) == 6 and got['tiles'] == 6 and got['head_fp32_repeats'] == 0
    logits = S.segment_compressed([z.read_chunk_bytes(i) for i in tiles], z.codec, seg).cpu().numpy()
    mosaic = np.zeros((classes, 2 * patch, 3 * patch), dtype=np.float32)
    for (i, j, _), lg in zip(tiles, logits):
        mosaic[:, i * patch:(i + 1) * patch, j * patch:(j + 1) * patch] = lg
    mosaic = np.ascontiguousarray(mosaic[:, :H, :W])
    t = np.float32(S.threshold_logit(thr))
    cls, counts = oracle(mosaic.reshape(1, classes, -1), labels.reshape(1, -1), t, 5)
    zc = zarrio.ZarrArray.open(out_store, 'class/0/0')
    assert zc.shape == (H, W) and zc.chunks == (patch, patch) and zc.dtype.str == ('|b1' if classes == 1 else '|u1')
    assert zc.meta['compressor'] == dict(id='zlib', level=9)
    assert np.array_equal(zc[:].astype(np.uint8), cls.reshape(H, W))
    for idx in zc.chunk_indices():  # edge chunks: the crop, zero-padded
        sl = zc.chunk_slices(idx)
        assert np.array_equal(zc.read_chunk(idx)[:sl[0].stop - sl[0].start, :sl[1].stop - sl[1].start].astype(np.uint8),
                              cls.reshape(H, W)[sl])
    zs = zarrio.ZarrArray.open(out_store, 'scores/0/0')
    assert zs.shape == (classes, H, W) and zs.dtype == np.float32
    lg = mosaic.reshape(1, classes, -1)
    assert float(np.abs(zs[:].reshape(lg.shape).astype(np.float64) - scores_f64(lg)).max()) <= score_bound(lg)
    want = S.class_metrics(counts[0], multiclass=classes > 1)
    assert got['records'].shape == (6, 6) and np.array_equal(got['records'].sum(axis=0), counts[0])
    for k, v in want.items():
        assert got[k] == v, k
    # without a target and scores: the same class map, no scores array, no metrics
    out2 = str(tmp_path / 'pred2.zarr')
    plain = zarrio.segment_image(store, seg, out2, batch_tiles=4, threshold=thr, coder='device')
    assert 'acc' not in plain and np.array_equal(zarrio.ZarrArray.open(out2, 'class/0/0')[:].astype(np.uint8),
                                                  cls.reshape(H, W))
    import os
    assert not os.path.exists(os.path.join(out2, 'scores'))
