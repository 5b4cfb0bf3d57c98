"""Host side of the prediction from the head's logits (segmenters.predict / class_metrics, slide.gather_counts,
cae_seg_predict's argument checks).  No GPU: the ABI calls below are refused before anything touches a device, the
pointers they carry are never followed."""
import ctypes
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _reference_metrics(tp, tn, fp, fn, p, tp_top, multiclass):
    """compute_class_metrics_dask lines 50-59 of the reference on given counts (tn_top = tn), with zero_division=0 of the
    per-image variant for prec / rec / f1"""
    total = tp + tn + fp + fn
    acc = (tp + tn) / total if total > 0 else float('nan')
    top = (tp_top + tn) / total if total > 0 else float('nan')
    prec = tp / (tp + fp) if tp + fp > 0 else 0.0
    rec = tp / (tp + fn) if tp + fn > 0 else 0.0
    f1 = 2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn > 0 else 0.0
    return dict(tp=tp, tp_top=tp_top, tn=tn, fp=fp, fn=fn, p=p, n=0 if multiclass else tn + fp, acc=acc, top_acc=top,
                prec=prec, rec=rec, f1=f1)


def _same(got, want):
    assert set(got) == set(want) == {'tp', 'tp_top', 'tn', 'fp', 'fn', 'p', 'n', 'acc', 'top_acc', 'prec', 'rec', 'f1'}
    for k, v in want.items():
        if isinstance(v, float) and math.isnan(v):
            assert math.isnan(got[k]), k
        else:
            assert got[k] == v, (k, got[k], v)


RECORDS = [((30, 50, 12, 8, 38, 30), False),     # a binary tile
           ((0, 100, 0, 0, 0, 0), False),        # all background, nothing predicted: prec / rec / f1 denominators zero
           ((0, 0, 0, 64, 64, 0), False),        # all foreground, nothing predicted: precision's denominator zero
           ((0, 0, 0, 0, 0, 0), False),          # an empty record: every denominator zero, acc NaN
           ((70, 0, 30, 30, 100, 95), True),     # several classes: fp = fn = pixels - tp, p = pixels
           ((0, 0, 100, 100, 100, 0), True)]


@pytest.mark.parametrize('rec,multi', RECORDS)
def test_class_metrics_follow_the_reference_formulas(rec, multi):
    from cnn_autoencoder_amd import segmenters
    want = _reference_metrics(*rec, multi)
    _same(segmenters.class_metrics(rec, multiclass=multi), want)
    _same(segmenters.class_metrics(np.array(rec, dtype=np.int64), multiclass=multi), want)
    _same(segmenters.class_metrics(torch.tensor(rec), multiclass=multi), want)


def test_class_metrics_of_a_sum_of_records():
    from cnn_autoencoder_amd import segmenters
    recs = np.array([r for r, multi in RECORDS if not multi], dtype=np.int64)
    want = _reference_metrics(*[int(v) for v in recs.sum(axis=0)], False)
    _same(segmenters.class_metrics(recs.sum(axis=0)), want)
    _same(segmenters.class_metrics(recs), want)  # an (M, 6) array is summed
    assert want['acc'] == (30 + 150) / 264 and want['p'] == 102 and want['n'] == 162
    with pytest.raises(ValueError):
        segmenters.class_metrics([1, 2, 3])


@pytest.mark.parametrize('thr', [0.0, 1.0, 1.5, -0.1, float('nan')])
def test_predict_refuses_a_score_threshold_outside_the_open_interval(thr):
    from cnn_autoencoder_amd import segmenters
    with pytest.raises(ValueError, match='threshold'):
        segmenters.predict(torch.zeros(1, 1, 4), threshold=thr)
    with pytest.raises(ValueError):
        segmenters.threshold_logit(thr, 'scores')


def test_threshold_logit_conventions():
    from cnn_autoencoder_amd import segmenters
    assert segmenters.threshold_logit(0.5) == 0.0
    assert segmenters.threshold_logit(0.9) == float(np.float32(math.log(0.9 / (1 - 0.9))))
    assert segmenters.threshold_logit(0.9, 'logits') == float(np.float32(0.9))
    assert segmenters.threshold_logit(1.5, 'logits') == 1.5  # any finite logit may be the threshold
    with pytest.raises(ValueError, match='threshold_on'):
        segmenters.threshold_logit(0.5, 'probabilities')
    with pytest.raises(ValueError, match='top_k'):
        segmenters.predict(torch.zeros(1, 3, 4), top_k=0)


def test_bad_arguments_are_refused_before_any_launch(built_lib):
    """every refusal of include/cae_hip.h's list returns CAE_ERR_ARG; n == 0 is CAE_OK; nothing is launched in either case
    (this process has no device, and the pointers are not device memory)"""
    from cnn_autoencoder_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(4096)
    need = L.cae_seg_predict_workspace(2, 3, 1000)
    assert need > 0 and need % 8 == 0

    def call(logits=p, target=p, n=2, c=3, hw=1000, k=5, cls=p, scores=None, counts=p, ws=p, ws_bytes=need):
        return L.cae_seg_predict(logits, target, n, c, hw, 0.0, k, cls, scores, counts, ws, ws_bytes, None)

    for bad in (dict(c=0), dict(c=257), dict(c=-1), dict(n=-1), dict(hw=0), dict(cls=None), dict(logits=None),
                dict(target=None), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=None), dict(k=0), dict(k=-3),
                dict(ws=ctypes.c_void_p(4100))):
        assert call(**bad) == -1, bad
        assert L.cae_last_error().startswith(b'cae_seg_predict'), bad
    assert call(target=None) == -1 and b'target' in L.cae_last_error()
    assert call(ws_bytes=need - 1) == -1 and str(need).encode() in L.cae_last_error()
    with pytest.raises(ValueError):
        _lib.check(call(c=257))
    # n == 0: CAE_OK whatever the pointers, unless another argument is bad
    assert call(n=0) == 0 and call(n=0, cls=None, logits=None, ws=None, ws_bytes=0) == 0
    assert call(n=0, c=0) == -1 and call(n=0, k=0) == -1 and call(n=0, target=None) == -1
    # the workspace: 32 bytes per (image, block), 0 for what the call refuses
    assert L.cae_seg_predict_workspace(0, 3, 1000) == 0 and L.cae_seg_predict_workspace(2, 0, 1000) == 0
    assert L.cae_seg_predict_workspace(2, 257, 1000) == 0 and L.cae_seg_predict_workspace(2, 3, 0) == 0
    assert L.cae_seg_predict_workspace(1, 1, 1) == 32 and L.cae_seg_predict_workspace(3, 7, 1025) == 3 * 2 * 32
    assert L.cae_seg_predict_workspace(4, 1, 1024 * 1024) == 4 * 1024 * 32


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _records(lo, hi):
    idx = torch.arange(lo, hi, dtype=torch.int64)
    return torch.stack([idx * 7 + j * (2 ** 33) for j in range(6)], dim=1)  # values beyond 32 bits


def _worker(rank, world, port, n_tiles, out_dir):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from cnn_autoencoder_amd import slide
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    lo, hi = slide.tile_range(rank, world, n_tiles)
    got = slide.gather_counts(_records(lo, hi))
    torch.save(dict(counts=got, range=(lo, hi)), os.path.join(out_dir, f'rank{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize('n_tiles', [5, 1])
def test_two_ranks_gather_ragged_counts(tmp_path, n_tiles):
    """5 tiles over two ranks are 3 + 2 (1 tile: 1 + 0): every rank ends with all records, int64, in tile order"""
    from cnn_autoencoder_amd import slide
    mp.spawn(_worker, args=(2, _free_port(), n_tiles, str(tmp_path)), nprocs=2, join=True)
    res = [torch.load(str(tmp_path / f'rank{r}.pt'), weights_only=False) for r in range(2)]
    assert res[0]['range'] == slide.tile_range(0, 2, n_tiles) and res[1]['range'][1] == n_tiles
    if n_tiles == 5:
        assert res[0]['range'] == (0, 3) and res[1]['range'] == (3, 5)
    for r in res:
        assert r['counts'].dtype == torch.int64 and r['counts'].shape == (n_tiles, slide.COUNTS_WIDTH)
        assert torch.equal(r['counts'], _records(0, n_tiles))


def test_gather_counts_without_a_process_group():
    from cnn_autoencoder_amd import slide
    local = _records(0, 4)
    got = slide.gather_counts(local)
    assert torch.equal(got, local) and got.data_ptr() != local.data_ptr()
    with pytest.raises(ValueError):
        slide.gather_counts(torch.zeros((4, 3), dtype=torch.int64))
    with pytest.raises(ValueError):
        slide.gather_counts(torch.zeros((4, 6), dtype=torch.float64))


def test_the_ring_table_has_the_class_map_ring_and_keeps_the_others():
    from cnn_autoencoder_amd import slide
    sc = object.__new__(slide.SlideCoder)
    sc.depth, sc._rings = 3, {}
    assert sc._ring('c').slots == 4
    assert [sc._ring(k).slots for k in 'tados'] == [2, 4, 5, 4, 3]
