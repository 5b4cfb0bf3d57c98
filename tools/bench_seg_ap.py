#!/usr/bin/env python3
"""Measure the score histogram kernels (cae_seg_score_hist, csrc/cae_seg_hist.hip) on one device.  A record, no verdict.

    python tools/bench_seg_ap.py [--out profiles/seg_ap/kernel_times_mi355x.json] [--batch 4x1024] [--classes 2,5,16]
                                 [--bits 11,14]

cae_seg_score_hist (both launches, the micro histogram) beside cae_seg_predict with scores and counts on the same
inputs -- the call that writes the scores the histogram reads -- and the head's 63 ms per 4 x 1024^2 batch (DESIGN
"Segmentation head"): device time per call by the method of tools/bench_segment_slide.py -- events around `--inner`
back-to-back calls that cycle through buffer sets of `--footprint-mib` in all, more than the 256 MiB Infinity Cache
holds, median of 9 groups after 2 warm-up groups, min and max beside it -- for logits that are sharp (N(0, 4^2), the
target's class raised by 3: most scores near 0 or 1, a trained head) and flat (N(0, 0.3^2): scores near 1 / C); the bytes
that must move (4 C + C per pixel in, the int64 table out) over the time as a fraction of 6.3 TB/s.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_segment_slide import HBM_ACHIEVABLE, timed_groups  # noqa: E402

HEAD_MS = 63.0  # the head's forward on a 4 x 1024^2 batch (DESIGN "Segmentation head")


def draw(n, c, edge, kind, g):
    import torch
    target = torch.randint(0, c, (n, edge, edge), generator=g, device='cuda').to(torch.uint8)
    if kind == 'flat':
        return 0.3 * torch.randn(n, c, edge, edge, generator=g, device='cuda'), target
    x = 4 * torch.randn(n, c, edge, edge, generator=g, device='cuda')
    x.scatter_add_(1, target[:, None].long(), torch.full((n, 1, edge, edge), 3.0, device='cuda'))
    return x, target


def bench(n, c, edge, bits, kind, inner, footprint):
    import torch
    from cnn_autoencoder_amd import _lib, segmenters
    hw = edge * edge
    nbytes = n * hw * 5 * c + 2 * (1 << bits) * 8
    sets = max(2, -(-footprint // (n * hw * 4 * c)))
    g = torch.Generator(device='cuda').manual_seed(edge + bits + c)
    L = _lib.lib()
    st = _lib.stream_ptr()
    ws_bytes = int(L.cae_seg_score_workspace(n, c, edge, edge, bits))
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device='cuda')
    hist = torch.empty((2, 1 << bits), dtype=torch.int64, device='cuda')
    pws_bytes = int(L.cae_seg_predict_workspace(n, c, hw))
    pws = torch.empty(max(pws_bytes // 8, 1), dtype=torch.int64, device='cuda')
    cls = torch.empty((n, edge, edge), dtype=torch.uint8, device='cuda')
    counts = torch.empty((n, 6), dtype=torch.int64, device='cuda')
    bufs = []
    for _ in range(sets):
        logits, target = draw(n, c, edge, kind, g)
        bufs.append((logits, target, segmenters.predict(logits, scores=True)['scores']))
    at = [0]

    def score_hist():
        _, target, scores = bufs[at[0] % sets]
        at[0] += 1
        _lib.check(L.cae_seg_score_hist(scores.data_ptr(), target.data_ptr(), None, n, c, edge, edge, bits, 0, 0,
                                        hist.data_ptr(), ws.data_ptr(), ws_bytes, st))

    def predict():
        logits, target, scores = bufs[at[0] % sets]
        at[0] += 1
        _lib.check(L.cae_seg_predict(logits.data_ptr(), target.data_ptr(), n, c, hw, 0.0, 5, cls.data_ptr(),
                                     scores.data_ptr(), counts.data_ptr(), pws.data_ptr(), pws_bytes, st))

    at[0] = 0
    score_hist()
    torch.cuda.synchronize()
    whole = int(hist.sum()) == n * hw * c and int(hist[1].sum()) == n * hw
    pr = segmenters.ap_from_histogram(hist)
    hist_ms, hist_all = timed_groups(score_hist, inner)
    pred_ms, pred_all = timed_groups(predict, inner)
    return dict(images=n, classes=c, edge=edge, bits=bits, logits=kind, buffer_sets=sets, workspace_bytes=ws_bytes,
                blocks_per_plane=ws_bytes // (n * c * (8 << bits)), hist_us=1e3 * hist_ms, hist_min_us=1e3 * min(hist_all),
                hist_max_us=1e3 * max(hist_all), predict_us=1e3 * pred_ms, predict_min_us=1e3 * min(pred_all),
                predict_max_us=1e3 * max(pred_all), head_ms=HEAD_MS if (n, edge) == (4, 1024) else None,
                hist_runs_ms=hist_all, predict_runs_ms=pred_all, bytes=nbytes,
                fraction_of_achievable_hbm=nbytes / (hist_ms * 1e-3) / HBM_ACHIEVABLE, every_pair_counted=whole,
                avg_prec=pr['avg_prec'], avg_prec_lo=pr['avg_prec_lo'], avg_prec_hi=pr['avg_prec_hi'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'seg_ap', 'kernel_times_mi355x.json'))
    ap.add_argument('--batch', default='4x1024')
    ap.add_argument('--classes', default='2,5,16')
    ap.add_argument('--bits', default='11,14')
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--footprint-mib', type=int, default=768, help='score bytes the timed calls cycle through')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_seg_ap.py measures on a HIP device; none is visible')
    n, edge = map(int, a.batch.split('x'))
    result = dict(device=torch.cuda.get_device_name(0), hbm_achievable=HBM_ACHIEVABLE, kernel=[])
    for c in (int(v) for v in a.classes.split(',')):
        for bits in (int(b) for b in a.bits.split(',')):
            for kind in ('sharp', 'flat'):
                row = bench(n, c, edge, bits, kind, a.inner, a.footprint_mib << 20)
                result['kernel'].append(row)
                print(json.dumps({k: v for k, v in row.items() if not k.endswith('runs_ms')}), flush=True)
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
