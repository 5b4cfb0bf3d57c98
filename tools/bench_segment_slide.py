#!/usr/bin/env python3
"""Measure the prediction from the head's logits and the slide segmentation driver on one device.

    python tools/bench_segment_slide.py [--out profiles/segment_slide_mi355x.json] [--shapes 4x1024,32x256]
                                        [--classes 1,5] [--batches 8] [--no-pipeline]

(a) cae_seg_predict against the same result as torch ops on the device (sigmoid / softmax, compare / argmax, counts by
    boolean sums and topk), with a target, with and without scores: device time per call, median of 9 timed groups of
    `--inner` back-to-back calls after 2 warm-up groups (events around a group: a single call is tens of microseconds),
    the calls cycling through buffer sets of `--footprint-mib` in all, more than the 256 MiB Infinity Cache holds;
    the bytes the kernel must move (logits in, target in, class map out, scores out) over its time as a fraction of
    6.3 TB/s, the achievable HBM rate of an MI355X (8 TB/s peak is printed beside it).
(b) SlideCoder.segment_batches(to_host=True) in tiles/s against the unpipelined loop it replaces on the same chunk bytes
    (segment_compressed, logits .cpu(), numpy argmax / compare), canonical codec and head, wall time per pass, median
    of `--runs` after 2 warm-ups; the shares of the driver's stages from SlideCoder.timers.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE, HBM_PEAK = 6.3e12, 8.0e12
HEAD = dict(channels_bn=192, channels_net=128, seg_channels_net=64, seg_channels_expansion=2, seg_channels_bn=1024,
            compression_level=4, concat_bridges=True)


def timed_groups(fn, inner, runs=9, warm=2):
    """-> (median, all) milliseconds per call of fn, from events around groups of `inner` calls"""
    import torch
    out = []
    for r in range(warm + runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        if r >= warm:
            out.append(a.elapsed_time(b) / inner)
    return statistics.median(out), out


def must_move(n, c, hw, scores):
    return n * hw * (4 * c + 1 + 1 + (4 * c if scores else 0))


def torch_predict(logits, target, t, top_k, scores):
    """the same result as torch ops: (cls, scores, counts)"""
    import torch
    n, c = logits.shape[:2]
    lg = logits.reshape(n, c, -1)
    tg = target.reshape(n, -1)
    if c == 1:
        on = lg[:, 0] > t
        pos = tg > 0
        tp, tn = (on & pos).sum(1), (~on & ~pos).sum(1)
        fp, fn = (on & ~pos).sum(1), (~on & pos).sum(1)
        counts = torch.stack([tp, tn, fp, fn, pos.sum(1), tp], dim=1)
        return on.to(torch.uint8), (torch.sigmoid(lg) if scores else None), counts
    cls = lg.argmax(dim=1)
    tp = (cls == tg).sum(1)
    top = (lg.topk(min(top_k, c), dim=1)[1] == tg[:, None, :]).any(dim=1).sum(1)
    hw = torch.full_like(tp, lg.shape[2])
    counts = torch.stack([tp, torch.zeros_like(tp), hw - tp, hw - tp, hw, top], dim=1)
    return cls.to(torch.uint8), (torch.softmax(lg, dim=1) if scores else None), counts


def bench_kernel(n, edge, c, scores, inner, footprint):
    import torch
    from cnn_autoencoder_amd import _lib
    hw = edge * edge
    nbytes = must_move(n, c, hw, scores)
    # the timed calls walk round `sets` buffer sets of `footprint` bytes in all: more than the Infinity Cache holds, so that
    # no call finds its logits on the die from the call before
    sets = max(2, -(-footprint // nbytes))
    g = torch.Generator().manual_seed(c + edge)
    L = _lib.lib()
    ws_bytes = int(L.cae_seg_predict_workspace(n, c, hw))
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device='cuda')
    counts = torch.empty((n, 6), dtype=torch.int64, device='cuda')
    bufs = []
    for _ in range(sets):
        logits = (5 * torch.randn(n, c, hw, generator=g)).cuda()
        target = torch.randint(0, max(c, 2), (n, hw), generator=g, dtype=torch.uint8).cuda()
        bufs.append((logits, target, torch.empty((n, hw), dtype=torch.uint8, device='cuda'),
                     torch.empty_like(logits) if scores else None))
    st = _lib.stream_ptr()
    at = [0]

    def hip():
        logits, target, cls, sc = bufs[at[0] % sets]
        at[0] += 1
        _lib.check(L.cae_seg_predict(logits.data_ptr(), target.data_ptr(), n, c, hw, 0.0, 5, cls.data_ptr(),
                                     None if sc is None else sc.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws_bytes, st))

    def ops():
        logits, target, _, _ = bufs[at[0] % sets]
        at[0] += 1
        return torch_predict(logits, target, 0.0, 5, scores)

    at[0] = 0
    hip()
    at[0] = 0
    ref = ops()
    torch.cuda.synchronize()
    same = bool(torch.equal(bufs[0][2], ref[0]) and torch.equal(counts, ref[2]))  # (random fp32 logits: no top-k ties)
    hip_ms, hip_all = timed_groups(hip, inner)
    torch_ms, torch_all = timed_groups(ops, max(inner // 4, 1))
    return dict(tiles=n, edge=edge, classes=c, scores=scores, buffer_sets=sets, hip_ms=hip_ms, torch_ms=torch_ms,
                hip_runs_ms=hip_all, torch_runs_ms=torch_all, bytes=nbytes, hip_bytes_per_s=nbytes / (hip_ms * 1e-3),
                fraction_of_achievable_hbm=nbytes / (hip_ms * 1e-3) / HBM_ACHIEVABLE,
                fraction_of_peak_hbm=nbytes / (hip_ms * 1e-3) / HBM_PEAK, equal_to_torch_ops=same)


def bench_pipeline(n, edge, c, batches, runs):
    import numpy as np
    import torch
    import cnn_autoencoder_amd as cae
    from cnn_autoencoder_amd import segmenters, slide, synth
    codec = cae.ConvolutionalAutoencoder(checkpoint=synth.synthetic_state(dict(synth.CANONICAL), seed=0))
    torch.manual_seed(0)
    seg = segmenters.JNet(**dict(HEAD, num_classes=c)).cuda().eval()
    tiles = np.stack([synth.histo_tile(edge, i % 4) for i in range(n)])
    bufs = codec.encode_batch(tiles)
    groups = [bufs] * batches
    sc = slide.SlideCoder(codec)

    def pipelined():
        done = 0
        for res in sc.segment_batches(groups, edge, edge, seg, to_host=True):
            done += res['cls'].shape[0]
        return done

    def loop():
        done = 0
        for g in groups:
            lg = segmenters.segment_compressed(g, codec, seg).cpu().numpy()
            cls = (lg[:, 0] > 0) if c == 1 else lg.argmax(axis=1).astype(np.uint8)
            done += cls.shape[0]
        return done

    def wall(fn):
        out = []
        for r in range(2 + runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= 2:
                out.append(time.perf_counter() - t0)
        return statistics.median(out), out

    pipe_s, pipe_all = wall(pipelined)
    timers = dict(sc.timers)
    loop_s, loop_all = wall(loop)
    total = n * batches
    stage = {k: v for k, v in timers.items() if k != 'head_fp32_repeats'}
    return dict(tiles_per_batch=n, edge=edge, classes=c, batches=batches, pipelined_s=pipe_s, loop_s=loop_s,
                pipelined_runs_s=pipe_all, loop_runs_s=loop_all, pipelined_tiles_per_s=total / pipe_s,
                loop_tiles_per_s=total / loop_s, timers_s=timers,
                shares_of_pass={k: v / pipe_s for k, v in stage.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'segment_slide_mi355x.json'))
    ap.add_argument('--shapes', default='4x1024,32x256')
    ap.add_argument('--classes', default='1,5')
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--footprint-mib', type=int, default=768, help='bytes the timed kernel calls cycle through')
    ap.add_argument('--batches', type=int, default=8)
    ap.add_argument('--runs', type=int, default=9)
    ap.add_argument('--no-pipeline', action='store_true')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_segment_slide.py measures on a HIP device; none is visible')
    shapes = [tuple(map(int, s.split('x'))) for s in a.shapes.split(',')]
    classes = [int(c) for c in a.classes.split(',')]
    result = dict(device=torch.cuda.get_device_name(0), hbm_achievable=HBM_ACHIEVABLE, hbm_peak=HBM_PEAK, kernel=[],
                  pipeline=[])
    for n, edge in shapes:
        for c in classes:
            for scores in (False, True):
                row = bench_kernel(n, edge, c, scores, a.inner, a.footprint_mib << 20)
                result['kernel'].append(row)
                print(json.dumps({k: v for k, v in row.items() if not k.endswith('runs_ms')}), flush=True)
                torch.cuda.empty_cache()
    if not a.no_pipeline:
        for n, edge in shapes:
            row = bench_pipeline(n, edge, classes[-1], a.batches, a.runs)
            result['pipeline'].append(row)
            print(json.dumps({k: v for k, v in row.items() if not k.endswith('runs_s')}), flush=True)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
