#!/usr/bin/env python3
"""Measure one training step of the canonical segmentation head (192 / 128 / 64 / 1024, four levels, bridges
concatenated) at 32 x 256^2 on one device.

    python tools/bench_segmenter_train.py [--out profiles/segmenter_train_mi355x.json] [--shape 32x256] [--no-trace]

  * forward + backward device time per step, median of 9 runs after 2 warm-ups (events around the step), for the
    JNetTrain kernels and for the same head as differentiable torch ops on the same device (force_torch=True), in the
    same visit;
  * the optimiser step (train.fused_clip_adam over the head's parameters), timed the same way;
  * peak memory: torch's allocator peak and the device memory in use (the handle's workspaces are not torch's);
  * per-stage max|s g| of one backward under the step's one host-read scale (what the per-stage renormalisation sees);
  * per-kernel rows from ONE `rocprofv3 --kernel-trace --stats` run of a fresh child process (`--child`), taken on its
    own, and the share of the NCHW <-> C8 conversions in it.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CANON = dict(channels_bn=192, channels_net=128, seg_channels_net=64, seg_channels_expansion=2, seg_channels_bn=1024,
             compression_level=4, concat_bridges=True)


def setup(n, edge, force_torch=False):
    import torch
    from cnn_autoencoder_amd import seg_train
    torch.manual_seed(0)
    m = seg_train.JNetTrain(**CANON, force_torch=force_torch).cuda().train()
    L = CANON['compression_level']
    l = edge >> L
    g = torch.Generator().manual_seed(1)
    y_q = torch.round(3 * torch.randn(n, CANON['channels_bn'], l, l, generator=g)).cuda()
    ch = [CANON['channels_net']] * (L - 1) + [3]
    brg = [torch.rand(n, c, l << (i + 1), l << (i + 1), generator=g).cuda() for i, c in enumerate(ch)]
    target = torch.randint(0, 2, (n, 1, edge, edge), generator=g).float().cuda()
    return m, y_q, brg, target


def step(m, y_q, brg, target):
    import torch.nn.functional as F
    for p in m.parameters():
        p.grad = None
    F.binary_cross_entropy_with_logits(m(y_q, brg)[0], target).backward()


def timed(fn, runs=9, warm=2, before=None):
    import torch
    ms = []
    for i in range(warm + runs):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warm:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), ms


def measure(n, edge, force_torch):
    import torch
    from cnn_autoencoder_amd import seg_train, train
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    m, y_q, brg, target = setup(n, edge, force_torch)
    opts = seg_train.setup_optim(m)
    fb_ms, fb_all = timed(lambda: step(m, y_q, brg, target))
    fused = []
    opt_ms, opt_all = timed(lambda: fused.append(train.fused_clip_adam(opts, max_norm=1.0)),
                            before=lambda: step(m, y_q, brg, target))
    free, total = torch.cuda.mem_get_info()
    out = dict(forward_backward_ms=fb_ms, forward_backward_runs_ms=fb_all, optimiser_ms=opt_ms, optimiser_runs_ms=opt_all,
               optimiser_fused=all(fused), torch_peak_bytes=torch.cuda.max_memory_allocated(), device_used_bytes=total - free)
    if not force_torch:
        m.record_grad_stats = True
        step(m, y_q, brg, target)
        m.check_backward()
        out['grad_stats'] = m.last_grad_stats
    return out


def child(n, edge):
    import torch
    m, y_q, brg, target = setup(n, edge)
    for _ in range(3):
        step(m, y_q, brg, target)
    torch.cuda.synchronize()


def trace(n, edge):
    prof = shutil.which('rocprofv3')
    if prof is None:
        return None
    d = tempfile.mkdtemp(prefix='seg_train_trace_')
    try:
        cmd = [prof, '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable,
               os.path.abspath(__file__), '--child', f'{n}x{edge}']
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return None
        stats = []
        for f in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
            stats = [dict(name=row.get('Name'), calls=int(row.get('Calls', 0)), total_ns=int(row.get('TotalDurationNs', 0)),
                          average_ns=float(row.get('AverageNs', 0))) for row in csv.DictReader(open(f))]
        return stats
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'segmenter_train_mi355x.json'))
    ap.add_argument('--shape', default='32x256')
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--child', default=None)
    a = ap.parse_args()
    if a.child:
        return child(*map(int, a.child.split('x')))
    import torch
    n, edge = map(int, a.shape.split('x'))
    result = dict(device=torch.cuda.get_device_name(0), config=CANON, tiles=n, edge=edge)
    result['kernels'] = measure(n, edge, False)
    print(json.dumps({k: v for k, v in result['kernels'].items() if not k.endswith('runs_ms')}), flush=True)
    result['torch_ops'] = measure(n, edge, True)
    print(json.dumps({k: v for k, v in result['torch_ops'].items() if not k.endswith('runs_ms')}), flush=True)
    result['kernels_over_torch'] = result['kernels']['forward_backward_ms'] / result['torch_ops']['forward_backward_ms']
    torch.cuda.empty_cache()
    if not a.no_trace:
        stats = trace(n, edge)
        result['kernel_stats'] = stats
        if stats:
            total = sum(r['total_ns'] for r in stats)
            conv = sum(r['total_ns'] for r in stats if 'nchw_to_c8' in r['name'] or 'c8_to_nchw' in r['name'])
            result['layout_conversion_share'] = conv / total if total else None
            print(json.dumps(dict(layout_conversion_share=result['layout_conversion_share'],
                                  top=[(r['name'][:60], r['total_ns']) for r in sorted(stats, key=lambda r: -r['total_ns'])[:8]])),
                  flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
