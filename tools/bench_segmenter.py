#!/usr/bin/env python3
"""Measure the canonical segmentation head (192 / 128 / 64 / 1024, four levels, bridges concatenated) on one device.

    python tools/bench_segmenter.py [--out profiles/segmenter_mi355x.json] [--shapes 32x256,4x1024] [--no-trace]

Per batch shape (tiles x tile edge):
  * device time per batch, median of 9 runs after 2 warm-ups (events around the call), for the HIP kernels and for the
    same head as torch ops on the same device (force_torch=True) -- the comparison this feature is held to;
  * per-kernel times from ONE `rocprofv3 --kernel-trace --stats` run of a fresh child process (`--child`), taken on its
    own (no counters, no other tracing);
  * issued f16 MFMA FLOP/s over 2500 TFLOP/s (the dense f16 peak of an MI355X), per convolution and over the head.
    Issued = 3 products (f16x3) x 2 x padded rows x padded contraction x taps x padded pixels: what the matrix pipes
    execute, padding included.
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
PEAK = 2500e12


def setup(n, edge):
    import torch
    from cnn_autoencoder_amd import segmenters
    torch.manual_seed(0)
    m = segmenters.JNet(**CANON).cuda().eval()
    L = CANON['compression_level']
    l = edge >> L
    g = torch.Generator().manual_seed(1)
    y_q = torch.round(3 * torch.randn(n, CANON['channels_bn'], l, l, generator=g)).cuda()
    ch = [CANON['channels_net']] * (L - 1) + [3]
    brg = [torch.rand(n, c, l << (i + 1), l << (i + 1), generator=g).cuda() for i, c in enumerate(ch)]
    return m, y_q, brg


def issued_flops(m, n, edge):
    """per stage of m.stage_plan(): (name, issued f16 MFMA FLOPs) with the kernel's padding (32-row channel tiles,
    16-channel chunks over the plane grids of the sources, 8 x 16 pixel tiles)"""
    from cnn_autoencoder_amd import _lib
    import ctypes
    tx, ty = ctypes.c_int(), ctypes.c_int()
    _lib.lib().cae_seg_tile(ctypes.byref(tx), ctypes.byref(ty))
    plan, out = m.stage_plan(), []
    size = edge >> CANON['compression_level']
    sizes = []
    for st in plan:
        sizes.append(size)  # input extent of the stage
        if st['up']:
            size *= 2
    for st, s in zip(plan, sizes):
        w = st['weight']
        cout = w.shape[1] if st['up'] else w.shape[0]
        rows = 4 * ((cout + 7) // 8 * 8) if st['up'] else cout
        rows = (rows + 31) // 32 * 32
        if st['up']:
            planes = (w.shape[0] + 7) // 8
        elif len(st['srcs']) == 2:
            planes = 2 * ((w.shape[1] // 2 + 7) // 8)
        else:
            planes = (w.shape[1] + 7) // 8
        k = (planes + 1) // 2 * 16
        pix = ((s + ty.value - 1) // ty.value) * ((s + tx.value - 1) // tx.value) * tx.value * ty.value
        out.append((st['name'], 3 * 2 * rows * k * st['ks'] ** 2 * pix * n))
    return out


def timed(fn, runs=9, warm=2):
    import torch
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), ms


def child(n, edge):
    import torch
    m, y_q, brg = setup(n, edge)
    with torch.no_grad():
        for _ in range(3):
            m(y_q, brg)
    torch.cuda.synchronize()


def trace(n, edge):
    """-> (kernel stats rows, per-dispatch durations of the last call's convolutions in launch order) or (None, None)"""
    prof = shutil.which('rocprofv3')
    if prof is None:
        return None, None
    d = tempfile.mkdtemp(prefix='seg_trace_')
    try:
        cmd = [prof, '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable,
               os.path.abspath(__file__), '--child', f'{n}x{edge}']
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return None, None
        stats, per_call = [], []
        for f in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
            stats = [dict(name=row.get('Name'), calls=int(row.get('Calls', 0)), total_ns=int(row.get('TotalDurationNs', 0)),
                          average_ns=float(row.get('AverageNs', 0))) for row in csv.DictReader(open(f))]
        for f in glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True):
            rows = sorted(csv.DictReader(open(f)), key=lambda row: int(row['Start_Timestamp']))
            conv = [int(row['End_Timestamp']) - int(row['Start_Timestamp']) for row in rows if 'seg_conv_f16_kernel' in row['Kernel_Name']]
            per_call = conv[-(len(conv) // 3):] if conv else []
        return stats, per_call
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'segmenter_mi355x.json'))
    ap.add_argument('--shapes', default='32x256,4x1024')
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--child', default=None)
    a = ap.parse_args()
    if a.child:
        n, edge = map(int, a.child.split('x'))
        return child(n, edge)
    import torch
    result = dict(device=torch.cuda.get_device_name(0), config=CANON, peak_f16_flops=PEAK, shapes=[])
    for shape in a.shapes.split(','):
        n, edge = map(int, shape.split('x'))
        m, y_q, brg = setup(n, edge)
        with torch.no_grad():
            hip_ms, hip_all = timed(lambda: m(y_q, brg))
            m.force_torch = True
            torch_ms, torch_all = timed(lambda: m(y_q, brg))
            m.force_torch = False
        flops = issued_flops(m, n, edge)
        total = sum(f for _, f in flops)
        entry = dict(tiles=n, edge=edge, hip_ms=hip_ms, torch_ms=torch_ms, hip_runs_ms=hip_all, torch_runs_ms=torch_all,
                     issued_f16_flops=total, head_fraction_of_peak=total / (hip_ms * 1e-3) / PEAK)
        del m, y_q, brg
        torch.cuda.empty_cache()
        if not a.no_trace:
            stats, per_call = trace(n, edge)
            entry['kernel_stats'] = stats
            if per_call and len(per_call) == len(flops):
                entry['convolutions'] = [dict(name=name, ns=ns, issued_f16_flops=f, fraction_of_peak=f / (ns * 1e-9) / PEAK)
                                         for (name, f), ns in zip(flops, per_call)]
        result['shapes'].append(entry)
        print(json.dumps({k: v for k, v in entry.items() if k not in ('kernel_stats', 'convolutions', 'hip_runs_ms', 'torch_runs_ms')}),
              flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
