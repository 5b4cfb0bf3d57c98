#!/usr/bin/env python3
"""Measure the tissue mask (csrc/cae_mask.hip, cnn_autoencoder_amd/tissue.py) on one device.

    python tools/bench_tissue.py [--out profiles/tissue_mi355x.json] [--edge 3072] [--no-trace] [--no-host]

The image is the procedural `histo` tile at edge x edge (3072: a 40x slide of about 98k^2 pixels at 1/32).
  device: tissue_mask on the image resident on the device, median of 9 calls after 2 warm-ups, each timed by device
          events and by the host clock around the call and a synchronise (the call holds two small device-to-host
          copies and the host's threshold, so the two differ by what the host adds);
  kernels: per-kernel rows of ONE `rocprofv3 --kernel-trace --stats` run of a fresh child process (`--child`) that makes
          3 calls; taken on its own so that tracing does not sit in the timings above;
  host:   the numpy / scipy restatement of the same contract (tests/tissue_restatement.py) on this machine's CPU, one
          run, as context and not as a threshold; its mask is compared with the device's for equality.
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
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

WARMUPS, RUNS = 2, 9


def image(edge):
    from cnn_autoencoder_amd import synth
    return synth.histo_tile(edge, 0)


def child(edge):
    import torch
    from cnn_autoencoder_amd import tissue
    img = torch.from_numpy(image(edge)).cuda()
    for _ in range(3):
        tissue.tissue_mask(img)
    torch.cuda.synchronize()


def trace(edge):
    """-> kernel stats rows of the child's 3 calls, or None where rocprofv3 is missing or fails"""
    prof = shutil.which('rocprofv3')
    if prof is None:
        return None
    d = tempfile.mkdtemp(prefix='tissue_trace_')
    try:
        cmd = [prof, '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable,
               os.path.abspath(__file__), '--child', '--edge', str(edge)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return None
        rows = []
        for f in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
            rows = [dict(name=row.get('Name'), calls=int(row.get('Calls', 0)), total_ns=int(row.get('TotalDurationNs', 0)),
                         average_ns=float(row.get('AverageNs', 0))) for row in csv.DictReader(open(f))]
        return rows
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tissue_mi355x.json'))
    ap.add_argument('--edge', type=int, default=3072)
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--no-host', action='store_true', help='leave out the host restatement (and the comparison with it)')
    ap.add_argument('--child', action='store_true')
    a = ap.parse_args()
    if a.child:
        return child(a.edge)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_tissue.py measures on a HIP device; none is visible')
    from cnn_autoencoder_amd import tissue
    img = image(a.edge)
    on_dev = torch.from_numpy(img).cuda()
    event_ms, wall_ms = [], []
    for k in range(WARMUPS + RUNS):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        mask = tissue.tissue_mask(on_dev)
        e1.record()
        torch.cuda.synchronize()
        if k >= WARMUPS:
            wall_ms.append((time.perf_counter() - t0) * 1e3)
            event_ms.append(e0.elapsed_time(e1))
    pixels = a.edge * a.edge
    result = dict(device=torch.cuda.get_device_name(0), edge=a.edge, pixels=pixels, warmups=WARMUPS, runs=RUNS,
                  parameters=dict(min_size=256, area_threshold=16384, radius=16),
                  tissue_fraction=float(mask.float().mean()),
                  device_ms=statistics.median(event_ms), device_min_ms=min(event_ms), device_max_ms=max(event_ms),
                  device_runs_ms=event_ms, wall_ms=statistics.median(wall_ms), wall_runs_ms=wall_ms,
                  pixels_per_s=pixels / (statistics.median(event_ms) * 1e-3))
    print(json.dumps({k: v for k, v in result.items() if not k.endswith('runs_ms')}), flush=True)
    if not a.no_trace:
        rows = trace(a.edge)
        result['kernel_stats_calls'] = 3
        result['kernel_stats'] = rows
        if rows:
            mine = [r for r in rows if any(s in r['name'] for s in ('mask_', 'obj_', 'wd_'))]
            result['kernel_ms_per_call'] = sum(r['total_ns'] for r in mine) / 3e6
            for r in sorted(mine, key=lambda r: -r['total_ns']):
                print(f"  {r['total_ns'] / 3e6:9.3f} ms/call  {r['calls'] // 3} x  {r['name'][:100]}", flush=True)
    if not a.no_host:
        import tissue_restatement as R
        t0 = time.perf_counter()
        want = R.tissue_mask(img)
        result['host_ms'] = (time.perf_counter() - t0) * 1e3
        result['host_cpus'] = os.cpu_count()
        result['equal_to_host'] = bool(np.array_equal(mask.cpu().numpy(), want['mask']))
        result['host_over_device'] = result['host_ms'] / result['device_ms']
        print(json.dumps(dict(host_ms=result['host_ms'], equal_to_host=result['equal_to_host'])), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
