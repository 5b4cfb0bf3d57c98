#!/usr/bin/env python3
"""Device patch sampler (DESIGN "Training input"): cae_t_sample_patches against the same contract as torch ops on the
device, and the reference-style per-patch transform on the CPU.

    python tools/bench_sampler.py [--steps 9] [--warmup 2] [--train-json FILE ...] [--out FILE] [--no-cpu]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_sampler.py --kernel-only

Batches of 128 and 16 patches of 3 x 256^2 from a pool of 64 tiles of 1024^2 (uint8 HWC, in HBM), one fixed seeded draw.
Columns: plain, noise only (std 0.001), rotation only (+-30 degrees), both.  Per column
  kernel   device time per batch of PatchSampler.gather (HIP events around the call, the upload of the draw included),
           median of --steps after --warmup; bytes/s against the stream floor 5 n C ps^2 bytes (n C ps^2 read,
           4 n C ps^2 written); its share of a RateMSE training step when --train-json names the output lines of
           tools/bench_train.py for these batches (run in the same visit);
  torch    the same for force_torch=True on the device.  Its normals are generated on the host ONCE, outside the timed
           window (the product's torch form generates them per call): the torch time is a lower bound;
  cpu      patches/s of the float32 torch-CPU transform, one patch at a time as the reference's dataset does it (crop,
           / 255, + randn * std, clip, normalise, affine_grid + grid_sample), on 16 threads: 16 workers of one thread
           each, and one worker with 16 intra-op threads.
Labelled columns (key 'labeled'; cae_t_sample_labeled_patches through LabeledPatchSampler.gather, a label pool of K = 2
with the image pool): batches of 128 and 16 patches of 3 x 128^2 (planes filtered in LDS) and 3 x 256^2 (the global-memory
variant), plain and rotated, the same measurement rule (HIP events around gather, median of --steps after --warmup).  Next
to each, the unlabelled PatchSampler.gather of the same batch -- for rotation the bilinear sample_rotate_kernel, the
yardstick the labelled path is reported against -- and the ratio of the two.  --labeled-only measures nothing else.
Prints one JSON line (and writes it to --out).  There is no CPU path for the first two: without a GPU this fails.
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TILES, TILE, PS, C = 64, 1024, 256, 3
COLUMNS = dict(plain=(False, False), noise=(True, False), rotation=(False, True), both=(True, True))
HBM_PEAK = 8.0e12  # bytes/s, MI355X


def device_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


def samplers(pool, noise, rotation, force_torch):
    from cnn_autoencoder_amd.sampler import PatchSampler
    return PatchSampler(pool, PS, add_noise=noise, noise_std=0.001, normalize=True, rotation=rotation, seed=1,
                        force_torch=force_torch)


def measure_device(pool, n, steps, warmup, train_ms, kernel_only=False):
    out = {}
    floor_bytes = 5 * n * C * PS * PS
    for name, (noise, rotation) in COLUMNS.items():
        row = {}
        for form in ('kernel',) if kernel_only else ('kernel', 'torch'):
            s = samplers(pool, noise, rotation, form == 'torch')
            tile, y0, x0, angle = s.draw(n, torch.Generator().manual_seed(n))
            if form == 'kernel':
                fn = lambda: s.gather(tile, y0, x0, angle)  # noqa: E731
            else:
                a = torch.deg2rad(angle) if angle is not None else None
                cs = torch.stack([torch.cos(a), torch.sin(a)]).to(torch.float32) if a is not None else None
                g = s.torch_normals(n, s.seed) if noise else None
                fn = lambda: s._gather_torch(tile, y0, x0, cs, 0.001 if noise else 0.0, g)  # noqa: E731
            r = device_ms(fn, steps, warmup)
            r['bytes_per_s'] = floor_bytes / (1e-3 * r['median_ms'])
            r['share_of_hbm_peak'] = r['bytes_per_s'] / HBM_PEAK
            if train_ms.get(n):
                r['share_of_train_step'] = r['median_ms'] / train_ms[n]
            row[form] = r
        if not kernel_only:
            row['kernel_faster_than_torch'] = row['kernel']['median_ms'] < row['torch']['median_ms']
        out[name] = row
        print(n, name, {k: round(v['median_ms'], 4) for k, v in row.items() if isinstance(v, dict)}, file=sys.stderr)
    return out


def measure_labeled(pool, labels, n, ps, steps, warmup):
    from cnn_autoencoder_amd.sampler import LabeledPatchSampler, PatchSampler
    out = {}
    for name, rotation in (('plain', False), ('rotation', True)):
        kw = dict(normalize=True, rotation=rotation, seed=1)
        s, u = LabeledPatchSampler(pool, labels, ps, **kw), PatchSampler(pool, ps, **kw)
        tile, y0, x0, angle = s.draw(n, torch.Generator().manual_seed(n))
        row = dict(labeled=device_ms(lambda: s.gather(tile, y0, x0, angle), steps, warmup),
                   unlabeled=device_ms(lambda: u.gather(tile, y0, x0, angle), steps, warmup))
        row['labeled_over_unlabeled'] = row['labeled']['median_ms'] / row['unlabeled']['median_ms']
        out[name] = row
        print('labeled', n, ps, name, {k: round(v['median_ms'], 4) for k, v in row.items() if isinstance(v, dict)},
              round(row['labeled_over_unlabeled'], 2), file=sys.stderr)
    return out


def cpu_patch(pool, tile, y0, x0, angle, noise):
    """one patch as the reference's transform makes it (the offsets here lie inside the tile)"""
    x = pool[tile, y0:y0 + PS, x0:x0 + PS].permute(2, 0, 1).to(torch.float32).div(255)
    if noise:
        x = (x + torch.randn(x.size()) * 0.001).clip_(0, 1)
    x = (x - 0.5) / 0.5
    if angle is not None:
        a = np.deg2rad(angle)
        theta = torch.tensor([[[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0]]], dtype=torch.float32)
        grid = F.affine_grid(theta, [1, C, PS, PS], align_corners=False)
        x = F.grid_sample(x[None], grid, mode='bilinear', padding_mode='zeros', align_corners=False)[0]
    return x


def measure_cpu(pool_cpu, n=128, reps=3):
    out = {}
    for name, (noise, rotation) in COLUMNS.items():
        s = samplers(pool_cpu, noise, rotation, False)
        tile, y0, x0, angle = (v.tolist() if v is not None else None for v in s.draw(n, torch.Generator().manual_seed(n)))
        one = lambda i: cpu_patch(pool_cpu, tile[i], y0[i], x0[i], angle[i] if angle else None, noise)  # noqa: E731
        row = {}
        for label, workers, intra in (('workers16_threads1', 16, 1), ('workers1_threads16', 1, 16)):
            torch.set_num_threads(intra)
            best = float('inf')
            with ThreadPoolExecutor(workers) as ex:
                list(ex.map(one, range(16)))  # warm-up
                for _ in range(reps):
                    t0 = time.perf_counter()
                    torch.stack(list(ex.map(one, range(n))))
                    best = min(best, time.perf_counter() - t0)
            row[label + '_patches_per_s'] = n / best
        out[name] = row
        print('cpu', name, {k: round(v) for k, v in row.items()}, file=sys.stderr)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--train-json', nargs='*', default=[], help='output lines of tools/bench_train.py (batch, ms_per_step)')
    ap.add_argument('--out')
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--kernel-only', action='store_true', help='the kernel columns only (for a kernel trace)')
    ap.add_argument('--labeled-only', action='store_true', help='the labelled columns only')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark measures an MI355X; there is no CPU path'
    train_ms = {}
    for path in args.train_json:
        with open(path) as f:
            d = json.loads(f.read().strip().splitlines()[-1])
        train_ms[int(d['batch'])] = float(d['ms_per_step'])
    pool_cpu = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (TILES, TILE, TILE, C), dtype=np.uint8))
    pool = pool_cpu.cuda()
    res = dict(device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, tiles=TILES, tile=TILE, patch=PS,
               channels=C, normalize=True, noise_std=0.001, degrees=30.0, train_step_ms=train_ms)
    labels = torch.from_numpy(np.random.default_rng(1).integers(0, 2, (TILES, TILE, TILE, 2), dtype=np.uint8)).cuda()
    res['labeled'] = {f'batch{n}_patch{ps}': measure_labeled(pool, labels, n, ps, args.steps, args.warmup)
                      for n in (128, 16) for ps in (128, 256)}
    for n in () if args.labeled_only else (128, 16):
        res[f'batch{n}'] = measure_device(pool, n, args.steps, args.warmup, train_ms, args.kernel_only)
    if not (args.kernel_only or args.labeled_only):
        res['kernel_faster_than_torch_at_128'] = all(v['kernel_faster_than_torch'] for v in res['batch128'].values())
        if not args.no_cpu:
            res['cpu'] = measure_cpu(pool_cpu)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
