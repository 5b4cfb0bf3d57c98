#!/usr/bin/env python3
"""Reduced-resolution and region decode on the canonical multiscale model (DESIGN "Scaled and region decode").

    python tools/bench_scaled_decode.py --steps K --warmup W [--out FILE] [--no-slide] [--chunk 256] [--grid 16]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_scaled_decode.py --colour-only --steps K

Per arithmetic path (f16x3, fp32) and batch (32 tiles of 1024^2, 256 of 256^2):
  synthesis  device time per batch (HIP events around the call) at scales 0 .. 3, median of the repetitions and their
             spread (min, max); scale 0 is Synthesizer.forward_u8, the unchanged full decode
Then decompress_image of a grid x grid-chunk 'cae' store: whole, one-chunk ROI and a quarter-grid ROI at scales 0 and 2, wall
time and tiles/s.  --colour-only runs, for a kernel trace, forward_scale(s = 1) (color_small_kernel) and Synthesizer.forward
(the generic colour launch inside cae_synthesis_multiscale) on the same latents.  Each mode is one process; run the GPU
steps chained with && and each under its own `timeout`.  Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def canonical_state(seed=0):
    """synth.CANONICAL with multiscale colour layers (seeded; the synthetic state carries none)"""
    from cnn_autoencoder_amd import synth
    cfg = dict(synth.CANONICAL, multiscale_analysis=True)
    state = synth.synthetic_state(cfg, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    k, c_net, c_org = cfg.get('kernel_size', 3), cfg['channels_net'], cfg['channels_org']
    b = synth._xavier_bound(c_net, c_org, k)
    for i in range(cfg['compression_level'] - 1):
        state['decoder'][f'color_layers.{i}.0.weight'] = torch.from_numpy(
            rng.uniform(-b, b, (c_org, c_net, k, k)).astype(np.float32))
    return state


def decoder(state, precision):
    import cnn_autoencoder_amd as cae
    os.environ['CAE_PRECISION'] = precision
    dec = cae.autoencoder_from_state_dict(state)['decoder'].module
    dec.precision = precision
    return dec


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


def measure_synthesis(state, steps, warmup):
    out = {}
    for precision in ('f16x3', 'fp32'):
        dec = decoder(state, precision)
        for n, tile in ((32, 1024), (256, 256)):
            y = torch.round(3.0 * torch.randn(n, 192, tile // 16, tile // 16,
                                              generator=torch.Generator().manual_seed(1))).cuda()
            row = {}
            for s in range(4):
                fn = (lambda: dec.forward_u8(y)) if s == 0 else (lambda s=s: dec.forward_scale_u8(y, s))
                row[f'scale{s}'] = device_ms(fn, steps, warmup)
            for s in (2, 3):
                row[f'scale{s}_faster_than_scale0'] = row[f'scale{s}']['median_ms'] < row['scale0']['median_ms']
            out[f'{precision}_{n}x{tile}'] = row
            print(precision, n, tile, {k: v['median_ms'] for k, v in row.items() if isinstance(v, dict)}, file=sys.stderr)
    return out


def measure_slide(state, steps, chunk, grid):
    from cnn_autoencoder_amd import synth, zarrio
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'ckpt.pth')
        torch.save(state, path)
        tiles = [synth.histo_tile(chunk, i) for i in range(8)]
        image = np.concatenate([np.concatenate([tiles[(i + j) % 8] for j in range(grid)], 1) for i in range(grid)], 0)
        store = os.path.join(tmp, 'slide.zarr')
        zarrio.compress_image('CAE', path, image, store, patch_size=chunk)
        q = grid // 4
        rois = {'whole': (None, grid * grid), 'one_chunk': ((chunk, 2 * chunk, chunk, 2 * chunk), 1),
                'quarter_grid': ((chunk, (1 + q) * chunk, chunk, (1 + q) * chunk), q * q)}
        for name, (roi, n_tiles) in rois.items():
            for s in (0, 2):
                zarrio.decompress_image(store, roi=roi, scale=s)  # warm-up: model build, workspaces, pinned buffers
                wall = []
                for _ in range(steps):
                    t0 = time.perf_counter()
                    zarrio.decompress_image(store, roi=roi, scale=s)
                    wall.append(time.perf_counter() - t0)
                med = statistics.median(wall)
                out[f'{name}_scale{s}'] = dict(tiles=n_tiles, median_s=med, min_s=min(wall), max_s=max(wall),
                                               tiles_per_s=n_tiles / med)
    return out


def colour_only(state, steps):
    for precision in ('f16x3', 'fp32'):
        dec = decoder(state, precision)
        y = torch.round(3.0 * torch.randn(32, 192, 64, 64, generator=torch.Generator().manual_seed(1))).cuda()
        for _ in range(steps):
            dec.forward_scale(y, 1)
            dec(y, bridges=False)
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out')
    ap.add_argument('--no-slide', action='store_true')
    ap.add_argument('--no-synthesis', action='store_true')
    ap.add_argument('--colour-only', action='store_true')
    ap.add_argument('--chunk', type=int, default=256)
    ap.add_argument('--grid', type=int, default=16)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark measures an MI355X; there is no CPU path'
    state = canonical_state()
    if args.colour_only:
        colour_only(state, args.steps)
        return
    res = dict(device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup)
    if not args.no_synthesis:
        res['synthesis'] = measure_synthesis(state, args.steps, args.warmup)
    if not args.no_slide:
        res['slide'] = dict(chunk=args.chunk, grid=args.grid, **measure_slide(state, max(3, args.steps // 2), args.chunk,
                                                                              args.grid))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
