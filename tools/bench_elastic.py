#!/usr/bin/env python3
"""Measure the elastic deformation (csrc/cae_elastic.hip) beside the step it follows, the host form it replaces and the
training step it feeds, on one device.

    python tools/bench_elastic.py [--out profiles/elastic/mi355x.json] [--shapes 128x3x128x1,16x3x256x1,32x3x256x1,128x3x256x0]

For every shape (patches x image channels x edge x mask channels; masks hold 0 / 1, displacements are N(0, 10^2)):
  device: cae_t_elastic_deform, timed by the method of the other bench tools: events around `--inner` back-to-back calls
          that cycle through buffer sets of `--footprint-mib` in all, median of 9 groups after 2 warm-up groups, min and
          max beside it;
  rate:   the stream floor 8 n (c + kt) ps^2 bytes (every value read once and written once) over that time;
  gather: LabeledPatchSampler.gather (PatchSampler.gather for a shape without masks) of a batch of the same shape with
          rotation on: the step the deformation follows, timed the same way;
  host:   the same contract the reference's way, per patch and channel on `--host-workers` worker processes (as a data
          loader's workers): scipy.ndimage.map_coordinates(order=3, mode='mirror') for the field, spline_filter +
          map_coordinates(order=3, mode='reflect') per image plane and map_coordinates(order=0) per mask plane; wall time
          of the whole batch, median of 3 after one warm-up.  The device result of the batch is compared with it;
  step:   for 256^2 shapes with masks, forward + backward + optimiser of the canonical segmentation head at the same batch
          (tools/bench_segmenter_train.measure, in this process and visit) and the call's share of it.
The one condition: the device call takes less time per batch than the host form.  The tool exits with status 1 where it
does not.  Every GPU step runs under its own time limit (`--step-limit` seconds): when one runs out, the process ends there
with a traceback and starts nothing more.
"""
import argparse
import contextlib
import faulthandler
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

SIGMA = 10.0


@contextlib.contextmanager
def limited(seconds):
    """ends the process (with every thread's traceback) if the block takes longer, even inside a blocking device call"""
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def host_sample(job):
    """one patch the reference's way: (x [c, ps, ps], t [kt, ps, ps] or None, d [2, 3, 3]) -> (x', t'); a worker process"""
    import numpy as np
    from scipy import ndimage
    x, t, d = job
    ps = x.shape[-1]
    u = 2.0 * np.arange(ps) / (ps - 1)
    grid = np.meshgrid(u, u, indexing='ij')
    i, j = np.meshgrid(np.arange(ps, dtype=np.float64), np.arange(ps, dtype=np.float64), indexing='ij')
    at = [np.clip(i + ndimage.map_coordinates(d[0], grid, order=3, mode='mirror'), -ps, 2 * ps),
          np.clip(j + ndimage.map_coordinates(d[1], grid, order=3, mode='mirror'), -ps, 2 * ps)]
    xo = np.stack([ndimage.map_coordinates(ndimage.spline_filter(p, order=3, mode='reflect'), at, order=3, mode='reflect',
                                           prefilter=False) for p in x])
    to = None if t is None else np.stack([ndimage.map_coordinates(p, at, order=0, mode='reflect') for p in t])
    return xo.astype(np.float32), to


def bench_case(n, c, ps, kt, inner, footprint, pool, limit):
    import numpy as np
    import torch
    from bench_segment_slide import timed_groups
    from cnn_autoencoder_amd import _lib
    from cnn_autoencoder_amd.sampler import LabeledPatchSampler, PatchSampler, elastic_coefficients, elastic_deform
    L, st = _lib.lib(), _lib.stream_ptr()
    plane = ps * ps
    ws_bytes = int(L.cae_t_elastic_deform_workspace(n, c, ps))
    floor_bytes = 8 * n * (c + kt) * plane
    sets = max(2, min(32, footprint // (floor_bytes + ws_bytes)))
    g = torch.Generator().manual_seed(ps + n)
    disp = torch.randn(n, 2, 3, 3, generator=g, dtype=torch.float64) * SIGMA
    coef = torch.from_numpy(elastic_coefficients(disp.numpy()).astype(np.float32)).cuda()
    x = [torch.rand(n, c, ps, ps, generator=g).mul_(2).sub_(1).cuda() for _ in range(sets)]
    t = [torch.randint(0, 2, (n, kt, ps, ps), generator=g).float().cuda() for _ in range(sets)] if kt else None
    xo = [torch.empty_like(v) for v in x]
    to = [torch.empty_like(v) for v in t] if kt else None
    ws = [torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device='cuda') for _ in range(sets)]
    at = [0]

    def call():
        k = at[0] % sets
        at[0] += 1
        _lib.check(L.cae_t_elastic_deform(x[k].data_ptr(), t[k].data_ptr() if kt else None, coef.data_ptr(), n, c, kt, ps,
                                          ws[k].data_ptr() if ws_bytes else None, ws_bytes, xo[k].data_ptr(),
                                          to[k].data_ptr() if kt else None, st))

    row = dict(patches=n, channels=c, edge=ps, mask_channels=kt, path='lds' if ps <= 128 else 'global', buffer_sets=sets,
               workspace_bytes=ws_bytes, stream_floor_bytes=floor_bytes)
    with limited(limit):
        ms, runs = timed_groups(call, inner)
    row.update(device_ms=ms, device_min_ms=min(runs), device_max_ms=max(runs), device_runs_ms=runs,
               bytes_per_s_against_floor=floor_bytes / (ms * 1e-3))

    # the step the deformation follows: a rotated batch of the same shape
    tiles = torch.randint(0, 256, (2, ps + 64, ps + 64, c), dtype=torch.uint8, generator=g).cuda()
    if kt:
        labels = torch.randint(0, 2, (2, ps + 64, ps + 64, kt), dtype=torch.uint8, generator=g).cuda()
        sampler = LabeledPatchSampler(tiles, labels, ps, rotation=True, batch_size=n)
    else:
        sampler = PatchSampler(tiles, ps, rotation=True, batch_size=n)
    draw = sampler.draw(n, torch.Generator().manual_seed(ps))
    with limited(limit):
        ms, runs = timed_groups(lambda: sampler.gather(*draw), inner)
    row.update(gather_ms=ms, gather_min_ms=min(runs), gather_max_ms=max(runs), gather_runs_ms=runs,
               device_over_gather=row['device_ms'] / ms)

    # the host form, the reference's way, on the worker processes
    xh, th, dh = x[0].cpu().numpy(), t[0].cpu().numpy() if kt else None, disp.numpy()
    jobs = [(xh[s], th[s] if kt else None, dh[s]) for s in range(n)]
    wall = []
    for _ in range(4):
        t0 = time.perf_counter()
        host = pool.map(host_sample, jobs, chunksize=1)
        wall.append((time.perf_counter() - t0) * 1e3)
    row.update(host_ms=statistics.median(wall[1:]), host_runs_ms=wall[1:])
    row['host_over_device'] = row['host_ms'] / row['device_ms']
    with limited(limit):
        got = elastic_deform(x[0], disp, t[0] if kt else None)
        gx, gt = got if kt else (got, None)
        row['max_abs_difference_to_host'] = float(np.abs(gx.cpu().numpy() - np.stack([h[0] for h in host])).max())
        if kt:
            row['mask_pixels_equal_to_host'] = float((gt.cpu().numpy() == np.stack([h[1] for h in host])).mean())
    return row


def head_step(n, edge, limit):
    import torch
    from bench_segmenter_train import measure
    with limited(limit):
        m = measure(n, edge, False)
    torch.cuda.empty_cache()
    return dict(forward_backward_ms=m['forward_backward_ms'], optimiser_ms=m['optimiser_ms'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'elastic', 'mi355x.json'))
    ap.add_argument('--shapes', default='128x3x128x1,16x3x256x1,32x3x256x1,128x3x256x0')
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--footprint-mib', type=int, default=768, help='bytes the timed kernel calls cycle through')
    ap.add_argument('--host-workers', type=int, default=16)
    ap.add_argument('--step-limit', type=int, default=120, help='seconds a GPU step may take')
    ap.add_argument('--no-head', action='store_true', help='leave out the head training step')
    a = ap.parse_args()
    import multiprocessing
    # fresh worker processes, started before this process opens the device; they never import torch
    pool = multiprocessing.get_context('spawn').Pool(a.host_workers)
    import torch
    if not torch.cuda.is_available():
        pool.terminate()
        raise SystemExit('bench_elastic.py measures on a HIP device; none is visible')
    result = dict(device=torch.cuda.get_device_name(0), sigma=SIGMA, host_workers=a.host_workers, cases=[])
    ok = True
    try:
        for n, c, ps, kt in (tuple(map(int, s.split('x'))) for s in a.shapes.split(',')):
            row = bench_case(n, c, ps, kt, a.inner, a.footprint_mib << 20, pool, a.step_limit)
            torch.cuda.empty_cache()
            if ps == 256 and kt and not a.no_head:
                row['head_step'] = head_step(n, ps, a.step_limit)
                step_ms = row['head_step']['forward_backward_ms'] + row['head_step']['optimiser_ms']
                row['share_of_head_step'] = row['device_ms'] / step_ms
            row['faster_than_host'] = row['device_ms'] < row['host_ms']
            ok = ok and row['faster_than_host']
            result['cases'].append(row)
            print(json.dumps({k: v for k, v in row.items() if not k.endswith('runs_ms')}), flush=True)
    finally:
        pool.terminate()
        pool.join()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
    print('wrote', a.out)
    if not ok:
        raise SystemExit(1)


if __name__ == '__main__':
    main()
