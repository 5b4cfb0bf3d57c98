#!/usr/bin/env python3
"""Measure the tile histogram kernel and what skipping background tiles does to a slide pass, on one device.

    python tools/bench_sparse.py [--out profiles/sparse_mi355x.json] [--shapes 32x512,8x1024] [--slide 16x16x512]
                                 [--no-slide]

(a) cae_tile_byte_hist (both launches) against the same histograms as torch ops on the device (torch.bincount of
    tile * 256 + value): device time per call by the method of tools/bench_seg_roc.py -- events around `--inner`
    back-to-back calls that cycle through buffer sets of `--footprint-mib` in all, more than the 256 MiB Infinity Cache
    holds, median of 9 groups after 2 warm-up groups, min and max beside it -- for bytes that are spread (uniform) and
    concentrated (99 % at one value, a slide's background); the bytes that must move (the tiles in, the int64 tables
    out) over the time as a fraction of 6.3 TB/s.
(b) zarrio.compress_image and decompress_image on a synthetic slide of `histo` tissue tiles in a background of 240 +- 2,
    with a hand-made mask at 1 / 32 that keeps about a tenth of the chunks: wall time per pass of the dense call (no new
    argument), the sparse call with the guard (max_fill_rmse; pass 1 looks at every candidate) and the sparse call
    without it and with a given fill value (no pass 1), `--slide-runs` alternating triples after one warm-up triple.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_segment_slide import HBM_ACHIEVABLE, timed_groups  # noqa: E402


def torch_hist(tiles):
    """the histograms (n, 256) of the batch as torch ops"""
    import torch
    n = tiles.shape[0]
    key = tiles.reshape(n, -1).to(torch.int32) + 256 * torch.arange(n, dtype=torch.int32, device=tiles.device)[:, None]
    return torch.bincount(key.reshape(-1), minlength=256 * n).view(n, 256)


def draw(n, edge, kind, g):
    import torch
    x = torch.randint(0, 256, (n, edge, edge, 3), generator=g, device='cuda', dtype=torch.uint8)
    if kind == 'concentrated':
        x = torch.where(torch.rand(x.shape, generator=g, device='cuda') < 0.99, torch.tensor(238, dtype=torch.uint8, device='cuda'), x)
    return x


def bench_kernel(n, edge, kind, inner, footprint):
    import torch
    from cnn_autoencoder_amd import _lib
    nbytes = n * edge * edge * 3 + n * 256 * 8
    sets = max(2, -(-footprint // nbytes))
    g = torch.Generator(device='cuda').manual_seed(edge + n)
    L = _lib.lib()
    ws_bytes = int(L.cae_tile_byte_hist_workspace(n, edge, edge, 3))
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device='cuda')
    hist = torch.empty((n, 256), dtype=torch.int64, device='cuda')
    bufs = [draw(n, edge, kind, g) for _ in range(sets)]
    st = _lib.stream_ptr()
    at = [0]

    def hip():
        tiles = bufs[at[0] % sets]
        at[0] += 1
        _lib.check(L.cae_tile_byte_hist(tiles.data_ptr(), None, n, edge, edge, 3, hist.data_ptr(), ws.data_ptr(), ws_bytes, st))

    def ops():
        tiles = bufs[at[0] % sets]
        at[0] += 1
        return torch_hist(tiles)

    at[0] = 0
    hip()
    at[0] = 0
    same = bool(torch.equal(hist, ops()))
    hip_ms, hip_all = timed_groups(hip, inner)
    torch_ms, torch_all = timed_groups(ops, max(inner // 4, 1))
    return dict(tiles=n, edge=edge, bytes_kind=kind, buffer_sets=sets, blocks_per_tile=int(L.cae_tile_byte_hist_blocks(
        n, edge, edge, 3)), workspace_bytes=ws_bytes, hip_ms=hip_ms, hip_min_ms=min(hip_all), hip_max_ms=max(hip_all),
        torch_ms=torch_ms, torch_min_ms=min(torch_all), torch_max_ms=max(torch_all), hip_runs_ms=hip_all,
        torch_runs_ms=torch_all, bytes=nbytes, fraction_of_achievable_hbm=nbytes / (hip_ms * 1e-3) / HBM_ACHIEVABLE,
        faster_than_torch_ops=bool(hip_ms < torch_ms), equal_to_torch_ops=same)


def slide_image(tiles_y, tiles_x, patch):
    """-> (image, mask at 1 / 32, chunks kept): tissue tiles in a block of about a tenth of the chunks, the rest 240 +- 2"""
    import numpy as np
    from cnn_autoencoder_amd import synth
    rng = np.random.default_rng(0)
    img = (240 + rng.integers(-2, 3, (tiles_y * patch, tiles_x * patch, 3), dtype=np.int16)).astype(np.uint8)
    side_y = max(1, round((tiles_y * tiles_x / 10) ** 0.5))
    side_x = max(1, round(tiles_y * tiles_x / 10 / side_y))
    y0, x0 = (tiles_y - side_y) // 2, (tiles_x - side_x) // 2
    f = patch // 32
    mask = np.zeros((tiles_y * f, tiles_x * f), dtype=bool)
    for i in range(y0, y0 + side_y):
        for j in range(x0, x0 + side_x):
            img[i * patch:(i + 1) * patch, j * patch:(j + 1) * patch] = synth.histo_tile(patch, i * tiles_x + j)
            mask[i * f:(i + 1) * f, j * f:(j + 1) * f] = True
    return img, mask, side_y * side_x


def bench_slide(tiles_y, tiles_x, patch, runs, guard):
    import numpy as np
    import torch
    from cnn_autoencoder_amd import synth, zarrio
    img, mask, kept = slide_image(tiles_y, tiles_x, patch)
    modes = dict(dense={}, sparse_guard=dict(mask=mask, mask_scale=1 / 32, max_fill_rmse=guard),
                 sparse=dict(mask=mask, mask_scale=1 / 32, fill_value=240))  # (no guard, a given value: no pass 1)
    times = {f'{m}_{what}': [] for m in modes for what in ('compress', 'decompress')}
    accounts = {}
    with tempfile.TemporaryDirectory() as tmp:
        ckpt = os.path.join(tmp, 'ckpt.pth')
        torch.save(synth.synthetic_state(dict(synth.CANONICAL), seed=0), ckpt)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        recs = {}
        for r in range(1 + runs):  # alternating, the first triple a warm-up
            for m, kw in modes.items():
                store = os.path.join(tmp, f'{m}_{r}.zarr')
                tc, z = timed(lambda: zarrio.compress_image('CAE', ckpt, img, store, patch_size=patch, **kw))
                td, recs[m] = timed(lambda: zarrio.decompress_image(store))
                accounts[m] = z.attrs.get('sparse')
                if r:
                    times[f'{m}_compress'].append(tc)
                    times[f'{m}_decompress'].append(td)
        # the sparse reads are the dense read where a chunk was coded and the fill value elsewhere
        same = bool(np.array_equal(recs['sparse'], recs['sparse_guard']))
    med = {k: statistics.median(v) for k, v in times.items()}
    return dict(image=list(img.shape), patch=patch, tiles=tiles_y * tiles_x, kept=kept, guard_rmse=guard, runs_s=times,
                median_s=med, accounts=accounts, sparse_reads_agree=same,
                compress_dense_over_sparse_guard=med['dense_compress'] / med['sparse_guard_compress'],
                compress_dense_over_sparse=med['dense_compress'] / med['sparse_compress'],
                decompress_dense_over_sparse=med['dense_decompress'] / med['sparse_decompress'],
                sparse_guard_faster_than_dense=bool(med['sparse_guard_compress'] < med['dense_compress']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sparse_mi355x.json'))
    ap.add_argument('--shapes', default='32x512,8x1024')
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--footprint-mib', type=int, default=768, help='bytes the timed kernel calls cycle through')
    ap.add_argument('--slide', default='16x16x512', help='chunk rows x chunk columns x patch of the slide passes')
    ap.add_argument('--slide-runs', type=int, default=3)
    ap.add_argument('--guard', type=float, default=4.0, help='max_fill_rmse of the guarded pass')
    ap.add_argument('--no-slide', action='store_true')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_sparse.py measures on a HIP device; none is visible')
    result = dict(device=torch.cuda.get_device_name(0), hbm_achievable=HBM_ACHIEVABLE, kernel=[], slide=None)
    for n, edge in (tuple(map(int, s.split('x'))) for s in a.shapes.split(',')):
        for kind in ('spread', 'concentrated'):
            row = bench_kernel(n, edge, kind, a.inner, a.footprint_mib << 20)
            result['kernel'].append(row)
            print(json.dumps({k: v for k, v in row.items() if not k.endswith('runs_ms')}), flush=True)
            torch.cuda.empty_cache()
    if not a.no_slide:
        result['slide'] = bench_slide(*map(int, a.slide.split('x')), a.slide_runs, a.guard)
        print(json.dumps({k: v for k, v in result['slide'].items() if k != 'runs_s'}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
