#!/usr/bin/env python3
"""Measure the ROC histogram kernels and what roc_bits adds to a segment_image pass, on one device.

    python tools/bench_seg_roc.py [--out profiles/seg_roc_mi355x.json] [--shapes 4x1024,32x256] [--bits 11,14]
                                  [--no-slide]

(a) cae_seg_roc_hist (both launches) against the same histogram as torch ops on the device (integer view of the logits,
    shifts, torch.bincount of bin + 2^bits * positive): device time per call by the method of tools/bench_segment_slide.py
    -- events around `--inner` back-to-back calls that cycle through buffer sets of `--footprint-mib` in all, more than
    the 256 MiB Infinity Cache holds, median of 9 groups after 2 warm-up groups, min and max beside it -- for logits that
    are spread (N(0, 3^2)) and concentrated (99 % of the pixels at one value, a slide's background); the bytes that must
    move (5 per pixel in, the int64 table out) over the time as a fraction of 6.3 TB/s.
(b) zarrio.segment_image on a ragged slide of the canonical codec and head with a target: wall time of a pass with
    roc_bits=14 against the same pass without it, `--slide-runs` alternating pairs after one warm-up pair.
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

from bench_segment_slide import HBM_ACHIEVABLE, HEAD, timed_groups  # noqa: E402


def torch_hist(logits, target, bits):
    """the histogram (2, 2^bits) of the batch as torch ops"""
    import torch
    B = 1 << bits
    x = logits.reshape(-1)
    u = (x + 0.0).view(torch.int32)
    key = torch.where(u < 0, ~u, u | -0x80000000)
    b = torch.where(torch.isnan(x), 0, (key >> (32 - bits)) & (B - 1))
    return torch.bincount(b + B * (target.reshape(-1) > 0), minlength=2 * B).view(2, B)


def draw(n, edge, kind, g):
    import torch
    x = 3 * torch.randn(n, 1, edge, edge, generator=g, device='cuda')
    if kind == 'concentrated':
        x = torch.where(torch.rand(x.shape, generator=g, device='cuda') < 0.99, torch.tensor(-6.0, device='cuda'), x)
    return x, (torch.rand(n, edge, edge, generator=g, device='cuda') < 0.2).to(torch.uint8)


def bench_kernel(n, edge, bits, kind, inner, footprint):
    import torch
    from cnn_autoencoder_amd import _lib
    nbytes = n * edge * edge * 5 + 2 * (1 << bits) * 8
    sets = max(2, -(-footprint // nbytes))
    g = torch.Generator(device='cuda').manual_seed(edge + bits)
    L = _lib.lib()
    ws_bytes = int(L.cae_seg_roc_workspace(n, edge, edge, bits))
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device='cuda')
    hist = torch.empty((2, 1 << bits), dtype=torch.int64, device='cuda')
    bufs = [draw(n, edge, kind, g) for _ in range(sets)]
    st = _lib.stream_ptr()
    at = [0]

    def hip():
        logits, target = bufs[at[0] % sets]
        at[0] += 1
        _lib.check(L.cae_seg_roc_hist(logits.data_ptr(), target.data_ptr(), None, n, edge, edge, bits, 0, hist.data_ptr(),
                                      ws.data_ptr(), ws_bytes, st))

    def ops():
        logits, target = bufs[at[0] % sets]
        at[0] += 1
        return torch_hist(logits, target, bits)

    at[0] = 0
    hip()
    at[0] = 0
    same = bool(torch.equal(hist, ops()))
    hip_ms, hip_all = timed_groups(hip, inner)
    torch_ms, torch_all = timed_groups(ops, max(inner // 4, 1))
    return dict(images=n, edge=edge, bits=bits, logits=kind, buffer_sets=sets, blocks_per_image=int(L.cae_seg_roc_blocks(
        n, edge, edge, bits)), workspace_bytes=ws_bytes, hip_ms=hip_ms, hip_min_ms=min(hip_all), hip_max_ms=max(hip_all),
        torch_ms=torch_ms, torch_min_ms=min(torch_all), torch_max_ms=max(torch_all), hip_runs_ms=hip_all,
        torch_runs_ms=torch_all, bytes=nbytes, fraction_of_achievable_hbm=nbytes / (hip_ms * 1e-3) / HBM_ACHIEVABLE,
        faster_than_torch_ops=bool(hip_ms < torch_ms), equal_to_torch_ops=same)


def bench_slide(tiles_y, tiles_x, patch, runs):
    """wall time of segment_image with and without roc_bits=14 on a (tiles_y x tiles_x)-chunk slide whose last row and
    column of chunks are ragged"""
    import numpy as np
    import torch
    from cnn_autoencoder_amd import segmenters, synth, zarrio
    H, W = tiles_y * patch - patch // 3, tiles_x * patch - patch // 5
    img = np.concatenate([np.concatenate([synth.histo_tile(patch, (i * tiles_x + j) % 4) for j in range(tiles_x)], axis=1)
                          for i in range(tiles_y)], axis=0)[:H, :W]
    torch.manual_seed(0)
    seg = segmenters.JNet(**dict(HEAD, num_classes=1)).cuda().eval()
    with tempfile.TemporaryDirectory() as tmp:
        ckpt = os.path.join(tmp, 'ckpt.pth')
        torch.save(synth.synthetic_state(dict(synth.CANONICAL), seed=0), ckpt)
        store = os.path.join(tmp, 'slide.zarr')
        zarrio.compress_image('CAE', ckpt, np.ascontiguousarray(img), store, patch_size=patch, batch_tiles=4)
        labels = (np.random.default_rng(0).random((H, W)) < 0.2).astype(np.uint8)
        zarrio.ZarrArray.create(store, 'labels/0', (H, W), (patch, patch), np.uint8, codec=zarrio.Zlib(1))[:] = labels

        def one(k, roc_bits):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = zarrio.segment_image(store, seg, os.path.join(tmp, f'pred{k}.zarr'), target_group='labels/0',
                                       batch_tiles=4, roc_bits=roc_bits)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        plain, roc, auc = [], [], None
        for r in range(1 + runs):  # alternating, the first pair a warm-up
            tp, _ = one(2 * r, None)
            tr, out = one(2 * r + 1, 14)
            auc = (out['auc'], out['auc_slack'])
            if r:
                plain.append(tp)
                roc.append(tr)
    return dict(image=[H, W], patch=patch, tiles=tiles_y * tiles_x, plain_runs_s=plain, roc_runs_s=roc,
                plain_s=statistics.median(plain), roc_s=statistics.median(roc),
                plain_spread_s=max(plain) - min(plain), added_s=statistics.median(roc) - statistics.median(plain),
                auc=auc[0], auc_slack=auc[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'seg_roc_mi355x.json'))
    ap.add_argument('--shapes', default='4x1024,32x256')
    ap.add_argument('--bits', default='11,14')
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--footprint-mib', type=int, default=768, help='bytes the timed kernel calls cycle through')
    ap.add_argument('--slide', default='6x6x512', help='chunk rows x chunk columns x patch of the segment_image pass')
    ap.add_argument('--slide-runs', type=int, default=3)
    ap.add_argument('--no-slide', action='store_true')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_seg_roc.py measures on a HIP device; none is visible')
    result = dict(device=torch.cuda.get_device_name(0), hbm_achievable=HBM_ACHIEVABLE, kernel=[], slide=None)
    for n, edge in (tuple(map(int, s.split('x'))) for s in a.shapes.split(',')):
        for bits in (int(b) for b in a.bits.split(',')):
            for kind in ('spread', 'concentrated'):
                row = bench_kernel(n, edge, bits, kind, a.inner, a.footprint_mib << 20)
                result['kernel'].append(row)
                print(json.dumps({k: v for k, v in row.items() if not k.endswith('runs_ms')}), flush=True)
                torch.cuda.empty_cache()
    if not a.no_slide:
        result['slide'] = bench_slide(*map(int, a.slide.split('x')), a.slide_runs)
        print(json.dumps(result['slide']), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
