#!/usr/bin/env python3
"""Measure the object-level entry points (csrc/cae_seg_objects.hip) against the host route they replace, on one device.

    python tools/bench_seg_objects.py [--out profiles/seg_objects_mi355x.json] [--shapes 4x1024,32x256] [--no-head]

For every shape (label planes per batch x edge) and label pattern -- 'nuclei': sparse blobs of 4 to 9 pixels radius on
about a tenth of the plane; 'tissue': one large region with holes; 'bernoulli': independent pixels at density 0.4 --
  device: cae_seg_components, cae_seg_object_cover, cae_seg_object_counts and cae_seg_object_roc_hist (14 bits), each
          timed by the method of tools/bench_seg_roc.py: events around `--inner` back-to-back calls that cycle through
          buffer sets of `--footprint-mib` in all, median of 9 groups after 2 warm-up groups, min and max beside it;
  host:   what a caller without them does per batch -- labels and logits to the host, scipy.ndimage.label (3x3
          structure) and find_objects per plane, the cover from the boxes' corners and two cumulative sums, the weighted
          confusion sums and the weighted histogram in numpy -- with the planes of a batch spread over 16 threads; wall
          time, median of 9 runs after 2 warm-ups.
The two routes are compared once per case (object numbers, cover, record, histogram) before anything is timed.
Unless --no-head, the canonical head's device time per batch of 4 x 1024^2 (cae_seg_forward through JNet.forward) is
measured in the same run, and the added device time per batch is given as a fraction of it.
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_segment_slide import HEAD, timed_groups  # noqa: E402

PATTERNS = ('nuclei', 'tissue', 'bernoulli')
HOST_THREADS = 16
BITS = 14


def host_plane(kind, edge, seed):
    """one (edge, edge) uint8 label plane"""
    import numpy as np
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:edge, 0:edge]

    def discs(count, r0, r1):
        out = np.zeros((edge, edge), dtype=bool)
        for _ in range(count):
            r, cy, cx = (int(v) for v in (rng.integers(r0, r1 + 1), rng.integers(0, edge), rng.integers(0, edge)))
            ys, xs = slice(max(cy - r, 0), cy + r + 1), slice(max(cx - r, 0), cx + r + 1)
            out[ys, xs] |= (yy[ys, xs] - cy) ** 2 + (xx[ys, xs] - cx) ** 2 <= r * r
        return out

    if kind == 'nuclei':
        return discs(max(edge * edge // 1400, 1), 4, 9).astype(np.uint8)
    if kind == 'tissue':
        c, a, b = edge / 2.0, 0.45 * edge, 0.38 * edge
        region = ((yy - c) / a) ** 2 + ((xx - c) / b) ** 2 <= 1.0
        return (region & ~discs(max(edge * edge // 6000, 1), 5, 20)).astype(np.uint8)
    assert kind == 'bernoulli', kind
    return (rng.random((edge, edge)) < 0.4).astype(np.uint8)


def make_sets(kind, n, edge, sets):
    """`sets` buffer sets of (target (n,edge,edge) uint8, logits (n,1,edge,edge) fp32) on the device: eight planes drawn
    on the host, rolled by random offsets"""
    import numpy as np
    import torch
    base = [torch.from_numpy(host_plane(kind, edge, 100 + i)).cuda() for i in range(8)]
    rng = np.random.default_rng(edge + n)
    g = torch.Generator(device='cuda').manual_seed(edge + n)
    out = []
    for _ in range(sets):
        planes = [torch.roll(base[int(rng.integers(0, 8))], (int(rng.integers(0, edge)), int(rng.integers(0, edge))), (0, 1))
                  for _ in range(n)]
        target = torch.stack(planes).contiguous()
        # a head that is mostly right: positive logits on the objects
        logits = 2.0 * torch.randn(n, 1, edge, edge, generator=g, device='cuda') + 3.0 * (target[:, None].float() * 2 - 1)
        out.append((target, logits.contiguous()))
    return out


def host_route(target, logits, t, pool):
    """-> (n_objects (n,), cover (n,h,w) int64, record (n,6), hist (2, 2^BITS)) in numpy, from device tensors"""
    import numpy as np
    from scipy import ndimage
    tg, lg = target.cpu().numpy(), logits.cpu().numpy()
    n, h, w = tg.shape
    eight = np.ones((3, 3), dtype=np.int64)

    def one(i):
        lab, count = ndimage.label(tg[i] > 0, structure=eight)
        sl = ndimage.find_objects(lab)
        y0 = np.maximum(np.array([s[0].start for s in sl], dtype=np.int64) - 1, 0)
        y1 = np.minimum(np.array([s[0].stop for s in sl], dtype=np.int64) + 1, h)
        x0 = np.maximum(np.array([s[1].start for s in sl], dtype=np.int64) - 1, 0)
        x1 = np.minimum(np.array([s[1].stop for s in sl], dtype=np.int64) + 1, w)
        d = np.zeros((h + 1, w + 1), dtype=np.int64)
        np.add.at(d, (y0, x0), 1)
        np.add.at(d, (y0, x1), -1)
        np.add.at(d, (y1, x0), -1)
        np.add.at(d, (y1, x1), 1)
        cover = d.cumsum(axis=0).cumsum(axis=1)[:h, :w]
        x = lg[i, 0]
        on, pos = x > t, tg[i] > 0
        tp, tn = cover[on & pos].sum(), cover[~on & ~pos].sum()
        fp, fn = cover[on & ~pos].sum(), cover[~on & pos].sum()
        u = (x + np.float32(0.0)).view(np.uint32)
        key = np.where(u >> np.uint32(31), ~u, u | np.uint32(0x80000000))
        b = np.where(np.isnan(x), 0, key >> np.uint32(32 - BITS)).astype(np.int64) + (pos.astype(np.int64) << BITS)
        hist = np.bincount(b.reshape(-1), weights=cover.reshape(-1), minlength=2 << BITS).astype(np.int64)
        return count, cover, np.array([tp, tn, fp, fn, tp + fn, tp], dtype=np.int64), hist.reshape(2, 1 << BITS)

    parts = list(pool.map(one, range(n)))
    return (np.array([p[0] for p in parts]), np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts]),
            sum(p[3] for p in parts))


def wall_ms(fn, runs=9, warm=2):
    import torch
    out = []
    for r in range(warm + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warm:
            out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), out


def bench_case(kind, n, edge, inner, footprint, pool):
    import numpy as np
    import torch
    from cnn_autoencoder_amd import _lib
    L = _lib.lib()
    st = _lib.stream_ptr()
    hw = edge * edge
    sets = max(2, min(48, -(-footprint // (n * hw * 11))))  # 1 + 4 + 2 + 4 bytes per pixel pass through the four calls
    bufs = make_sets(kind, n, edge, sets)
    i64 = lambda nbytes: torch.empty(max(int(nbytes) // 8, 1), dtype=torch.int64, device='cuda')  # noqa: E731
    labels = [torch.empty((n, edge, edge), dtype=torch.int32, device='cuda') for _ in range(sets)]
    covers = [torch.empty((n, edge, edge), dtype=torch.uint16, device='cuda') for _ in range(sets)]
    count = torch.empty((n,), dtype=torch.int64, device='cuda')
    record = torch.empty((n, 6), dtype=torch.int64, device='cuda')
    hist = torch.empty((2, 1 << BITS), dtype=torch.int64, device='cuda')
    ws = {k: i64(v) for k, v in (('components', L.cae_seg_components_workspace(n, edge, edge)),
                                 ('cover', L.cae_seg_object_cover_workspace(n, edge, edge)),
                                 ('counts', L.cae_seg_object_counts_workspace(n, 1, hw)),
                                 ('hist', L.cae_seg_object_roc_workspace(n, edge, edge, BITS)))}
    at = [0]

    def nxt():
        k = at[0] % sets
        at[0] += 1
        return k

    def components():
        k = nxt()
        _lib.check(L.cae_seg_components(bufs[k][0].data_ptr(), None, n, edge, edge, 0, labels[k].data_ptr(), count.data_ptr(),
                                        ws['components'].data_ptr(), ws['components'].numel() * 8, st))

    def cover():
        k = nxt()
        _lib.check(L.cae_seg_object_cover(labels[k].data_ptr(), None, n, edge, edge, covers[k].data_ptr(),
                                          ws['cover'].data_ptr(), ws['cover'].numel() * 8, st))

    def counts():
        k = nxt()
        _lib.check(L.cae_seg_object_counts(bufs[k][1].data_ptr(), bufs[k][0].data_ptr(), covers[k].data_ptr(), n, 1, hw, 0.0,
                                           5, record.data_ptr(), ws['counts'].data_ptr(), ws['counts'].numel() * 8, st))

    def histogram():
        k = nxt()
        _lib.check(L.cae_seg_object_roc_hist(bufs[k][1].data_ptr(), bufs[k][0].data_ptr(), covers[k].data_ptr(), None, n,
                                             edge, edge, BITS, 0, hist.data_ptr(), ws['hist'].data_ptr(),
                                             ws['hist'].numel() * 8, st))

    # every set labelled and covered once (the later entry points read these), and the two routes compared on set 0
    for fn in (components, cover):
        at[0] = 0
        for _ in range(sets):
            fn()
    for fn in (components, counts, histogram):  # set 0 last: count, record and hist are its
        at[0] = 0
        fn()
    torch.cuda.synchronize()
    h_count, h_cover, h_record, h_hist = host_route(bufs[0][0], bufs[0][1], np.float32(0), pool)
    same = bool(np.array_equal(count.cpu().numpy(), h_count) and np.array_equal(covers[0].cpu().numpy(), h_cover)
                and np.array_equal(record.cpu().numpy(), h_record) and np.array_equal(hist.cpu().numpy(), h_hist))
    row = dict(pattern=kind, planes=n, edge=edge, buffer_sets=sets, objects_per_plane=float(h_count.mean()),
               foreground=float((bufs[0][0] > 0).float().mean()), max_cover=int(h_cover.max()), equal_to_host_route=same,
               workspace_bytes={k: v.numel() * 8 for k, v in ws.items()})
    total = 0.0
    for name, fn in (('components', components), ('cover', cover), ('counts', counts), ('hist', histogram)):
        ms, runs = timed_groups(fn, inner)
        row[name + '_ms'], row[name + '_min_ms'], row[name + '_max_ms'], row[name + '_runs_ms'] = ms, min(runs), max(runs), runs
        total += ms
    row['device_ms'] = total
    at[0] = 0
    host_ms, host_runs = wall_ms(lambda: host_route(*bufs[nxt()], np.float32(0), pool))
    row.update(host_ms=host_ms, host_min_ms=min(host_runs), host_max_ms=max(host_runs), host_runs_ms=host_runs,
               host_threads=HOST_THREADS, device_faster_than_host=bool(total < host_ms))
    return row


def bench_head(n, edge, inner):
    """device time of the canonical head on a batch of n tiles of edge^2 pixels, ms per batch"""
    import torch
    import cnn_autoencoder_amd as cae
    from cnn_autoencoder_amd import segmenters, synth
    from cnn_autoencoder_amd.codec import _module
    codec = cae.ConvolutionalAutoencoder(checkpoint=synth.synthetic_state(dict(synth.CANONICAL), seed=0))
    dec = _module(codec._model['decoder'])
    torch.manual_seed(0)
    seg = segmenters.JNet(**dict(HEAD, num_classes=1)).cuda().eval()
    down = 2 ** len(dec.synthesis_track)
    with torch.no_grad():
        y_q = torch.round(2.0 * torch.randn(n, HEAD['channels_bn'], edge // down, edge // down, device='cuda'))
        _, brg = dec(y_q)
        ms, runs = timed_groups(lambda: seg(y_q, fx_brg=brg), inner)
    return dict(planes=n, edge=edge, head_ms=ms, head_min_ms=min(runs), head_max_ms=max(runs), head_runs_ms=runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'seg_objects_mi355x.json'))
    ap.add_argument('--shapes', default='4x1024,32x256')
    ap.add_argument('--patterns', default=','.join(PATTERNS))
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--footprint-mib', type=int, default=768, help='bytes the timed kernel calls cycle through')
    ap.add_argument('--no-head', action='store_true')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_seg_objects.py measures on a HIP device; none is visible')
    result = dict(device=torch.cuda.get_device_name(0), bits=BITS, host_threads=HOST_THREADS, head=None, cases=[])
    if not a.no_head:
        result['head'] = bench_head(4, 1024, 5)
        print(json.dumps({k: v for k, v in result['head'].items() if not k.endswith('runs_ms')}), flush=True)
        torch.cuda.empty_cache()
    with ThreadPoolExecutor(max_workers=HOST_THREADS) as pool:
        for n, edge in (tuple(map(int, s.split('x'))) for s in a.shapes.split(',')):
            for kind in a.patterns.split(','):
                row = bench_case(kind, n, edge, a.inner, a.footprint_mib << 20, pool)
                if result['head'] is not None:
                    # per batch of the head's 4 x 1024^2 pixels
                    per_batch = row['device_ms'] * (4 * 1024 * 1024) / (n * edge * edge)
                    row['device_share_of_head'] = per_batch / result['head']['head_ms']
                result['cases'].append(row)
                print(json.dumps({k: v for k, v in row.items() if not k.endswith('runs_ms')}), flush=True)
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
