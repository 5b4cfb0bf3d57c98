#!/usr/bin/env python3
"""Measure the border weight map (csrc/cae_seg_distances.hip) beside the step it joins and the host procedure it
replaces, on one device.

    python tools/bench_weight_map.py [--out profiles/weight_map/mi355x.json] [--shapes 16x256,4x1024] [--objects 10,100,1000]

For every shape (label planes per batch x edge) and blob mask of about the given number of objects per plane
(Gaussian-filtered noise thresholded at a fifth of the plane, the filter's width searched for the object count):
  device: cae_seg_components, cae_seg_object_distances and cae_seg_weight_map, each timed by the method of
          tools/bench_seg_objects.py: events around `--inner` back-to-back calls that cycle through buffer sets of
          `--footprint-mib` in all, median of 9 groups after 2 warm-up groups, min and max beside it;
  rate:   the row pass evaluates planes x edge^2 x edge x 2 candidates; over the time of the whole distances call (the
          column pass included: a lower bound of the row pass's own rate);
  gather: LabeledPatchSampler.gather of a batch of the same shape with rotation on, without the weight-map keywords: the
          step the map joins, timed the same way;
  host:   sampler.WeightsDistances(force_torch=True), the reference's procedure (scipy.ndimage.label and one
          distance_transform_edt per object), wall time of one plane of the batch times the planes (one run: it takes
          seconds to minutes).
The device map of that plane is compared with the host procedure's in the same run (largest difference, labels equal).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_segment_slide import timed_groups  # noqa: E402

CLASS_WEIGHTS, SIGMA, W_0 = [1.0, 2.0], 5, 10


def blob_plane(edge, objects, seed):
    """one (edge, edge) uint8 mask of about `objects` 8-connected objects on a fifth of the plane -> (mask, count)"""
    import numpy as np
    from scipy import ndimage
    noise = np.random.default_rng(seed).standard_normal((edge, edge))
    eight = np.ones((3, 3))

    def at(width):
        f = ndimage.gaussian_filter(noise, width, mode='wrap')
        mask = f > np.quantile(f, 0.8)
        return mask.astype(np.uint8), ndimage.label(mask, structure=eight)[1]

    lo, hi = 0.5, edge / 4.0  # narrow filters leave many objects, wide ones few
    best = at(lo)
    for _ in range(12):
        mid = (lo * hi) ** 0.5
        cand = at(mid)
        if abs(cand[1] - objects) < abs(best[1] - objects):
            best = cand
        if cand[1] > objects:
            lo = mid
        else:
            hi = mid
    return best


def bench_case(n, edge, objects, inner, footprint, host):
    import numpy as np
    import torch
    from cnn_autoencoder_amd import _lib
    from cnn_autoencoder_amd.sampler import LabeledPatchSampler, WeightsDistances
    L = _lib.lib()
    st = _lib.stream_ptr()
    hw = edge * edge
    base = [blob_plane(edge, objects, 100 * objects + i) for i in range(2)]
    sets = max(2, min(32, -(-footprint // (n * hw * 33))))  # 1 + 4 + 8 + 4 + 8 bytes per pixel written, 16 of workspace
    rng = np.random.default_rng(edge + n)
    targets = []
    for k in range(sets):
        planes = [torch.roll(torch.from_numpy(base[(k + i) % 2][0]).cuda(),
                             (int(rng.integers(0, edge)), int(rng.integers(0, edge))), (0, 1)) for i in range(n)]
        if k == 0:
            planes[0] = torch.from_numpy(base[0][0]).cuda()  # the plane the host procedure gets
        targets.append(torch.stack(planes).contiguous())
    floats = [t.float() for t in targets]
    labels = [torch.empty((n, edge, edge), dtype=torch.int32, device='cuda') for _ in range(sets)]
    d2 = [torch.empty((n, 2, edge, edge), dtype=torch.int32, device='cuda') for _ in range(sets)]
    out = [torch.empty((n, 2, edge, edge), dtype=torch.float32, device='cuda') for _ in range(sets)]
    counts = [torch.empty((n,), dtype=torch.int64, device='cuda') for _ in range(sets)]
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    cw = torch.tensor(CLASS_WEIGHTS, dtype=torch.float32, device='cuda')
    i64 = lambda nbytes: torch.empty(max(int(nbytes) // 8, 1), dtype=torch.int64, device='cuda')  # noqa: E731
    ws_c, ws_d = i64(L.cae_seg_components_workspace(n, edge, edge)), i64(L.cae_seg_object_distances_workspace(n, edge, edge))
    at = [0]

    def nxt():
        k = at[0] % sets
        at[0] += 1
        return k

    def components():
        k = nxt()
        _lib.check(L.cae_seg_components(targets[k].data_ptr(), None, n, edge, edge, 0, labels[k].data_ptr(),
                                        counts[k].data_ptr(), ws_c.data_ptr(), ws_c.numel() * 8, st))

    def distances():
        k = nxt()
        _lib.check(L.cae_seg_object_distances(labels[k].data_ptr(), n, edge, edge, d2[k].data_ptr(), ws_d.data_ptr(),
                                              ws_d.numel() * 8, st))

    def weight_map():
        k = nxt()
        _lib.check(L.cae_seg_weight_map(floats[k].data_ptr(), d2[k].data_ptr(), counts[k].data_ptr(), cw.data_ptr(), len(CLASS_WEIGHTS),
                                        float(2 * SIGMA ** 2), float(W_0), n, hw, out[k].data_ptr(), flag.data_ptr(), st))

    for fn in (components, distances, weight_map):  # every set once: the later entry points read what the earlier wrote
        at[0] = 0
        for _ in range(sets):
            fn()
    torch.cuda.synchronize()
    row = dict(planes=n, edge=edge, objects_asked=objects, objects_per_plane=float(counts[0].float().mean()), buffer_sets=sets,
               foreground=float((targets[0] > 0).float().mean()), flag=int(flag.item()),
               workspace_bytes=dict(components=ws_c.numel() * 8, distances=ws_d.numel() * 8))
    total = 0.0
    for name, fn in (('components', components), ('distances', distances), ('map', weight_map)):
        ms, runs = timed_groups(fn, inner)
        row[name + '_ms'], row[name + '_min_ms'], row[name + '_max_ms'], row[name + '_runs_ms'] = ms, min(runs), max(runs), runs
        total += ms
    row['device_ms'] = total
    row['candidates'] = n * hw * edge * 2
    row['candidates_per_s_over_distances_call'] = row['candidates'] / (row['distances_ms'] * 1e-3)

    # the step the map joins: a labelled batch of the same shape, rotation on, no weight-map keywords
    pool = torch.randint(0, 256, (2, edge + 64, edge + 64, 3), dtype=torch.uint8, device='cuda')
    pool_labels = torch.stack([torch.from_numpy(np.pad(base[i][0], 32, mode='wrap')) for i in range(2)]).cuda()
    sampler = LabeledPatchSampler(pool, pool_labels, edge, rotation=True, batch_size=n)
    draw = sampler.draw(n, torch.Generator().manual_seed(edge))
    ms, runs = timed_groups(lambda: sampler.gather(*draw), inner)
    row['gather_ms'], row['gather_min_ms'], row['gather_max_ms'], row['gather_runs_ms'] = ms, min(runs), max(runs), runs
    row['device_over_gather'] = total / ms
    row['distances_over_gather'] = row['distances_ms'] / ms

    if host:
        one = floats[0][:1, None]
        t0 = time.perf_counter()
        want = WeightsDistances(CLASS_WEIGHTS, SIGMA, W_0, force_torch=True)(one)
        host_ms = (time.perf_counter() - t0) * 1e3
        got = WeightsDistances(CLASS_WEIGHTS, SIGMA, W_0)(one)
        row.update(host_ms_one_plane=host_ms, host_ms=host_ms * n, host_over_device=host_ms * n / total,
                   max_abs_difference_to_host=float((got - want).abs().max()),
                   labels_equal_to_host=bool(torch.equal(got[:, 1], want[:, 1])))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'weight_map', 'mi355x.json'))
    ap.add_argument('--shapes', default='16x256,4x1024')
    ap.add_argument('--objects', default='10,100,1000')
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--footprint-mib', type=int, default=768, help='bytes the timed kernel calls cycle through')
    ap.add_argument('--no-host', action='store_true', help='leave out the host procedure (and the comparison with it)')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_weight_map.py measures on a HIP device; none is visible')
    result = dict(device=torch.cuda.get_device_name(0), class_weights=CLASS_WEIGHTS, sigma=SIGMA, w_0=W_0, cases=[])
    for n, edge in (tuple(map(int, s.split('x'))) for s in a.shapes.split(',')):
        for objects in (int(v) for v in a.objects.split(',')):
            row = bench_case(n, edge, objects, a.inner, a.footprint_mib << 20, not a.no_host)
            result['cases'].append(row)
            print(json.dumps({k: v for k, v in row.items() if not k.endswith('runs_ms')}), flush=True)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
