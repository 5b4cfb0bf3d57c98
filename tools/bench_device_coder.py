#!/usr/bin/env python3
"""Device rANS coder against the host coder on the canonical model.

    python tools/bench_device_coder.py --steps K --warmup W [--out FILE] [--no-slide] [--cpus N]

Per tile size (1024^2: 192 x 64 x 64 symbols per stream; 256^2: 192 x 16 x 16) and streams in flight (32, 64, 128, 256),
on the symbols of seeded synthetic tiles:
  device   encode / decode on the device clock (HIP events around the kernels and the read-back of offsets / statuses)
           and by wall time (host clock around the whole call: encode includes the D2H of the packed bytes, decode their
           H2D), as tiles/s, ns per symbol and ms per batch (the latency a caller sees), and host CPU seconds per tile
           (process time over the timed loop)
  host     the host coder on the same symbols (its default pool), wall time and CPU seconds per tile
Then SlideCoder.run tiles/s (1024^2, 32 tiles per batch), device mode against host mode, and both again in a child process
restricted to 8 CPUs.  Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def canonical():
    import cnn_autoencoder_amd as cae
    from cnn_autoencoder_amd import synth
    state = synth.synthetic_state(synth.CANONICAL, seed=0)
    codec = cae.ConvolutionalAutoencoder(checkpoint=state)
    eb = codec._model['fact_ent'].module
    eb.fit_quantiles()  # quantiles at the aux-loss fixed point, as bench.py
    eb.update(force=True)
    return codec, eb


def variants(t, n):
    """n tile batches' worth of distinct tiles from t (flips / transposes on the device)"""
    ops = [lambda x: x, lambda x: x.flip(1), lambda x: x.flip(2), lambda x: x.transpose(1, 2),
           lambda x: x.flip(1).flip(2), lambda x: x.transpose(1, 2).flip(1), lambda x: x.transpose(1, 2).flip(2),
           lambda x: x.transpose(1, 2).flip(1).flip(2)]
    out = torch.cat([ops[i % len(ops)](t).contiguous() for i in range((n + len(t) - 1) // len(t))])
    return out[:n].contiguous()


def symbols(codec, eb, tiles_dev):
    enc = codec._model['encoder'].module
    parts = [enc.forward_u8_symbols(tiles_dev[i:i + 32].contiguous(), eb) for i in range(0, len(tiles_dev), 32)]
    s = torch.cat(parts)
    return s.reshape(s.size(0), s.size(1), -1).contiguous()


def measure_device(eb, sym, steps, warmup):
    from cnn_autoencoder_amd.entropy import rans_decode_device, rans_encode_device
    h = eb._sync_handle()
    n, C, hw = sym.shape
    for _ in range(warmup):
        payloads = eb.encode_symbols_device(sym)
        eb.decode_symbols_device(payloads, hw)
    dev_enc, dev_dec = [], []
    for _ in range(steps):  # device clock
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        rans_encode_device(h, sym)
        e1.record()
        back = rans_decode_device(h, C, payloads, hw)
        e2.record()
        torch.cuda.synchronize()
        dev_enc.append(e0.elapsed_time(e1))
        dev_dec.append(e1.elapsed_time(e2))
    assert torch.equal(back, sym)
    wall_enc, wall_dec = [], []
    c0 = time.process_time()
    for _ in range(steps):  # wall clock, what a caller sees
        t0 = time.perf_counter()
        payloads = eb.encode_symbols_device(sym)
        t1 = time.perf_counter()
        eb.decode_symbols_device(payloads, hw)
        t2 = time.perf_counter()
        wall_enc.append(t1 - t0)
        wall_dec.append(t2 - t1)
    cpu = time.process_time() - c0
    nsym = n * C * hw

    def row(ms_list):
        ms = float(np.median(ms_list))
        return dict(ms_per_batch=ms, tiles_per_s=n / (ms * 1e-3), ns_per_symbol=ms * 1e6 / nsym,
                    ns_per_symbol_per_lane=ms * 1e6 / (C * hw), ms_min=float(np.min(ms_list)), ms_max=float(np.max(ms_list)))
    return dict(encode_device_clock=row(dev_enc), decode_device_clock=row(dev_dec),
                encode_wall=row([1e3 * v for v in wall_enc]), decode_wall=row([1e3 * v for v in wall_dec]),
                host_cpu_s_per_tile=cpu / (steps * n), bytes=payloads.offsets[-1])


def measure_host(eb, sym, steps, warmup):
    n, C, hw = sym.shape
    sh = sym.cpu().numpy()
    for _ in range(warmup):
        p = eb.encode_symbols(sh, packed=True)
        eb.decode_symbols(p, hw)
    we, wd = [], []
    c0 = time.process_time()
    for _ in range(steps):
        t0 = time.perf_counter()
        p = eb.encode_symbols(sh, packed=True)
        t1 = time.perf_counter()
        eb.decode_symbols(p, hw)
        t2 = time.perf_counter()
        we.append(t1 - t0)
        wd.append(t2 - t1)
    cpu = time.process_time() - c0
    return dict(encode_wall_ms=1e3 * float(np.median(we)), decode_wall_ms=1e3 * float(np.median(wd)),
                encode_tiles_per_s=n / float(np.median(we)), decode_tiles_per_s=n / float(np.median(wd)),
                host_cpu_s_per_tile=cpu / (steps * n))


def slide_rates(codec, tiles_dev, steps, warmup):
    from cnn_autoencoder_amd import slide
    batches = [variants(tiles_dev, 32)[i::1] for i in range(1)]
    batches = [b.contiguous() for b in (batches[0], batches[0].flip(1), batches[0].flip(2), batches[0].transpose(1, 2))]
    out = {}
    for mode in ('host', 'device'):
        sc = slide.SlideCoder(codec, coder=mode)
        sc.run([batches[k % 4] for k in range(warmup)])
        torch.cuda.synchronize()
        seq = [batches[k % 4] for k in range(steps)]
        c0, t0 = time.process_time(), time.perf_counter()
        stats, _ = sc.run(seq)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out[mode] = dict(tiles_per_s=32 * steps / dt, ms_per_step=1e3 * dt / steps,
                         host_cpu_s_per_tile=(time.process_time() - c0) / (32 * steps), bpp=float(slide.slide_summary(stats, 1024 * 1024)['bpp']))
        del sc
    out['device_vs_host'] = out['device']['tiles_per_s'] / out['host']['tiles_per_s']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-slide', action='store_true')
    ap.add_argument('--slide-only', action='store_true', help='only the SlideCoder.run comparison (the 8-CPU child)')
    ap.add_argument('--cpus', type=int, default=0, help='restrict this process to its first N allowed CPUs first')
    args = ap.parse_args()
    if args.cpus > 0:
        os.sched_setaffinity(0, sorted(os.sched_getaffinity(0))[:args.cpus])
    from cnn_autoencoder_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit('no HIP device: this tool measures the MI355X')
    codec, eb = canonical()
    t1024 = torch.from_numpy(synth.histo_tiles(8, 1024)).cuda()
    line = dict(tool='bench_device_coder', steps=args.steps, warmup=args.warmup,
                cpus_allowed=len(os.sched_getaffinity(0)), device=torch.cuda.get_device_name())
    if not args.slide_only:
        t256 = torch.from_numpy(synth.histo_tiles(32, 256, first_index=1000)).cuda()
        line['coder'] = {}
        for H, base in ((1024, t1024), (256, t256)):
            sym_all = symbols(codec, eb, variants(base, 256))
            for n in (32, 64, 128, 256):
                sym = sym_all[:n].contiguous()
                key = f'{H}x{H}_streams{n}'
                line['coder'][key] = dict(device=measure_device(eb, sym, args.steps, args.warmup),
                                          host=measure_host(eb, sym, max(2, args.steps // 2), 1))
                print(key, json.dumps(line['coder'][key]), file=sys.stderr, flush=True)
            del sym_all
            torch.cuda.empty_cache()
    if not args.no_slide:
        line['slide_run_1024'] = slide_rates(codec, t1024, max(args.steps, 8), args.warmup)
        if not args.slide_only and args.cpus == 0:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--cpus', '8', '--slide-only', '--steps',
                                str(args.steps), '--warmup', str(args.warmup)], capture_output=True, text=True, timeout=400)
            try:
                line['slide_run_1024_8cpu'] = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])['slide_run_1024']
            except Exception as e:  # noqa: BLE001 - report, keep the line
                line['slide_run_1024_8cpu'] = dict(error=repr(e)[:200], stderr=r.stderr[-500:])
    s = json.dumps(line)
    print(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(s + '\n')


if __name__ == '__main__':
    main()
