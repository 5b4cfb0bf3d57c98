"""Cost of the MS-SSIM distortion in the training step of the canonical model (channels_net 128, channels_bn 192,
compression_level 4, GDN; 256 x 256 patches) at batch 128 and batch 16, in one process:

  * ms per training step under RateMSE (for scale), under RateMSSSIM with the fused loss kernels, and under RateMSSSIM with
    the forced torch-op form (force_torch=True: depthwise conv2d under autograd);
  * device ms of the loss forward + backward alone, both forms, on fixed device tensors;
  * the fused loss time as a multiple of its HBM floor: X and Y read in both directions and the gradient written, over
    the five scales (20 B per element and scale), at the achievable 6.3 TB/s and at the 8 TB/s of the data sheet.

Timing: events on the stream around each repetition, after warm-up; median, min and max of --reps (>= 7) repetitions.
Prints one JSON line and, with --out, writes it to a file (profiles/msssim_train/bench_mi355x.json is such a run).

    python tools/bench_train_msssim.py [--batches 128,16] [--size 256] [--reps 9] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE, HBM_SPEC = 6.3e12, 8.0e12  # bytes / s


def timed(fn, reps, warmup):
    """-> dict(median, min, max) of the device ms of fn()"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), reps=reps)


def floor_bytes(n, c, side, win=11):
    """X, Y read forward and backward + the gradient written, summed over the five scales"""
    total, s = 0, side
    for _ in range(5):
        total += 20 * n * c * s * s
        s = (s + 2 * (s % 2) - 2) // 2 + 1
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='128,16')
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--lam', type=float, default=1.0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.reps < 7:
        ap.error('--reps must be at least 7')
    import cnn_autoencoder_amd as cae
    from cnn_autoencoder_amd import criteria, synth, train
    torch.cuda.set_device(0)
    cfg = dict(synth.CANONICAL)
    res = dict(device=torch.cuda.get_device_name(0), size=args.size, model='canonical', runs=[])

    def guarded(fn):
        """the torch-op form depends on the library's depthwise convolutions: an error is recorded, not hidden"""
        try:
            return fn()
        except RuntimeError as e:
            torch.cuda.synchronize()
            return dict(error=str(e)[:2000])

    for batch in [int(b) for b in args.batches.split(',')]:
        x = torch.rand(batch, cfg['channels_org'], args.size, args.size, device='cuda')
        x_r0 = (x + 0.05 * torch.randn_like(x))
        run = dict(batch=batch)

        def loss_only(force_torch):
            dist = criteria.DistMSSSIMLoss(args.size, force_torch=force_torch)

            def once():
                t = x_r0.detach().requires_grad_(True)
                dist(x=x, x_r=[t])['dist'][0].backward()
            return timed(once, args.reps, args.warmup)

        def step(name, **kw):
            model = cae.autoencoder_from_state_dict(synth.synthetic_state(cfg, seed=0), train=True)
            crit = criteria.setup_loss(name, **kw)
            opts = train.setup_optim(model)
            return timed(lambda: train.train_step(x, model, crit, opts), args.reps, args.warmup)

        run['loss_fused'] = loss_only(False)
        run['loss_torch_ops'] = guarded(lambda: loss_only(True))
        run['step_rate_mse'] = step('RateMSE', distortion_lambda=0.01)
        run['step_rate_msssim_fused'] = step('RateMSSSIM', patch_size=args.size, distortion_lambda=args.lam)
        run['step_rate_msssim_torch_ops'] = guarded(
            lambda: step('RateMSSSIM', patch_size=args.size, distortion_lambda=args.lam, force_torch=True))
        nbytes = floor_bytes(batch, cfg['channels_org'], args.size)
        fused_s = run['loss_fused']['median_ms'] * 1e-3
        run['hbm_floor'] = dict(bytes=nbytes, floor_ms_at_6p3_TBps=nbytes / HBM_ACHIEVABLE * 1e3,
                                floor_ms_at_8_TBps=nbytes / HBM_SPEC * 1e3,
                                fused_over_floor_6p3=fused_s / (nbytes / HBM_ACHIEVABLE),
                                fused_over_floor_8=fused_s / (nbytes / HBM_SPEC))
        if 'median_ms' in run['loss_torch_ops']:
            run['torch_ops_over_fused_loss'] = run['loss_torch_ops']['median_ms'] / run['loss_fused']['median_ms']
        res['runs'].append(run)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
