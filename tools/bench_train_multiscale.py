"""ms per training step of the canonical model (channels_net 128, channels_bn 192, compression_level 4, GDN; 256 x 256
patches, batch 128) without and with multiscale colour layers (RateMultiscaleMSE, per-level lambda), the colour layers in
both forms (edge GEMM, and the padded stride-1 form of CAE_EDGE_GEMM=0), in one process.  Prints one JSON line.

    python tools/bench_train_multiscale.py [--batch 128] [--size 256] [--steps 10] [--warmup 3]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    import cnn_autoencoder_amd as cae
    from cnn_autoencoder_amd import criteria, synth, train
    torch.cuda.set_device(0)
    cfg = dict(synth.CANONICAL)
    L = cfg['compression_level']
    x = torch.rand(args.batch, cfg['channels_org'], args.size, args.size, device='cuda')

    def run(multiscale: bool, edge: str) -> float:
        os.environ['CAE_EDGE_GEMM'] = edge
        model = cae.autoencoder_from_state_dict(synth.synthetic_state(cfg, seed=0), train=True)
        if multiscale:
            torch.manual_seed(0)
            kw = {k: cfg[k] for k in ('channels_org', 'channels_net', 'channels_bn', 'compression_level', 'kernel_size',
                                      'bias', 'act_layer_type') if k in cfg}
            dec = cae.Synthesizer(multiscale_analysis=True, **kw).cuda()
            model['decoder'] = nn.DataParallel(dec, device_ids=[torch.cuda.current_device()]).train()
            crit = criteria.setup_loss('RateMultiscaleMSE', channels_org=cfg['channels_org'], compression_level=L,
                                       distortion_lambda=[0.01 / 2 ** s for s in range(L)])
        else:
            crit = criteria.setup_loss('RateMSE', distortion_lambda=0.01)
        opts = train.setup_optim(model)
        for _ in range(args.warmup):
            train.train_step(x, model, crit, opts)
        torch.cuda.synchronize()
        best = float('inf')
        for _ in range(2):  # two repetitions, the faster one
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.steps):
                train.train_step(x, model, crit, opts)
            t1.record()
            torch.cuda.synchronize()
            best = min(best, t0.elapsed_time(t1) / args.steps)
        return best

    res = dict(batch=args.batch, size=args.size, steps=args.steps)
    res['plain_ms'] = run(False, '1')
    res['multiscale_edge_ms'] = run(True, '1')
    res['multiscale_padded_ms'] = run(True, '0')
    res['edge_over_plain'] = res['multiscale_edge_ms'] / res['plain_ms']
    res['padded_over_plain'] = res['multiscale_padded_ms'] / res['plain_ms']
    print(json.dumps(res))


if __name__ == '__main__':
    main()
