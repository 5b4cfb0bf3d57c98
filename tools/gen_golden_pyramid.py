"""Writes tests/golden/ref_loss_pyramid.npz: values of the reference's multiscale objective (setup_loss('RateMultiscaleMSE'):
GeneralLoss with DistMSEPyramidLoss and RateLoss, _lossutils.py:5-151, _ratedist.py:10-43, 88-93) on seeded tensors.

Needs the reference's sources (loaded through oracle.gen_golden.load_reference_criteria); the fixture holds data only.
Per case (channels_org, compression_level, height, width): the input x, the per-level targets of downsample_pyramid,
the per-level reconstructions x_r, p_y, and for a scalar lambda and a per-level lambda list the reference's `dist`
list, `dist_loss` and `loss` (the scalar lambda weights level 0 only: zip stops at the shorter input).

    python tools/gen_golden_pyramid.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_golden import load_reference_criteria  # noqa: E402

CASES = [(3, 3, 64, 80), (3, 4, 37, 45), (1, 4, 64, 80), (1, 3, 37, 45)]
LAMBDAS = {'scalar': 0.01}


def main():
    crit = load_reference_criteria()
    aux = torch.tensor(3.5)

    class _Fe:
        def loss(self):
            return aux

    class _Wrapped:
        module = _Fe()

    out = {}
    meta = []
    for ci, (c, L, H, W) in enumerate(CASES):
        g = torch.Generator().manual_seed(1000 + ci)
        x = torch.rand(1, c, H, W, generator=g)
        pyr = crit['_ratedist'].DistMSEPyramidLoss(channels_org=c, compression_level=L)
        targets = [x]
        for _ in range(L - 1):
            targets.append(pyr.downsample_pyramid(targets[-1]))
        x_r = [(t + 0.05 * torch.randn(t.shape, generator=g)).clamp(0, 1) for t in targets]
        p_y = torch.rand(1, 8, max(H // 2 ** L, 1), max(W // 2 ** L, 1), generator=g).clamp_min(1e-9)
        pre = f'c{ci}_'
        out[pre + 'x'] = x.numpy()
        out[pre + 'p_y'] = p_y.numpy()
        for s in range(L):
            out[pre + f'target{s}'] = targets[s].numpy()
            out[pre + f'x_r{s}'] = x_r[s].numpy()
        lams = dict(LAMBDAS, list=[1.0 / 2 ** s for s in range(L)])
        for tag, lam in lams.items():
            loss_fn = crit['_lossutils'].setup_loss('RateMultiscaleMSE', channels_org=c, compression_level=L,
                                                    distortion_lambda=lam)
            ld = loss_fn(inputs=x, outputs=dict(x_r=list(x_r), p_y=p_y, y=None), net={'fact_ent': _Wrapped()})
            out[pre + f'dist_{tag}'] = np.array([float(d) for d in ld['dist']], dtype=np.float64)
            out[pre + f'dist_loss_{tag}'] = np.float64(float(ld['dist_loss']))
            out[pre + f'loss_{tag}'] = np.float64(float(ld['loss']))
        meta.append(dict(channels_org=c, compression_level=L, height=H, width=W, lambdas=lams))
    out['cases_json'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(ROOT, 'tests', 'golden', 'ref_loss_pyramid.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path}: {len(CASES)} cases')


if __name__ == '__main__':
    main()
