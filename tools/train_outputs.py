#!/usr/bin/env python3
"""Forward outputs and gradients of four small training models, for comparing two versions of the training host layer
(cnn_autoencoder_amd/train.py) bit for bit.

    python tools/train_outputs.py dump SEED OUT.npz      # run the models of this checkout, write every tensor
    python tools/train_outputs.py compare A.npz B.npz    # one JSON line: bit-identity of outputs / data gradients, largest
                                                         # difference of the parameter gradients

Models (batch 2): GDN (32 / 40 channels, 40 x 56), LeakyReLU with pre-convolutions (40 / 32, 37 x 45), multiscale GDN
(32 / 40, 40 x 56) and residual GDN units (40 / 32, 37 x 45).  Per model: y = analysis(x), (x_r, colour outputs) =
synthesis(y as a leaf), loss = sum of every output against fixed random weights.  `y`, `x_r*` and `g_y` (the synthesis
track's input gradient) come from kernels without atomics: two runs of one checkout agree bit for bit.  Weight, bias, beta
and gamma gradients (`p.*`) end in an atomic flush and differ from run to run.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODELS = dict(
    gdn=(dict(channels_net=32, channels_bn=40, act_layer_type='GDN', bias=True), (40, 56)),
    lrelu=(dict(channels_net=40, channels_bn=32, act_layer_type='LeakyReLU', bias=True), (37, 45)),
    multiscale=(dict(channels_net=32, channels_bn=40, act_layer_type='GDN', bias=True, multiscale_analysis=True), (40, 56)),
    residual=(dict(channels_net=40, channels_bn=32, act_layer_type='GDN', use_residual=True), (37, 45)),
)


def dump(seed: int, path: str) -> None:
    import cnn_autoencoder_amd as cae
    torch.cuda.set_device(0)
    out = {}
    for name, (kw, (h, w)) in MODELS.items():
        torch.manual_seed(seed)
        enc_kw = {k: v for k, v in kw.items() if k != 'multiscale_analysis'}
        enc = cae.Analyzer(channels_org=3, compression_level=3, **enc_kw).cuda().train()
        dec = cae.Synthesizer(channels_org=3, compression_level=3, **kw).cuda().train()
        x = torch.rand(2, 3, h, w, device='cuda')
        y = enc(x)
        y_leaf = y.detach().requires_grad_(True)
        x_r, _ = dec(y_leaf)
        outs = [y] + [t for t in x_r if t is not None]
        sum((t * torch.rand_like(t)).sum() for t in outs).backward()
        out[f'{name}.y'] = y
        for j, t in enumerate(t for t in x_r if t is not None):
            out[f'{name}.x_r{j}'] = t
        out[f'{name}.g_y'] = y_leaf.grad
        for part, m in (('enc', enc), ('dec', dec)):
            for k, p in m.named_parameters():
                if p.grad is not None:
                    out[f'{name}.p.{part}.{k}'] = p.grad
    np.savez(path, **{k: v.detach().float().cpu().numpy() for k, v in out.items()})
    print(f'{len(out)} tensors -> {path}')


def compare(a_path: str, b_path: str) -> None:
    a, b = np.load(a_path), np.load(b_path)
    assert sorted(a.files) == sorted(b.files), 'different tensor names'
    exact = [k for k in a.files if '.p.' not in k]
    differing = [k for k in exact if a[k].tobytes() != b[k].tobytes()]
    rel = {k: float(np.abs(a[k] - b[k]).max() / max(np.abs(a[k]).max(), 1e-30)) for k in a.files if '.p.' in k}
    worst = max(rel, key=rel.get)
    print(json.dumps(dict(a=a_path, b=b_path, exact_tensors=len(exact), not_bit_identical=differing,
                          param_grads=len(rel), param_grad_max_rel_diff=rel[worst], at=worst)))
    if differing:
        sys.exit(1)


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[1] == 'dump':
        dump(int(sys.argv[2]), sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == 'compare':
        compare(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
