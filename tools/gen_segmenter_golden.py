#!/usr/bin/env python3
"""Generate the segmentation head's golden fixtures, tests/golden/seg_*.npz, by running the REFERENCE's own JNet.

Run only where the reference is present (it is absent on the GPU box); never from a test or from smoke():

    python tools/gen_segmenter_golden.py

``src/models/tasks/_segmenters.py`` imports only torch, so it is loaded by file path and runs unmodified: the fixtures
are reference-pinned end to end.  Per configuration (tests/segmenter_restatement.py GOLDEN_CONFIGS):
  seg_<name>.npz           state dict ('sd/<key>') and 'logits'
  seg_<name>_inputs.npz    'y_q', 'bridge/<i>'
  seg_<name>_stages<k>.npz the output of every layer with parameters, captured by forward hooks under the layer's name
                           and split over as many files as keep each one below the size limit
Only data is written; no reference source is copied.  GroupNorm's gamma / beta are redrawn from the seed (their
default 1 / 0 would leave the affine map untested).  The reference's in-place ReLU overwrites its inputs when
batch_norm=False, so the model is fed clones and the hooks clone what they see.
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import segmenter_restatement as SR  # noqa: E402

REF = '/root/reference/src/models/tasks/_segmenters.py'
LIMIT = 556 * 1000  # the largest file in tests/golden before these


def load_reference():
    spec = importlib.util.spec_from_file_location('ref_segmenters', REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def save(path, arrays):
    np.savez(path, **arrays)
    size = os.path.getsize(path)
    assert size <= LIMIT, (path, size)
    print(f'{os.path.relpath(path, ROOT)}: {size} bytes, {len(arrays)} arrays')


def main():
    ref = load_reference()
    for seed, (name, (cfg, (lh, lw), n)) in enumerate(SR.GOLDEN_CONFIGS.items()):
        torch.manual_seed(100 + seed)
        model = ref.JNet(**cfg).eval()
        with torch.no_grad():
            for m in model.modules():
                if isinstance(m, nn.GroupNorm):
                    m.weight.copy_(1.0 + 0.5 * torch.randn_like(m.weight))
                    m.bias.copy_(0.3 * torch.randn_like(m.bias))
        L = cfg['compression_level']
        y_q = torch.round(3.0 * torch.randn(n, cfg['channels_bn'], lh, lw))
        ch = [cfg['channels_net']] * (L - 1) + [3]
        brg = [torch.rand(n, c, lh * 2 ** (i + 1), lw * 2 ** (i + 1)) for i, c in enumerate(ch)] if cfg['concat_bridges'] else []
        stages = {}
        for key, m in model.named_modules():
            if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d, nn.GroupNorm)):
                m.register_forward_hook(lambda mod, inp, out, key=key: stages.__setitem__(key, out.detach().clone().numpy()))
        with torch.no_grad():
            logits, aux = model(y_q.clone(), [b.clone() for b in brg] if brg else None)
        assert aux is None
        arrays = {'sd/' + k: v.numpy() for k, v in model.state_dict().items()}
        arrays['logits'] = logits.numpy()
        save(os.path.join(SR.GOLDEN, f'seg_{name}.npz'), arrays)
        inputs = {'y_q': y_q.numpy()}
        inputs.update({f'bridge/{i}': b.numpy() for i, b in enumerate(brg)})
        save(os.path.join(SR.GOLDEN, f'seg_{name}_inputs.npz'), inputs)
        part, k, used = {}, 0, 0
        for key, v in stages.items():
            if part and used + v.nbytes + 1024 * (len(part) + 1) > LIMIT:
                save(os.path.join(SR.GOLDEN, f'seg_{name}_stages{k}.npz'), part)
                part, k, used = {}, k + 1, 0
            part[key] = v
            used += v.nbytes
        save(os.path.join(SR.GOLDEN, f'seg_{name}_stages{k}.npz'), part)


if __name__ == '__main__':
    main()
