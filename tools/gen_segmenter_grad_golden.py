#!/usr/bin/env python3
"""Generate the gradient goldens of the segmentation head, tests/golden/seg_grad_*.npz, by running the REFERENCE's own
JNet in float64 on the CPU (sibling of gen_segmenter_golden.py).

Run only where the reference is present; never from a test or from smoke():

    python tools/gen_segmenter_grad_golden.py <reference checkout>

``src/models/tasks/_segmenters.py`` imports only torch, so it is loaded by file path and runs unmodified.  Per
configuration of tests/segmenter_restatement.py GOLDEN_CONFIGS the existing golden state dict and inputs are used
(inputs cloned: the reference's in-place ReLU overwrites them when batch_norm=False), with the seeded target of
tests/segmenter_train_restatement.py make_target and BCEWithLogits (mean) for one class, CrossEntropy (mean) otherwise:
  seg_grad_<name>.npz [seg_grad_<name>_<k>.npz]   'target', 'loss', 'grad/<parameter key>' (float64)
split over as many files as keep each one below the size limit.  Only data is written; no reference source is copied.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import segmenter_restatement as SR  # noqa: E402
import segmenter_train_restatement as ST  # noqa: E402

LIMIT = 556 * 1000


def load_reference(checkout):
    spec = importlib.util.spec_from_file_location('ref_segmenters', os.path.join(checkout, 'src/models/tasks/_segmenters.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def save(path, arrays):
    np.savez(path, **arrays)
    size = os.path.getsize(path)
    assert size <= LIMIT, (path, size)
    print(f'{os.path.relpath(path, ROOT)}: {size} bytes, {len(arrays)} arrays')


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = load_reference(sys.argv[1])
    for name in SR.GOLDEN_CONFIGS:
        cfg, sd, y_q, brg, _, _ = SR.load_golden(name)
        model = ref.JNet(**cfg).double().train()
        model.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
        target = ST.make_target(name)
        logits, aux = model(y_q.double().clone(), [b.double().clone() for b in brg] if brg else None)
        assert aux is None
        loss = ST.head_loss(logits, target)
        loss.backward()
        arrays = {'target': target.numpy(), 'loss': np.float64(loss.item())}
        grads = {'grad/' + k: p.grad.numpy() for k, p in model.named_parameters()}
        assert set(grads) == {'grad/' + k for k in sd}
        part, k, used = arrays, 0, sum(v.nbytes for v in arrays.values())
        for key, v in grads.items():
            if used + v.nbytes + 1024 * (len(part) + 1) > LIMIT:
                save(os.path.join(SR.GOLDEN, f'seg_grad_{name}' + (f'_{k}' if k else '') + '.npz'), part)
                part, k, used = {}, k + 1, 0
            part[key] = v
            used += v.nbytes
        save(os.path.join(SR.GOLDEN, f'seg_grad_{name}' + (f'_{k}' if k else '') + '.npz'), part)


if __name__ == '__main__':
    main()
