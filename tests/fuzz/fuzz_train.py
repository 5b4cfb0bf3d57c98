#!/usr/bin/env python3
"""Randomised gradient-parity sweep of the TRAINING path on the GPU: random unit variants (residual, batch norm, groups, bias,
activation, kernel size, depth, multiscale colour layers on the decoder) and sizes (tests/fuzz/train_cases.py).  Both tracks
of every case are judged twice (tests/train_replay.py):
  * per operation: every kernel call of a composed track (residual / batch-norm / grouped units, colour layers behind them)
    replayed alone in float64 from the inputs and the gradient it received, within c * 2^-24 * sum|terms| (+ one bf16 ulp
    where the kernel rounds) -- an operation that is wrong fails here whatever the conditioning of the model;
  * end to end: every output, parameter gradient and latent gradient against the float64 restatement
    (oracle/train_oracle.residual_track(bf16=False) on a float64 copy of the modules), within E2E_MULTIPLE x the distance of
    the restatement WITH the kernels' rounding points from it, plus E2E_FLOOR of the unit's largest gradient.
Canonical-style models take the fused track functions (end-to-end verdict only), the others the per-operation composition.
usage: fuzz_train.py [n_cases] [seed]   -> prints failures and the count of results judged by each rule, exits 1 on a failure."""
import os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cnn_autoencoder_amd as cae  # noqa: E402
from train_cases import build, describe, draw_case, generators  # noqa: E402
from train_replay import e2e_rule, judge_track  # noqa: E402

n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 60
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
rngs = generators(seed)
print(f'fuzz_train: seed {seed}, {n_cases} cases', flush=True)

fails = 0
count = dict(ops=0, local=0, mask_flips=0, multiple=0, floor=0, multiscale=0, blown=0)
t0 = time.time()
for case in range(n_cases):
    c = draw_case(*rngs)
    desc = describe(case, c)
    try:
        enc, dec, x_in, yq_in = build(c, cae)
    except (ValueError, NotImplementedError) as e:
        print('skip', desc, repr(e)[:80], flush=True)
        continue
    count['multiscale'] += c['multiscale']
    act = c['kw']['act_layer_type']
    act_name = act if act in ('LeakyReLU', 'ReLU') else None
    problems = []
    for name, mod, track, inp, synthesis in (
            ('analysis', enc, enc.analysis_track, x_in, False), ('synthesis', dec, dec.synthesis_track, yq_in, True)):
        V, rows = judge_track(mod, track, inp, synthesis, act_name, limit=1e4)
        if V is None:
            count['blown'] += 1
            continue
        count['ops'] += V.ops
        count['local'] += len(V.ratios)
        count['mask_flips'] += V.mask_flips
        problems += [f'{name} local: {f}' for f in V.failures[:5]]
        for row in rows:
            rule = e2e_rule(row)
            if rule == 'fail':
                pname, e_k, e_b, umax, _ = row
                problems.append(f'{name} {pname}: {e_k:.3e} from float64 (bf16 restatement {e_b:.3e}, unit max {umax:.3e})')
            else:
                count[rule] += 1
    if problems:
        fails += 1
        print('FAIL', desc, problems, flush=True)
    if (case + 1) % 10 == 0:
        print(f'... {case + 1} cases, {fails} failures so far, {time.time() - t0:.0f} s', flush=True)
print(f'{n_cases} cases ({count["multiscale"]} with multiscale decoders; {count["blown"]} tracks whose restatement blew up, '
      f'not judged), {fails} failures, {time.time() - t0:.0f} s')
print(f'per operation: {count["ops"]} kernel calls, {count["local"]} results within their local float64 bound, '
      f'{count["mask_flips"]} activation-mask disagreements at |pre-activation| within rounding of 0')
print(f'end to end: {count["multiple"]} results within 4 x the bf16 restatement\'s distance from float64, {count["floor"]} only '
      f'within the floor (1e-2 of the unit\'s largest gradient)')
sys.exit(1 if fails else 0)
