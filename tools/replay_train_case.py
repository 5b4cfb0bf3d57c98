#!/usr/bin/env python3
"""Rebuild case K of the training sweep with seed S (tests/fuzz/fuzz_train.py) and judge its analysis and synthesis tracks
(a) per operation (tests/train_replay.py: every kernel call replayed alone in float64), (b) end to end against the float64
restatement (oracle.train_oracle.residual_track(bf16=False) on double leaves), next to the bf16 restatement's own distance
from it, (c) again with CAE_EDGE_GEMM=0 and with CAE_GDN_FUSED=0.  Needs the GPU.
    replay_train_case.py SEED:CASE [SEED:CASE ...]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'fuzz'))
import cnn_autoencoder_amd as cae  # noqa: E402
import train_cases  # noqa: E402
from train_replay import e2e_rule, judge_track  # noqa: E402


def run(seed, k):
    c = train_cases.case(seed, k)
    print(f'seed {seed} {train_cases.describe(k, c)}', flush=True)
    act = c['kw']['act_layer_type']
    act_name = act if act in ('LeakyReLU', 'ReLU') else None
    for env in ({}, {'CAE_EDGE_GEMM': '0'}, {'CAE_GDN_FUSED': '0'}):
        old = {k_: os.environ.get(k_) for k_ in env}
        os.environ.update(env)
        try:
            enc, dec, x, yq = train_cases.build(c, cae)
            for name, mod, track, inp, synthesis in (('analysis', enc, enc.analysis_track, x, False),
                                                     ('synthesis', dec, dec.synthesis_track, yq, True)):
                V, rows = judge_track(mod, track, inp, synthesis, act_name)
                tag = ' '.join(f'{k_}={v}' for k_, v in env.items()) or 'default'
                print(f'  [{tag}] {name}: per-operation replay: {V.summary()}', flush=True)
                for f in V.failures[:10]:
                    print('    LOCAL FAIL', f, flush=True)
                worst = sorted(rows, key=lambda r: -r[1] / max(r[2], 1e-3 * r[3], 1e-30))[:4]
                print(f'    end to end: {sum(e2e_rule(r) == "fail" for r in rows)} of {len(rows)} results outside the bound', flush=True)
                for pname, e_k, e_b, umax, gmax in worst:
                    print(f'    {pname:44s} |gpu - f64| {e_k:.3e}  |bf16 restatement - f64| {e_b:.3e}  ratio {e_k / max(e_b, 1e-30):6.2f}'
                          f'  (/ unit max {e_k / umax:.2e}; / own max {e_k / max(gmax, 1e-30):.2e})', flush=True)
        finally:
            for k_, v in old.items():
                if v is None:
                    os.environ.pop(k_, None)
                else:
                    os.environ[k_] = v


for arg in sys.argv[1:]:
    s, k = arg.split(':')
    run(int(s), int(k))
