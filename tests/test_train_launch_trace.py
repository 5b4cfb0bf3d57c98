"""The launch sequence of the training host layer (cnn_autoencoder_amd/train.py), held still on the CPU.

The library is replaced by a stub whose every entry point records (name, arguments) and returns 0 (the two size queries
return their real formulas); `_lib.check` and `_lib.stream_ptr` are neutralised.  The autograd functions of train.py then run
forward and backward on CPU tensors: nothing is computed, but every integer the host derives from shapes, every choice of
entry point, every optional pointer and the order of the calls is exactly what a GPU run would hand to the library.

An argument is recorded as its value if it is an int below 2^20, as "null" for None and as "ptr" otherwise (no buffer
identities: tensor lifetimes may change and addresses get reused).  Next to each trace stands the count per ATen op seen by a
TorchDispatchMode over the same forward and backward -- the torch ops of the host layer that become launches on a device too.

tests/golden/train_launch_trace.json was recorded by this module's recorder (`python tests/test_train_launch_trace.py
--record OUT`, PYTHONPATH pointing at a checkout of that commit) from train.py as it stood before its launches moved into one
wrapper per entry point and its steps into shared helpers.  The test asserts the call trace EQUALS the recorded one and that
no ATen op runs more often than recorded (fewer is allowed).
"""
import collections
import contextlib
import json
import os
import sys

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'train_launch_trace.json')


class _StubLib:
    """every attribute is a recording entry point"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append([name] + [a if isinstance(a, int) and not isinstance(a, bool) and a < 2 ** 20
                                        else ('null' if a is None else 'ptr') for a in args])
            if name == 'cae_t_packed_bytes':
                k, n, ks = args
                return -(-k // 32) * ks * ks * -(-n // 32) * 2048
            if name == 'cae_t_gdn_saved_elems':
                return args[0] * args[1]
            return 0
        return entry


class _CountOps(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.counts = collections.Counter()

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.counts[str(func)] += 1
        return func(*args, **(kwargs or {}))


@contextlib.contextmanager
def _stubbed(env):
    """train.py on the stub library, with the environment switches of a case; -> (stub, op counter)"""
    from cnn_autoencoder_amd import _lib
    stub, ops = _StubLib(), _CountOps()
    keep = (_lib.lib, _lib.stream_ptr, _lib.check)
    keys = ('CAE_EDGE_GEMM', 'CAE_GDN_FUSED')
    old = {k: os.environ.pop(k, None) for k in keys}
    os.environ.update(env)
    _lib.lib, _lib.stream_ptr, _lib.check = (lambda: stub), (lambda: None), (lambda rc: None)
    try:
        with ops:
            yield stub, ops
    finally:
        _lib.lib, _lib.stream_ptr, _lib.check = keep
        for k in keys:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def _leaf(*shape):
    return torch.full(shape, 0.01).requires_grad_(True)


def _track_tensors(specs, synthesis):
    """flat parameter list of a fused track, in train._split_params order"""
    out = []
    for s in specs:
        if s.has_pre:
            out.append(_leaf(s.cin, s.cin, s.ks, s.ks))
            if s.has_bias:
                out.append(_leaf(s.cin))
        out.append(_leaf(s.cin, s.cout, s.ks, s.ks) if synthesis else _leaf(s.cout, s.cin, s.ks, s.ks))
        if s.has_bias:
            out.append(_leaf(s.cout))
        if s.has_gdn:
            out += [_leaf(s.cout_p), _leaf(s.cout_p, s.cout_p)]
    return out


def _backward(outs):
    sum(o.sum() for o in outs).backward()


def _analysis(chans, ks, bias, gdn, act=0, pre=False, image=(2, 3, 20, 24)):
    def run(T):
        last = len(chans) - 2
        specs = tuple(T.LayerSpec(a, b, ks, bias, gdn and i < last, act=act, has_pre=pre)
                      for i, (a, b) in enumerate(zip(chans, chans[1:])))
        _backward([T.AnalysisFn.apply(torch.zeros(image), specs, *_track_tensors(specs, False))])
    return run


def _synthesis(chans, ks, bias, gdn, act=0, pre=False, colour=(), read=None, input_grad=True, latent=(5, 6)):
    """colour: cout per non-last level; read: indices of the outputs (0 = x_r) the loss reads, None = all"""
    def run(T):
        last = len(chans) - 2
        specs = tuple(T.LayerSpec(a, b, ks, bias, gdn and i < last, act=act, has_pre=pre)
                      for i, (a, b) in enumerate(zip(chans, chans[1:])))
        cspecs = tuple(T.ColourSpec(chans[i + 1], co, ks, bias) for i, co in enumerate(colour)) or None
        ct = []
        for cs in cspecs or ():
            ct += [_leaf(cs.cout, cs.cin, cs.ks, cs.ks)] + ([_leaf(cs.cout)] if cs.has_bias else [])
        yq = torch.zeros((2, chans[0]) + latent, requires_grad=input_grad)
        out = T.SynthesisFn.apply(yq, specs, cspecs, *_track_tensors(specs, True), *ct)
        outs = list(out) if cspecs else [out]
        _backward([o for i, o in enumerate(outs) if read is None or i in read])
    return run


def _conv_s1(synthesis, act, bias):
    def run(T):
        _backward([T._ConvS1Fn.apply(_leaf(2, 40, 9, 11), synthesis, 3, act, _leaf(40, 40, 3, 3), _leaf(40) if bias else None)])
    return run


def _conv_s2(T):
    _backward([T._ConvS2Fn.apply(_leaf(2, 40, 9, 11), 3, _leaf(32, 40, 3, 3), _leaf(32))])
    _backward([T._ConvS2Fn.apply(_leaf(2, 32, 8, 6), 5, _leaf(40, 32, 5, 5), None)])


def _gdn(c):
    def run(T):
        for inverse in (False, True):
            _backward([T._GdnFn.apply(_leaf(2, c - 3, 7, 5), inverse, _leaf(c), _leaf(c, c))])
    return run


def _colour_fn(T):
    for cout, bias in ((3, True), (4, False)):  # edge form, padded form
        cs = T.ColourSpec(40, cout, 3, bias)
        _backward([T._ColourFn.apply(_leaf(2, 40, 9, 11), cs, _leaf(cout, 40, 3, 3), _leaf(cout) if bias else None)])


def _batch_norm(T):
    _backward([T._BatchNormFn.apply(_leaf(2, 40, 9, 11), _leaf(40), _leaf(40), 1e-5)[0]])
    _backward([T._BatchNormFn.apply(_leaf(2, 40, 9, 11), None, None, 1e-5)[0]])


def _composed(synthesis, residual, act, batch_norm=False, groups=False, colour=False):
    """train._composed_track over two unit modules (they construct without a device)"""
    def run(T):
        from cnn_autoencoder_amd import modules as M
        cls = {(False, False): M.DownsamplingUnit, (False, True): M.ResidualDownsamplingUnit,
               (True, False): M.UpsamplingUnit, (True, True): M.ResidualUpsamplingUnit}[(synthesis, residual)]
        torch.manual_seed(0)
        units = [cls(32, 32, 3, groups=groups, batch_norm=batch_norm, bias=True, act_layer_type=act),
                 cls(32, 40, 3, batch_norm=batch_norm, bias=False, act_layer_type=act)]
        for u in units:
            u.train()
        x = _leaf(2, 32, 6, 5)
        if colour:
            cs = (T.ColourSpec(32, 3, 3, True),)
            out, cols = T._composed_track(units, x, True, cs, [_leaf(3, 32, 3, 3), _leaf(3)])
            _backward([out] + cols)
        else:
            _backward([T._composed_track(units, x, synthesis)])
    return run


def _track_inputs(T):
    """_track_inputs / _colour_inputs of fused-form units (pure host code: the GDN parameters come from _gdn_params)"""
    from cnn_autoencoder_amd import modules as M
    units = [M.UpsamplingUnit(40, 40, 3, act_layer_type='GDN'), M.UpsamplingUnit(40, 3, 3, act_layer_type=None)]
    specs, tensors = T._track_inputs(None, units, True)
    assert [t.shape[0] for t in tensors] == [40, 40, 64, 64, 40, 3] and specs[0].has_gdn and not specs[1].has_gdn
    assert torch.equal(tensors[2][40:], torch.ones(24)) and not tensors[3][40:].any() and not tensors[3][:, 40:].any()
    units = [M.DownsamplingUnit(3, 32, 3, bias=True, act_layer_type='ReLU'), M.ResidualDownsamplingUnit(32, 32, 3)]
    assert T._track_inputs(None, units[:1], False)[0][0].has_pre and T._track_inputs(None, units, False) == (None, None)


_E0, _G0 = {'CAE_EDGE_GEMM': '0'}, {'CAE_GDN_FUSED': '0'}
CASES = {
    'analysis_gdn': ({}, _analysis((3, 32, 32), 3, True, True)),
    'analysis_gdn_padded_edge': (_E0, _analysis((3, 32, 32), 3, True, True)),
    'analysis_gdn_unfused': (_G0, _analysis((3, 32, 32), 3, True, True)),
    'analysis_gdn_160': ({}, _analysis((3, 160, 32), 3, True, True)),
    'analysis_k5_plain_odd': ({}, _analysis((3, 32, 32), 5, False, False, image=(2, 3, 21, 19))),
    'analysis_leaky_pre': ({}, _analysis((3, 40, 40), 3, True, False, act=1, pre=True)),
    'analysis_relu_three_units': ({}, _analysis((3, 40, 32, 40), 3, False, False, act=2)),
    'synthesis_gdn': ({}, _synthesis((32, 32, 3), 3, True, True)),
    'synthesis_gdn_no_input_grad': ({}, _synthesis((32, 32, 3), 3, True, True, input_grad=False)),
    'synthesis_gdn_padded_edge': (_E0, _synthesis((32, 32, 3), 3, True, True)),
    'synthesis_gdn_padded_edge_no_input_grad': (_E0, _synthesis((32, 32, 3), 3, True, True, input_grad=False)),
    'synthesis_gdn_unfused_160': (_G0, _synthesis((32, 160, 3), 3, False, True)),
    'synthesis_colour_edge_and_padded': ({}, _synthesis((32, 32, 40, 3), 3, True, True, colour=(3, 4))),
    'synthesis_colour_all_padded': (_E0, _synthesis((32, 32, 40, 3), 3, True, True, colour=(3, 4))),
    'synthesis_colour_one_unread': ({}, _synthesis((32, 32, 40, 3), 3, True, True, colour=(3, 4), read=(0, 2))),
    'synthesis_colour_only': (_E0, _synthesis((32, 32, 40, 3), 3, False, True, colour=(3, 3), read=(1,))),
    'synthesis_colour_plain': ({}, _synthesis((32, 40, 3), 3, True, False, colour=(3,))),
    'synthesis_colour_plain_padded_edge': (_E0, _synthesis((32, 40, 3), 3, True, False, colour=(3,))),
    'synthesis_colour_leaky_pre': ({}, _synthesis((32, 40, 3), 3, True, False, act=1, pre=True, colour=(3,))),
    'synthesis_relu_pre_k5_three_units': ({}, _synthesis((32, 40, 32, 3), 5, False, False, act=2, pre=True)),
    'synthesis_relu_pre_no_input_grad': ({}, _synthesis((40, 3), 3, True, False, act=2, pre=True, input_grad=False)),
    'synthesis_leaky_three_units': ({}, _synthesis((32, 40, 32, 3), 3, True, False, act=1)),
    'synthesis_plain': ({}, _synthesis((32, 40, 3), 3, True, False)),
    'synthesis_plain_padded_edge': (_E0, _synthesis((32, 40, 3), 3, False, False)),
    'synthesis_single_layer': ({}, _synthesis((32, 40), 3, True, False, latent=(7, 5))),
    'synthesis_single_edge_layer': ({}, _synthesis((40, 3), 3, False, False, input_grad=False)),
    'synthesis_single_edge_layer_input_grad': ({}, _synthesis((40, 3), 3, True, False)),
    'conv_s1_analysis': ({}, _conv_s1(False, 0, True)),
    'conv_s1_analysis_act': ({}, _conv_s1(False, 1, False)),
    'conv_s1_synthesis': ({}, _conv_s1(True, 0, False)),
    'conv_s1_synthesis_act': ({}, _conv_s1(True, 1, True)),
    'conv_s2': ({}, _conv_s2),
    'gdn_fn': ({}, _gdn(32)),
    'gdn_fn_unfused': (_G0, _gdn(64)),
    'gdn_fn_160': ({}, _gdn(160)),
    'colour_fn': ({}, _colour_fn),
    'colour_fn_padded': (_E0, _colour_fn),
    'batch_norm_fn': ({}, _batch_norm),
    'composed_analysis_residual_gdn': ({}, _composed(False, True, 'GDN')),
    'composed_synthesis_residual_gdn_colour': ({}, _composed(True, True, 'GDN', colour=True)),
    'composed_analysis_batch_norm_leaky': ({}, _composed(False, False, 'LeakyReLU', batch_norm=True)),
    'composed_synthesis_batch_norm_relu': ({}, _composed(True, False, 'ReLU', batch_norm=True)),
    'composed_analysis_residual_relu_grouped': ({}, _composed(False, True, 'ReLU', groups=True)),
    'composed_synthesis_residual_leaky': ({}, _composed(True, True, 'LeakyReLU')),
    'track_inputs': ({}, _track_inputs),
}


def trace(name):
    """-> dict(calls=[[entry point, arguments...]], aten={op: count}) of one case"""
    from cnn_autoencoder_amd import train as T
    env, run = CASES[name]
    with _stubbed(env) as (stub, ops):
        run(T)
    return dict(calls=stub.calls, aten=dict(sorted(ops.counts.items())))


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_cases_are_the_recorded_ones():
    assert sorted(_golden()) == sorted(CASES)


@pytest.mark.parametrize('name', sorted(CASES))
def test_launch_trace_equals_the_recorded_one(name):
    want, got = _golden()[name], trace(name)
    assert len(got['calls']) == len(want['calls']), (len(got['calls']), len(want['calls']))
    for k, (g, w) in enumerate(zip(got['calls'], want['calls'])):
        assert g == w, f'call {k}: {g} != {w}'
    more = {op: (n, want['aten'].get(op, 0)) for op, n in got['aten'].items() if n > want['aten'].get(op, 0)}
    assert not more, f'ATen ops that run more often than recorded (now, recorded): {more}'


if __name__ == '__main__':
    if ROOT not in sys.path:
        sys.path.append(ROOT)  # (behind PYTHONPATH: the recorder runs on the train.py that comes first)
    if len(sys.argv) == 3 and sys.argv[1] == '--record':
        import cnn_autoencoder_amd.train as _T
        out = {name: trace(name) for name in sorted(CASES)}
        with open(sys.argv[2], 'w') as f:
            f.write('{\n' + ',\n'.join(f'{json.dumps(k)}: {json.dumps(v, separators=(",", ":"))}' for k, v in out.items())
                    + '\n}\n')
        print(f'{len(out)} cases, {sum(len(v["calls"]) for v in out.values())} calls recorded from {_T.__file__}')
    else:
        sys.exit('usage: test_train_launch_trace.py --record OUT.json')
