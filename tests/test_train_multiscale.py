"""Training with multiscale colour layers (multiscale_analysis, _autoencoders.py:417-452) and the pyramid MSE
(RateMultiscaleMSE, _ratedist.py:10-43, 88-93) on the GPU: the pyramid kernel against the reference's targets, the colour
layer kernels against F.conv2d with reflect padding, decoder gradients against the CPU restatement applied one layer at a
time, and a 20-step loss curve.  Tolerance as tests/test_train.py: 1e-3 of the largest magnitude against the restatement with
the same bf16 rounding points."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def cae(built_lib):
    import cnn_autoencoder_amd as cae
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return cae


def rel(got, want) -> float:
    return float((got.double().cpu() - want.double().cpu()).abs().max() / max(float(want.abs().max()), 1e-30))


def bf(x):
    return x.bfloat16().float()


def test_pyramid_down_kernel_matches_the_reference_targets(cae):
    from cnn_autoencoder_amd import criteria
    g = np.load(os.path.join(GOLD, 'ref_loss_pyramid.npz'))
    cases = json.loads(bytes(g['cases_json']).decode())
    for ci, case in enumerate(cases):
        t = torch.from_numpy(g[f'c{ci}_x']).cuda()
        for s in range(1, case['compression_level']):
            t = criteria.pyramid_down(t)
            assert rel(t, torch.from_numpy(g[f'c{ci}_target{s}'])) < 1e-6, (ci, s)


@pytest.mark.parametrize('edge', ['1', '0'])
@pytest.mark.parametrize('ks,c_org', [(3, 3), (3, 1), (5, 3), (5, 1)])
@pytest.mark.parametrize('size', ['P+1', 'P+2', 'odd', 'even'])
def test_colour_layer_kernels_match_reflect_conv(cae, ks, c_org, size, edge, monkeypatch):
    """forward (pointwise + cae_t_col2im_s1r), weight / bias gradient (cae_t_im2col_s1r + cae_t_wgrad_pointwise) and the data
    gradient accumulated onto an existing fp32 gradient (cae_t_pointwise_acc); edge '0': the padded stride-1 form."""
    from cnn_autoencoder_amd import train
    monkeypatch.setenv('CAE_EDGE_GEMM', edge)
    P = ks // 2
    h, w = {'P+1': (P + 1, P + 1), 'P+2': (P + 2, P + 1), 'odd': (13, 17), 'even': (16, 20)}[size]
    cin, n = 48, 2
    torch.manual_seed(ks * 10 + c_org)
    a = bf(torch.randn(n, cin, h, w)).requires_grad_(True)
    wt = bf(torch.randn(c_org, cin, ks, ks) / (cin * ks * ks) ** 0.5).requires_grad_(True)
    b = torch.randn(c_org).requires_grad_(True)
    out = F.conv2d(F.pad(a, (P,) * 4, mode='reflect'), wt, b)
    g = torch.randn_like(out)
    out.backward(bf(g))
    cs = train.ColourSpec(cin, c_org, ks, True)
    a16 = train._from_nchw(a.detach().cuda(), cs.cin_p)[0]
    got = train._colour_forward(a16, cs, wt.detach().cuda(), b.detach().cuda())
    assert got.shape == out.shape and rel(got, out.detach()) < 1e-3
    base = torch.randn(n, h, w, cs.cin_p)
    acc = base.clone().cuda()
    g_w, g_b = train._colour_backward(g.cuda(), a16, cs, wt.detach().cuda(), True, acc)
    assert rel(g_w, wt.grad) < 1e-3
    assert rel(g_b, b.grad) < 1e-3
    gx = (acc.cpu() - base)[..., :cin].permute(0, 3, 1, 2)
    assert rel(gx, a.grad) < 1e-3
    assert float((acc.cpu() - base)[..., cin:].abs().max()) == 0.0


def test_colour_layer_rejects_levels_not_above_the_padding(cae):
    from cnn_autoencoder_amd import train
    cs = train.ColourSpec(32, 3, 5, False)
    a16 = torch.zeros((1, 2, 8, 32), dtype=torch.bfloat16, device='cuda')
    with pytest.raises(ValueError, match='too small'):
        train._colour_forward(a16, cs, torch.zeros(3, 32, 5, 5, device='cuda'), None)


def _decoder(cae, seed, **kw):
    torch.manual_seed(seed)
    dec = cae.Synthesizer(multiscale_analysis=True, **kw)
    dec.cuda().train()
    return dec


def _restatement(dec, yq, act, bf16=True):
    """oracle.train_oracle.synthesis one unit at a time (+ the activation of non-last levels), a reflect-padded F.conv2d per
    colour layer on the level's output with bf16 operands and a bf16-rounded output gradient -> (x_r list, leaf params)"""
    from oracle import train_oracle as T
    from conftest import oracle_layers
    sd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    layers = oracle_layers({'decoder': sd, 'act_layer_type': act}, 'decoder')
    leaf = lambda t: None if t is None else t.detach().clone().requires_grad_(True)  # noqa: E731
    layers = [{k: leaf(v) for k, v in l.items() if k in ('weight', 'bias', 'beta', 'gamma', 'pre_weight', 'pre_bias')}
              for l in layers]
    L = len(layers)
    colours = [dict(weight=leaf(sd[f'color_layers.{i}.0.weight']), bias=leaf(sd.get(f'color_layers.{i}.0.bias')))
               for i in range(L - 1)]
    a = act if act in ('LeakyReLU', 'ReLU') else None
    fx, cols = yq, []
    for i, l in enumerate(layers):
        fx = T.synthesis(fx, [l], bf16=bf16, act=a)
        if i < L - 1:
            fx = T._act(fx, a)
            k = colours[i]['weight'].shape[-1]
            c = F.conv2d(F.pad(T._r(fx, bf16), (k // 2,) * 4, mode='reflect'), T._r(colours[i]['weight'], bf16),
                         colours[i]['bias'])
            cols.append(T._g(c, bf16))
    return [fx] + cols[::-1], layers, colours


def _check_parity(dec, layers, colours, yq, yq_dev, x_r, x_ref):
    """1e-3 of the largest magnitude; 2.5e-3 for a unit whose weight gradient sums over fewer than 256 input positions
    (single bf16 rounding flips show there, as in tests/test_train.py)"""
    n, _, lh, lw = yq.shape
    assert len(x_r) == len(x_ref)
    for got, want in zip(x_r, x_ref):
        assert got.shape == want.shape
        assert rel(got.detach(), want.detach()) < 1e-3
    assert rel(yq_dev.grad, yq.grad) < 1e-3
    grads = {n: p.grad.detach().cpu() for n, p in dec.named_parameters() if p.grad is not None}
    from test_train import _param_names
    for i, l in enumerate(layers):
        for key, sub in _param_names(l):
            if l.get(key) is not None:
                name = f'synthesis_track.{i}.{sub}'
                assert rel(grads[name], l[key].grad) < (1e-3 if n * lh * lw * 4 ** i >= 256 else 2.5e-3), name
    for i, c in enumerate(colours):
        assert rel(grads[f'color_layers.{i}.0.weight'], c['weight'].grad) < 1e-3, i
        if c['bias'] is not None:
            assert rel(grads[f'color_layers.{i}.0.bias'], c['bias'].grad) < 1e-3, i


@pytest.mark.parametrize('kw,shape,edge', [
    (dict(channels_org=3, channels_net=32, channels_bn=48, compression_level=3, act_layer_type='GDN'), (2, 5, 7), '1'),
    (dict(channels_org=3, channels_net=128, channels_bn=192, compression_level=4, act_layer_type='GDN'), (1, 4, 4), '1'),
    (dict(channels_org=3, channels_net=32, channels_bn=48, compression_level=3, act_layer_type='LeakyReLU', bias=True),
     (2, 5, 7), '1'),
    (dict(channels_org=3, channels_net=32, channels_bn=48, compression_level=3, act_layer_type='GDN', kernel_size=5, bias=True),
     (1, 6, 5), '1'),
    (dict(channels_org=1, channels_net=32, channels_bn=48, compression_level=3, act_layer_type='GDN'), (2, 5, 6), '1'),
    (dict(channels_org=3, channels_net=32, channels_bn=48, compression_level=3, act_layer_type='GDN', bias=True), (2, 5, 7), '0'),
])
def test_multiscale_decoder_gradients_match_the_restatement(cae, kw, shape, edge, monkeypatch):
    monkeypatch.setenv('CAE_EDGE_GEMM', edge)
    dec = _decoder(cae, 5, **kw)
    n, lh, lw = shape
    torch.manual_seed(2)
    yq = torch.round(3 * torch.randn(n, kw['channels_bn'], lh, lw)).requires_grad_(True)
    yq_dev = yq.detach().cuda().requires_grad_(True)
    x_r, _ = dec(yq_dev)
    L = kw['compression_level']
    assert len(x_r) == L and all(t is not None for t in x_r)
    gs = [torch.randn(t.shape) for t in x_r]
    torch.autograd.backward(list(x_r), [g.cuda() for g in gs])
    x_ref, layers, colours = _restatement(dec, yq, kw['act_layer_type'])
    torch.autograd.backward(x_ref, gs)
    _check_parity(dec, layers, colours, yq, yq_dev, x_r, x_ref)


def test_composed_colour_layers_equal_the_fused_ones(cae):
    """_ColourFn behind the units of a composed track against the colour layers inside SynthesisFn (same model)."""
    from cnn_autoencoder_amd import train
    kw = dict(channels_org=3, channels_net=32, channels_bn=48, compression_level=3, act_layer_type='GDN', bias=True)
    dec = _decoder(cae, 9, **kw)
    units = dec._units()
    torch.manual_seed(3)
    yq = torch.round(3 * torch.randn(2, 48, 5, 7)).cuda()
    res = {}
    for form in ('fused', 'composed'):
        dec.zero_grad(set_to_none=True)
        y = yq.clone().requires_grad_(True)
        if form == 'fused':
            x_r, _ = dec(y)
        else:
            specs, tensors = train._track_inputs(dec, units, True)
            colour, ctensors = train._colour_inputs(dec, units)
            out, cols = train._composed_track(units, y, True, colour, ctensors)
            x_r = [out] + cols[::-1]
        torch.manual_seed(4)
        torch.autograd.backward(list(x_r), [torch.randn(t.shape).cuda() for t in x_r])
        res[form] = ([t.detach().cpu() for t in x_r], y.grad.cpu(),
                     {n: p.grad.detach().cpu() for n, p in dec.named_parameters() if p.grad is not None})
    (xf, gf, pf), (xc, gc, pc) = res['fused'], res['composed']
    for a, b in zip(xf, xc):
        assert rel(b, a) < 1e-3
    assert rel(gc, gf) < 2e-3
    assert sorted(pf) == sorted(pc)
    for name in pf:
        assert rel(pc[name], pf[name]) < 2e-3, name


def test_multiscale_channel_plan_fails_as_in_inference(cae):
    dec = cae.Synthesizer(channels_org=3, channels_net=32, channels_bn=48, compression_level=3, channels_expansion=2,
                          act_layer_type='GDN', multiscale_analysis=True).cuda().train()
    with pytest.raises((NotImplementedError, RuntimeError, ValueError)):
        dec(torch.zeros(1, 48, 4, 4, device='cuda', requires_grad=True))


def test_twenty_multiscale_training_steps_follow_the_restatement(cae):
    """decoder-only training (fixed latents) with GeneralLoss('MultiscaleMSE') and a per-level lambda: the HIP decoder and
    the restatement run the same 20 Adam steps; the loss curves agree to rtol 2e-3 and the loss decreases."""
    from cnn_autoencoder_amd import criteria
    kw = dict(channels_org=3, channels_net=32, channels_bn=48, compression_level=3, act_layer_type='GDN')
    dec = _decoder(cae, 11, **kw)
    torch.manual_seed(12)
    x = torch.rand(2, 3, 80, 112)
    yq = torch.round(2 * torch.randn(2, 48, 10, 14))
    lam = [0.01, 0.005, 0.0025]
    crit = criteria.GeneralLoss('MultiscaleMSE', None, channels_org=3, compression_level=3, distortion_lambda=lam)
    opt = torch.optim.Adam(dec.parameters(), lr=1e-3)
    _, layers, colours = _restatement(dec, yq, 'GDN')
    ref_params = [t for l in layers for t in l.values() if t is not None] + \
                 [t for c in colours for t in c.values() if t is not None]
    ref_opt = torch.optim.Adam(ref_params, lr=1e-3)
    got, want = [], []
    xd, yd = x.cuda(), yq.cuda()
    for _ in range(20):
        x_r, _ = dec(yd)
        loss = crit(inputs=xd, outputs=dict(x_r=x_r))['loss']
        loss.backward()
        opt.step()
        opt.zero_grad()
        got.append(float(loss.detach()))
        x_ref, _, _ = _restatement_with(layers, colours, yq)
        ref_loss = crit(inputs=x, outputs=dict(x_r=x_ref))['loss']
        ref_loss.backward()
        ref_opt.step()
        ref_opt.zero_grad()
        want.append(float(ref_loss))
    np.testing.assert_allclose(got, want, rtol=2e-3)
    assert got[-1] < got[0]


def _restatement_with(layers, colours, yq):
    from oracle import train_oracle as T
    fx, cols = yq, []
    L = len(layers)
    for i, l in enumerate(layers):
        fx = T.synthesis(fx, [l], bf16=True)
        if i < L - 1:
            k = colours[i]['weight'].shape[-1]
            c = F.conv2d(F.pad(T._r(fx, True), (k // 2,) * 4, mode='reflect'), T._r(colours[i]['weight'], True),
                         colours[i]['bias'])
            cols.append(T._g(c, True))
    return [fx] + cols[::-1], layers, colours


@pytest.mark.parametrize('c_org', [1, 3])
@pytest.mark.parametrize('kind,edge', [('grouped', '1'), ('residual', '1'), ('residual', '0'), ('batch norm', '1')])
def test_composed_multiscale_decoders_match_float64(cae, kind, edge, c_org, monkeypatch):
    """Multiscale decoders on composed tracks (_ColourFn behind grouped, residual or batch-norm units; grouped colour layers
    with groups = channels_org): every kernel call replayed alone in float64 within its local bound, colour layers included
    (tests/train_replay.py), and every output, parameter gradient and the latent gradient as close to the float64 restatement
    (oracle.train_oracle.residual_track(levels=True) + reflect-padded colour convolutions) as the bf16 restatement is
    (train_replay.e2e_rule).  edge '0': the colour layers' padded stride-1 form."""
    from train_replay import e2e_rule, judge_track
    monkeypatch.setenv('CAE_EDGE_GEMM', edge)
    # (one image channel makes a grouped model a dense one, which takes the fused track: batch norm keeps it composed)
    kw = {'grouped': dict(channels_net=c_org, channels_bn=c_org, groups=True, bias=True, act_layer_type='ReLU',
                          batch_norm=c_org == 1),
          'residual': dict(channels_net=32, channels_bn=48, use_residual=True, act_layer_type='GDN'),
          'batch norm': dict(channels_net=32, channels_bn=48, batch_norm=True, bias=True, act_layer_type='LeakyReLU')}[kind]
    dec = _decoder(cae, 31 + c_org, channels_org=c_org, compression_level=3, **kw)
    with torch.no_grad():
        for m in dec.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)
    torch.manual_seed(6)
    yq = torch.round(3 * torch.randn(2, kw['channels_bn'], 4, 5))
    act = kw['act_layer_type']
    V, rows = judge_track(dec, dec.synthesis_track, yq, True, act if act in ('LeakyReLU', 'ReLU') else None)
    print(kind, c_org, V.summary())
    assert sum('colour' in k for k in V.ratios) > 0 and not V.failures, V.failures[:5]
    assert any(r[0].startswith('color_layers.') for r in rows) and sum(r[0].startswith('out ') for r in rows) == 3
    for row in rows:
        assert e2e_rule(row) != 'fail', row
