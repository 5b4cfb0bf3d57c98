"""Every inference unit against float64, on both arithmetic paths, from the GPU's own input to that unit.

The analysis track is observed unit by unit through cae_analysis_levels, the synthesis track through its bridges and
colour outputs; each unit is replayed alone in float64 and judged with the condition-aware bound of
tests/inference_replay.py (the constants C_CONV and C_NORM, and what was observed, are documented there).  The cases
go where the kernels' routes and indexing change: the fused first layer, the interior strided kernels at 1, 2, 4 and 6
channel tiles, the k = 5 192-channel fp32 detour, the stand-alone GDN kernel, stride-1 stages (reflect and zero
padding, residual units, the fp32 stage route above 128 channels), the last layers (NCHW, uint8, product map) and the
colour layers; sizes 1 and 2 rows above the padding, widths around the 32-pixel row groups and heights around the
16-row tiles, batches of 1 and 3.

test_inference_judge_rejects_wrong_kernels (no GPU) shows that the bound rejects subtly wrong kernels.
"""
import math
import os

import numpy as np
import pytest
import torch

import inference_replay as R

PRECISIONS = ['fp32', 'f16x3']


# ----------------------------------------------------------------------------------------------------- judge (CPU)
def _emulate_f16x3_conv(x, w, b, k, seed, mutate=None, tile=(slice(0, 16), slice(0, 16), slice(0, 32))):
    """one f16x3 strided reflect convolution as the kernel computes it: split operands, three f16 products per term
    (exact in fp32), fp32 accumulation in 16-term steps in a shuffled order, bias in the epilogue; `mutate` plants
    one defect (`tile`: the output rows, columns and channels of 'drop_al_bh_on_one_tile')"""
    P = k // 2
    xh, xl = (t.float().numpy() for t in R.split(x))
    wh, wl = (t.float().numpy() for t in R.split(w))
    bb = b.float().numpy()
    if mutate == 'zero_lo_plane':
        xl[:, 3] = 0.0

    def cols(a, mode):
        ap = np.pad(a, ((0, 0), (0, 0), (P, P), (P, P)), mode=mode)
        n, c, hp, wp = ap.shape
        oh, ow = (hp - k) // 2 + 1, (wp - k) // 2 + 1
        out = np.empty((n, oh, ow, c, k, k), np.float32)
        for ky in range(k):
            for kx in range(k):
                out[..., ky, kx] = ap[:, :, ky:ky + 2 * oh:2, kx:kx + 2 * ow:2].transpose(0, 2, 3, 1)
        return out.reshape(n, oh, ow, -1)

    def run(xh, xl, mode):
        ch, cl = cols(xh, mode), cols(xl, mode)
        Wh, Wl = wh.reshape(wh.shape[0], -1), wl.reshape(wl.shape[0], -1)
        terms = np.concatenate([ch[..., None, :] * Wh, ch[..., None, :] * Wl, cl[..., None, :] * Wh], -1)
        if mutate == 'drop_al_bh_on_one_tile':  # the xl * wh products of output tile (32 channels, 16 x 16 pixels)
            kk = Wh.shape[1]
            terms[:, tile[0], tile[1], tile[2], 2 * kk:] = 0.0
        perm = np.random.default_rng(seed).permutation(terms.shape[-1])
        terms = terms[..., perm]
        acc = np.zeros(terms.shape[:-1], np.float32)
        for t in range(0, terms.shape[-1], 16):
            acc = (acc + terms[..., t:t + 16].sum(-1, dtype=np.float32)).astype(np.float32)
        bias = np.broadcast_to(bb, acc.shape).copy()
        if mutate == 'skip_bias_on_padded_rows':  # output rows whose window reaches into the padding
            bias[:, 0] = 0.0
            bias[:, -1] = 0.0
        return (acc + bias).transpose(0, 3, 1, 2)

    out = run(xh, xl, 'edge' if mutate == 'clamp_instead_of_reflect' else 'reflect')
    if mutate == 'shift_last_ragged_column':  # the last output column reads its window one pixel to the right
        sh = lambda a: np.concatenate([a[..., 1:], a[..., -2:-1]], -1)  # noqa: E731
        out[..., -1] = run(sh(xh), sh(xl), 'reflect')[..., -1]
    return torch.from_numpy(out).double()


MUTATIONS = ['drop_al_bh_on_one_tile', 'zero_lo_plane', 'shift_last_ragged_column', 'clamp_instead_of_reflect',
             'skip_bias_on_padded_rows']


def test_inference_judge_rejects_wrong_kernels():
    """The f16x3 convolution bound passes a faithful emulation of the kernel's arithmetic and fails each planted defect
    (40 -> 40 channels: two channel tiles, ragged; k = 3; 17 x 33: odd rows, one pixel past a 32-pixel row group)."""
    g = torch.Generator().manual_seed(0)
    cin, cout, k = 40, 40, 3
    x = torch.rand(1, cin, 17, 33, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    b = (torch.rand(cout, generator=g) - 0.5) * 0.1
    ref, B = R.conv_step(R.op_conv_s2(k), x, w, b, f16=True)
    for seed in range(3):
        assert R.ratio(_emulate_f16x3_conv(x, w, b, k, seed), ref, B) <= 1.0, seed
    for mut in MUTATIONS:
        r = R.ratio(_emulate_f16x3_conv(x, w, b, k, 0, mut), ref, B)
        if os.environ.get('CAE_TEST_VERBOSE'):
            print(f'{mut}: err / bound {r:.1f}')
        assert r > 1.0, (mut, r)


def test_split_model_matches_the_documented_contract():
    """hi = f16(v), lo = f16(v - hi): |v - (hi + lo)| <= max(2^-22 |v|, 2^-25), and the relative error of small values
    is far above 2^-22 (lo is subnormal below |v| = 2^-3)"""
    v = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, 1 << 18).astype(np.float32))
    v = torch.cat([v * s for s in (1.0, 0.25, 0.06, 0.01, 1e-3, 1e-4)]).double()
    hi, lo = R.split(v)
    err = (v - hi - lo).abs()
    assert bool((err <= torch.maximum(R.SPLIT_REL * v.abs(), torch.full_like(v, R.SPLIT_ABS))).all())
    small = (v.abs() > 5e-4) & (v.abs() < 1e-3)
    assert float((err[small] / v[small].abs()).max()) > 2.0 ** -16


# ----------------------------------------------------------------------------------------------------- GPU helpers
def _cae():
    import cnn_autoencoder_amd as cae
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return cae


def _realistic(mod, seed):
    """weights at realistic magnitudes (std 1/sqrt(fan-in): |w| ~ 0.01-0.05 at 40-128 channels), small biases, beta
    near 1 and gamma = 0.1 I (gdn_init_params) plus small off-diagonal entries"""
    from cnn_autoencoder_amd.modules import GDN, _ConvParams
    from oracle import cae_oracle as O
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, _ConvParams):
                k = m.kernel_size
                fan = m.weight.shape[0] * k * k / 4 if m.transposed else m.weight.shape[1] * k * k
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / math.sqrt(fan))
                if m.bias is not None:
                    m.bias.copy_((torch.rand(m.bias.shape, generator=g) - 0.5) * 0.1)
            elif isinstance(m, GDN):
                c = m.in_channels
                beta_eff = 1.0 + 0.2 * torch.rand(c, generator=g)
                gamma_eff = 0.1 * torch.eye(c) + 0.004 * torch.rand(c, c, generator=g) * (1 - torch.eye(c))
                m.beta.copy_(O.nonneg_init(beta_eff))  # (the parametrisation gives back beta_eff, gamma_eff)
                m.gamma.copy_(O.nonneg_init(gamma_eff))
    return mod


def _analyzer(precision, seed=0, **kw):
    cae = _cae()
    torch.manual_seed(seed)
    enc = _realistic(cae.Analyzer(**kw), seed).eval()
    enc.precision = precision
    return enc


def _synthesizer(precision, seed=0, **kw):
    cae = _cae()
    torch.manual_seed(seed)
    dec = _realistic(cae.Synthesizer(**kw), seed).eval()
    dec.precision = precision
    return dec


def _check_analysis(enc, x, route):
    f16 = enc.precision_code() == 1
    with torch.no_grad():
        y, levels = enc.forward_levels(x)
    torch.cuda.synchronize()
    assert enc.fp32_fallbacks == 0
    units = enc._units()
    assert len(levels) == len(units) - 1
    inp = (x.double() / 255.0).float().permute(0, 3, 1, 2) if x.dtype == torch.uint8 else x
    outs = list(levels) + [y]
    for i, u in enumerate(units):
        last = i == len(units) - 1
        assert outs[i].shape[1] == u.main.out_channels  # padded channels never leave the library
        ref, B = R.replay_unit(u, inp if i == 0 else outs[i - 1], enc._dims[4], False, f16, not last)
        R.judge(outs[i], ref, B, f'{route} unit {i} ({enc.precision})')
    return y, levels


def _check_synthesis(dec, yq, route, colours=False):
    f16 = dec.precision_code() == 1
    with torch.no_grad():
        x_r, brg = dec(yq.cuda())
    torch.cuda.synchronize()
    assert dec.fp32_fallbacks == 0
    units, ks = dec._units(), dec._dims[4]
    for i, u in enumerate(units):
        last = i == len(units) - 1
        assert brg[i].shape[1] == u.main.out_channels
        ref, B = R.replay_unit(u, yq if i == 0 else brg[i - 1], ks, True, f16, not last)
        R.judge(brg[i], ref, B, f'{route} unit {i} ({dec.precision})')
    if colours:
        L = len(units)
        for i in range(L - 1):
            conv = dec.color_layers[i][0]
            cf16 = f16 and conv.out_channels <= 32
            ref, B = R.conv_step(R.op_conv_s1(ks), brg[i], conv.dense_weight(), conv.bias, cf16)
            R.judge(x_r[L - 1 - i], ref, B, f'{route} colour {i} ({dec.precision})')


# ----------------------------------------------------------------------------------------------------- analysis
# (id, Analyzer kwargs, (n, h, w), uint8 input)
ANALYSIS = [
    # fused first layer (conv_first[_f16]): 1 / 3 / 4 image channels, k 3 / 5, GDN / none, 32 and 40 outputs
    ('first_c1_k3_gdn_32', dict(channels_org=1, channels_net=32, channels_bn=16, compression_level=2, kernel_size=3,
                                act_layer_type='GDN'), (1, 17, 33), False),
    ('first_c3_k5_gdn_40_u8', dict(channels_org=3, channels_net=40, channels_bn=16, compression_level=2, kernel_size=5,
                                   act_layer_type='GDN'), (3, 16, 31), True),
    ('first_c4_k3_none_40', dict(channels_org=4, channels_net=40, channels_bn=16, compression_level=2, kernel_size=3),
     (1, 15, 65), False),
    ('first_c4_k5_none_32_u8', dict(channels_org=4, channels_net=32, channels_bn=48, compression_level=2,
                                    kernel_size=5), (1, 6, 32), True),
    ('first_c1_k5_gdn_40_u8', dict(channels_org=1, channels_net=40, channels_bn=16, compression_level=2, kernel_size=5,
                                   act_layer_type='GDN'), (1, 33, 17), True),
    # LeakyReLU units: the stride-1 pre-convolution (reflect) in front of every layer, first layer included
    ('lrelu_c3_k3_32', dict(channels_org=3, channels_net=32, channels_bn=16, compression_level=2, kernel_size=3,
                            act_layer_type='LeakyReLU', bias=True), (3, 17, 32), False),
    ('lrelu_c1_k5_40_u8', dict(channels_org=1, channels_net=40, channels_bn=16, compression_level=2, kernel_size=5,
                               act_layer_type='LeakyReLU', bias=True), (1, 16, 33), True),
    # more than 4 image channels: layout conversion + the interior kernel as the first layer
    ('c8_first_40', dict(channels_org=8, channels_net=40, channels_bn=16, compression_level=2, kernel_size=3,
                         act_layer_type='GDN'), (1, 17, 31), False),
    ('c8_first_40_u8', dict(channels_org=8, channels_net=40, channels_bn=16, compression_level=2, kernel_size=5,
                            act_layer_type='GDN'), (1, 16, 33), True),
    # conv_s2[_f16] interior: cout 16 / 40 / 72 / 128 (CT 1, 2, 4, 4 ragged), cin 16 / 40 / 128, k 3 / 5
    ('int_16to16_k3_gdn_last72', dict(channels_org=3, channels_net=16, channels_bn=72, compression_level=3,
                                      kernel_size=3, act_layer_type='GDN'), (1, 31, 65), False),
    ('int_40to40_k5_lrelu_last16', dict(channels_org=3, channels_net=40, channels_bn=16, compression_level=3,
                                        kernel_size=5, act_layer_type='LeakyReLU', bias=True), (1, 17, 33), False),
    ('int_128to128_k3_none_last40', dict(channels_org=3, channels_net=128, channels_bn=40, compression_level=3,
                                         kernel_size=3, bias=True), (3, 15, 16), False),
    ('int_72to72_k5_gdn_last128', dict(channels_org=3, channels_net=72, channels_bn=128, compression_level=3,
                                       kernel_size=5, act_layer_type='GDN'), (1, 12, 31), False),
    ('int_40to40_k3_relu_last48', dict(channels_org=3, channels_net=40, channels_bn=48, compression_level=3,
                                       kernel_size=3, act_layer_type='ReLU', bias=True), (1, 6, 33), False),
    # 192 outputs: k = 3 CT 6 + gdn_f16_kernel; k = 5 the fp32 detour (conv_f16_fits false); last layers 48 / 192
    ('c192_k3_gdn_last48', dict(channels_org=3, channels_net=192, channels_bn=48, compression_level=3, kernel_size=3,
                                act_layer_type='GDN'), (1, 16, 33), False),
    ('c192_k5_gdn_detour_last48', dict(channels_org=3, channels_net=192, channels_bn=48, compression_level=3,
                                       kernel_size=5, act_layer_type='GDN'), (1, 12, 17), False),
    ('last192_k3', dict(channels_org=3, channels_net=32, channels_bn=192, compression_level=2, kernel_size=3,
                        act_layer_type='GDN'), (3, 17, 31), False),
    # residual units: stride-1 reflect stages with GDN at 40 and 128 channels, 160 (stages on the fp32 kernels),
    # LeakyReLU residual (two stages + post activation)
    ('res_gdn_40', dict(channels_org=3, channels_net=40, channels_bn=16, compression_level=3, kernel_size=3,
                        act_layer_type='GDN', use_residual=True), (1, 17, 32), False),
    ('res_gdn_128_k5', dict(channels_org=3, channels_net=128, channels_bn=16, compression_level=3, kernel_size=5,
                            act_layer_type='GDN', use_residual=True), (1, 12, 16), False),
    ('res_gdn_160_fp32_stages', dict(channels_org=3, channels_net=160, channels_bn=16, compression_level=3,
                                     kernel_size=3, act_layer_type='GDN', use_residual=True), (1, 15, 17), False),
    ('res_lrelu_40', dict(channels_org=3, channels_net=40, channels_bn=16, compression_level=3, kernel_size=3,
                          act_layer_type='LeakyReLU', use_residual=True, bias=True), (3, 9, 33), False),
]


@pytest.mark.gpu
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('case', ANALYSIS, ids=[c[0] for c in ANALYSIS])
def test_analysis_units_against_float64(built_lib, case, precision):
    name, kw, (n, h, w), u8 = case
    enc = _analyzer(precision, seed=len(name), **kw)
    g = torch.Generator().manual_seed(1)
    c = kw['channels_org']
    if u8:
        x = torch.randint(0, 256, (n, h, w, c), generator=g, dtype=torch.uint8).cuda()
    else:
        x = torch.rand(n, c, h, w, generator=g).cuda()
    _check_analysis(enc, x, name)


@pytest.mark.gpu
@pytest.mark.parametrize('precision', PRECISIONS)
def test_levels_do_not_change_the_latents(built_lib, precision):
    """cae_analysis_levels launches the same kernels as cae_analysis: bit-identical latents, also on the detour route"""
    for kw in (dict(channels_org=3, channels_net=40, channels_bn=48, compression_level=3, act_layer_type='GDN'),
               dict(channels_org=3, channels_net=192, channels_bn=48, compression_level=3, kernel_size=5,
                    act_layer_type='GDN')):
        enc = _analyzer(precision, **kw)
        x = torch.rand(2, 3, 33, 40, generator=torch.Generator().manual_seed(2)).cuda()
        with torch.no_grad():
            y0 = enc(x)
            y1, levels = enc.forward_levels(x)
        assert torch.equal(y0, y1)
        assert [tuple(t.shape) for t in levels] == [(2, kw['channels_net'], 17, 20), (2, kw['channels_net'], 9, 10)]


@pytest.mark.gpu
@pytest.mark.parametrize('precision', PRECISIONS)
def test_analysis_symbols_are_the_rounded_float_latents(built_lib, precision):
    """the _symbols epilogue (48 and 192 latent channels): round(y - median) of the float output, bit-exact"""
    from cnn_autoencoder_amd import entropy
    for bn in (48, 192):
        enc = _analyzer(precision, channels_org=3, channels_net=32, channels_bn=bn, compression_level=2,
                        act_layer_type='GDN')
        eb = entropy.EntropyBottleneck(bn).cuda()
        with torch.no_grad():
            eb.quantiles[:, 0, 1] += torch.linspace(-0.4, 0.4, bn, device=eb.quantiles.device)
        eb.update(force=True)
        x = torch.randint(0, 256, (3, 17, 33, 3), generator=torch.Generator().manual_seed(3), dtype=torch.uint8).cuda()
        with torch.no_grad():
            y = enc.forward_u8(x)
            sym = enc.forward_u8_symbols(x, eb)
            med = eb.quantiles[:, 0, 1].detach().float().view(1, -1, 1, 1)
        assert torch.equal(sym, torch.round(y - med).int())


# ----------------------------------------------------------------------------------------------------- synthesis
# (id, Synthesizer kwargs, (n, lh, lw), colour layers)
SYNTHESIS = [
    # deconv_s2[_f16] + IGDN at 40 / 128 / 192 channels, k 3 / 5; last layer deconv_last[_f16] (bridges on)
    ('igdn_40_k3', dict(channels_org=3, channels_net=40, channels_bn=16, compression_level=3, kernel_size=3,
                        act_layer_type='GDN'), (1, 4, 9), False),
    ('igdn_128_k5', dict(channels_org=3, channels_net=128, channels_bn=48, compression_level=3, kernel_size=5,
                         act_layer_type='GDN'), (1, 4, 8), False),
    ('igdn_192_k3', dict(channels_org=1, channels_net=192, channels_bn=48, compression_level=2, kernel_size=3,
                         act_layer_type='GDN'), (3, 8, 17), False),
    ('igdn_192_k5', dict(channels_org=3, channels_net=192, channels_bn=16, compression_level=2, kernel_size=5,
                         act_layer_type='GDN'), (1, 8, 16), False),
    # 4-channel output: the last-layer edge kernel without the product map
    ('last_c4_k3', dict(channels_org=4, channels_net=40, channels_bn=16, compression_level=2, kernel_size=3,
                        act_layer_type='GDN'), (1, 9, 16), False),
    # stride-1 transposed convolutions (zero padding on C8SP rows): LeakyReLU pre-convolutions, residual units
    ('lrelu_40_k3', dict(channels_org=3, channels_net=40, channels_bn=16, compression_level=3, kernel_size=3,
                         act_layer_type='LeakyReLU', bias=True), (1, 4, 9), False),
    ('res_gdn_40', dict(channels_org=3, channels_net=40, channels_bn=40, compression_level=2, kernel_size=3,
                        act_layer_type='GDN', use_residual=True), (1, 8, 17), False),
    ('res_gdn_128_k5', dict(channels_org=3, channels_net=128, channels_bn=128, compression_level=2, kernel_size=5,
                            act_layer_type='GDN', use_residual=True), (1, 4, 8), False),
    ('res_gdn_160_fp32_stages', dict(channels_org=3, channels_net=160, channels_bn=160, compression_level=2,
                                     kernel_size=3, act_layer_type='GDN', use_residual=True), (1, 4, 9), False),
    ('res_relu_40', dict(channels_org=3, channels_net=40, channels_bn=16, compression_level=2, kernel_size=3,
                         act_layer_type='ReLU', use_residual=True, bias=True), (3, 8, 8), False),
    # multiscale colour layers, 1 and 3 image channels, k 3 / 5
    ('colour_c3_k3', dict(channels_org=3, channels_net=32, channels_bn=16, compression_level=3, kernel_size=3,
                          act_layer_type='GDN', multiscale_analysis=True), (1, 4, 9), True),
    ('colour_c1_k5', dict(channels_org=1, channels_net=40, channels_bn=16, compression_level=3, kernel_size=5,
                          act_layer_type='GDN', multiscale_analysis=True), (3, 2, 5), True),
]


@pytest.mark.gpu
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('case', SYNTHESIS, ids=[c[0] for c in SYNTHESIS])
def test_synthesis_units_against_float64(built_lib, case, precision):
    name, kw, (n, lh, lw), colours = case
    dec = _synthesizer(precision, seed=len(name), **kw)
    yq = torch.randn(n, kw['channels_bn'], lh, lw, generator=torch.Generator().manual_seed(4)) * 2
    _check_synthesis(dec, yq, name, colours)


@pytest.mark.gpu
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('c_org,ks,net', [(3, 3, 128), (1, 3, 40), (3, 5, 40), (4, 3, 32)])
def test_last_two_synthesis_layers_without_bridges(built_lib, precision, c_org, ks, net):
    """No bridges: on f16x3 with k = 3 and <= 3 image channels layer L-2 writes the product map and the last layer is
    pmap_gather (judged together from the latents: IGDN output bound through |W_last|, its split, the <= 4-term sum);
    else the deconv_last kernels.  Float and uint8 outputs (u8 == trunc(clip(255 ref)) away from integer boundaries)."""
    from cnn_autoencoder_amd import _lib
    dec = _synthesizer(precision, seed=5, channels_org=c_org, channels_net=net, channels_bn=16, compression_level=2,
                       kernel_size=ks, act_layer_type='GDN')
    f16 = dec.precision_code() == 1
    yq = torch.randn(3, 16, 9, 16, generator=torch.Generator().manual_seed(6)) * 2
    with torch.no_grad():
        out, _, _ = dec._run(yq.cuda(), _lib.FMT_F32_NCHW, False)
        u8 = dec.forward_u8(yq.cuda())
    torch.cuda.synchronize()
    assert dec.fp32_fallbacks == 0
    u0, u1 = dec._units()
    y, By = R.replay_unit(u0, yq, ks, True, f16, True)
    w, b = u1.effective_main()
    ref, B = R.conv_step(R.op_deconv_s2(ks), y, w, b, f16, By)
    route = f'last_two_c{c_org}_k{ks}' + ('_pmap' if f16 and ks == 3 and c_org <= 3 else '')
    R.judge(out, ref, B, f'{route} ({precision})')
    R.judge_u8(u8.permute(0, 3, 1, 2), ref, B, f'{route} u8 ({precision})')


# ----------------------------------------------------------------------------------------------------- f16x3 contract
@pytest.mark.gpu
def test_f16x3_accuracy_model_under_power_of_two_scaling(built_lib):
    """One GDN layer with w, b scaled by 2^-s and beta by 2^-2s computes the same function.  fp32: every s within the
    C_CONV bound.  f16x3: the error against float64 on the UNSPLIT operands stays within the per-operand model
    max(2^-22 |v|, 2^-25) at every s, and grows with s (small weights lose relative accuracy: lo is subnormal)."""
    import torch.nn.functional as F
    kw = dict(channels_org=40, channels_net=40, channels_bn=16, compression_level=2, kernel_size=3,
              act_layer_type='GDN', bias=True)
    x = torch.rand(1, 40, 17, 33, generator=torch.Generator().manual_seed(7))
    E = lambda v: torch.maximum(R.SPLIT_REL * v.abs(), torch.full_like(v, R.SPLIT_ABS))  # noqa: E731
    op = R.op_conv_s2(3)
    errs = {}
    for precision in PRECISIONS:
        for s in (0, 4, 8, 12):
            enc = _analyzer(precision, seed=8, **kw)
            u = enc._units()[0]
            with torch.no_grad():
                u.main.weight.mul_(2.0 ** -s)
                u.main.bias.mul_(2.0 ** -s)
                beta_eff, gamma_eff = u.gdn.effective()
                from oracle import cae_oracle as O
                u.gdn.beta.copy_(O.nonneg_init(beta_eff * 2.0 ** (-2 * s)))  # (s = 12: clamped at beta_min 1e-6)
                _, levels = enc.forward_levels(x.cuda())
            torch.cuda.synchronize()
            got = levels[0]
            w, b = u.effective_main()
            beta, gamma = u.gdn.effective()
            if precision == 'fp32':
                ref, B = R.replay_unit(u, x, 3, False, False, True)
                R.judge(got, ref, B, f'gdn scaled 2^-{s} (fp32)')
                continue
            # float64 on the unsplit operands, and the corrected model's bound
            xd, wd, bd = x.double(), w.double(), b.double()
            z = op(xd, wd) + bd.view(1, -1, 1, 1)
            S = op(xd.abs(), wd.abs()) + bd.abs().view(1, -1, 1, 1)
            Bz = (op(E(xd), wd.abs()) + op(xd.abs(), E(wd)) + op(E(xd), E(wd)) + R.SPLIT_REL * S
                  + R.C_CONV * R.U * S)
            y, By = R.gdn_step(z, Bz, beta, gamma, False, False)
            g = gamma.double()[:, :, None, None]
            N = F.conv2d(z * z, g, beta.double())
            dN = F.conv2d(z * z, E(g))  # gamma's split
            By = R.store_split(y, By + z.abs() * dN / (2 * N ** 1.5))
            err = float((got.double().cpu() - y).abs().max())
            errs[s] = err
            R.judge(got, y, By, f'gdn scaled 2^-{s} (f16x3 vs unsplit)')
    if os.environ.get('CAE_TEST_VERBOSE'):
        print('f16x3 max |err| per s:', {s: f'{e:.2e}' for s, e in errs.items()})
    assert errs[12] > 16 * errs[0], errs  # the old "22 significant bits" wording would keep these equal


# ----------------------------------------------------------------------------------------------------- small levels
@pytest.mark.gpu
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('ks,L,h', [(5, 2, 3), (3, 3, 2)])
def test_levels_not_above_the_reflect_padding_raise(built_lib, precision, ks, L, h):
    """k = 5, L = 2, h = 3 (level 1 input: 2 rows) and k = 3, L = 3, h = 2 (level 1 input: 1 row): F.pad(mode='reflect')
    rejects these in the reference; inference refuses them before any launch, as training does"""
    enc = _analyzer(precision, channels_org=3, channels_net=32, channels_bn=16, compression_level=L, kernel_size=ks,
                    act_layer_type='GDN')
    with pytest.raises(ValueError, match='too small for reflect padding'):
        enc(torch.rand(1, 3, h, 24).cuda())
    with pytest.raises(ValueError, match='too small for reflect padding'):
        enc.forward_u8(torch.zeros(1, h, 24, 3, dtype=torch.uint8).cuda())
    y = enc(torch.rand(1, 3, 2 ** (L - 1) * (ks // 2) + 1, 24).cuda())  # one row above the padding at the last level
    assert bool(torch.isfinite(y).all())


@pytest.mark.gpu
def test_colour_layers_not_above_the_reflect_padding_raise(built_lib):
    dec = _synthesizer('fp32', channels_org=3, channels_net=32, channels_bn=16, compression_level=2, kernel_size=5,
                       act_layer_type='GDN', multiscale_analysis=True)
    with pytest.raises(ValueError, match='too small for reflect padding'):
        dec(torch.randn(1, 16, 1, 4).cuda())
