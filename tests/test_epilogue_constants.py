"""Bias and beta as the conv / deconv epilogues read them: whole channel tiles in 16-byte pieces, from HBM or from LDS.

The kernels fetch the per-channel vectors of a channel tile as four aligned groups of four floats in accumulator order
(load_acc_tile, cae_kernels.hpp); deconv_s2_f16_kernel keeps a copy of both in LDS.  An indexing mistake there moves a
channel's bias or beta to another channel, so every case gives each channel its own bias (0.002 (c + 1), alternating
sign) and beta (1 + 0.01 (c + 1)), a dense gamma and a batch of 2, and judges the layer against its float64
restatement within the bound tests/test_inference_kernels.py uses for that layer (inference_replay): neighbouring
channels differ by 0.004 in bias and by 1 % in beta, thousands of times the bound.

Shapes: transposed layers at 1, 2, 4 channel tiles with and without IGDN on one full block (8 x 32 inputs), on partial
rows / columns with a stray column (9 x 33) and on less than one block (3 x 5), the product-map form at 128 -> 3;
strided layers at the same widths with and without GDN on 34 x 66 and 5 x 7 inputs; 192 channels (6 tiles, the
normalisation as a kernel of its own) once each way.  Host vectors that are not 16-byte aligned at the C ABI are
handled: the library pads them into device buffers of its own.
"""
import numpy as np
import pytest
import torch

import inference_replay as R
from test_inference_kernels import PRECISIONS, _analyzer, _check_analysis, _check_synthesis, _synthesizer


def _distinct_channels(mod):
    """every bias and beta distinct per channel (gamma is dense already: _realistic)"""
    from cnn_autoencoder_amd.modules import GDN, _ConvParams
    from oracle import cae_oracle as O
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, _ConvParams) and m.bias is not None:
                c = torch.arange(1, m.bias.numel() + 1, dtype=torch.float32)
                m.bias.copy_(0.002 * c * (1 - 2 * (c % 2)))
            elif isinstance(m, GDN):
                c = torch.arange(1, m.in_channels + 1, dtype=torch.float32)
                m.beta.copy_(O.nonneg_init(1.0 + 0.01 * c))
    return mod


def _latents(n, c, h, w, seed):
    return torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(seed)) * 2


@pytest.mark.gpu
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('hw', [(8, 32), (9, 33), (3, 5)], ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('igdn', [True, False], ids=['igdn', 'plain'])
@pytest.mark.parametrize('net', [32, 64, 128])
def test_transposed_layer_constants(built_lib, net, igdn, hw, precision):
    """unit 0 = deconv_s2[_f16] 16 -> net (+ IGDN) on an hw input, unit 1 the last layer; both judged"""
    dec = _distinct_channels(_synthesizer(precision, seed=net, channels_org=3, channels_net=net, channels_bn=16,
                                          compression_level=2, kernel_size=3, bias=True,
                                          act_layer_type='GDN' if igdn else None))
    _check_synthesis(dec, _latents(2, 16, *hw, seed=7), f'deconv_{net}_{"igdn" if igdn else "plain"}_{hw[0]}x{hw[1]}')


@pytest.mark.gpu
@pytest.mark.parametrize('precision', PRECISIONS)
def test_product_map_constants(built_lib, precision):
    """128 -> 3 without bridges on 9 x 33: on f16x3 layer L-2 (bias, IGDN) leaves as the product map and the last layer
    is the gather; judged together from the latents, as test_last_two_synthesis_layers_without_bridges does"""
    from cnn_autoencoder_amd import _lib
    dec = _distinct_channels(_synthesizer(precision, seed=11, channels_org=3, channels_net=128, channels_bn=16,
                                          compression_level=2, kernel_size=3, bias=True, act_layer_type='GDN'))
    f16 = dec.precision_code() == 1
    yq = _latents(2, 16, 9, 33, seed=8)
    with torch.no_grad():
        out, _, _ = dec._run(yq.cuda(), _lib.FMT_F32_NCHW, False)
        u8 = dec.forward_u8(yq.cuda())
    torch.cuda.synchronize()
    assert dec.fp32_fallbacks == 0
    u0, u1 = dec._units()
    y, By = R.replay_unit(u0, yq, 3, True, f16, True)
    w, b = u1.effective_main()
    ref, B = R.conv_step(R.op_deconv_s2(3), y, w, b, f16, By)
    R.judge(out, ref, B, f'pmap_128_9x33 ({precision})')
    R.judge_u8(u8.permute(0, 3, 1, 2), ref, B, f'pmap_128_9x33 u8 ({precision})')


@pytest.mark.gpu
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('hw', [(34, 66), (5, 7)], ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('gdn', [True, False], ids=['gdn', 'plain'])
@pytest.mark.parametrize('net', [32, 64, 128])
def test_strided_layer_constants(built_lib, net, gdn, hw, precision):
    """unit 0 = conv_s2[_f16] net -> net (+ GDN) on an hw input of net channels (more than 4 image channels: the
    interior kernel is the first layer), unit 1 the last layer; both judged"""
    enc = _distinct_channels(_analyzer(precision, seed=net + 1, channels_org=net, channels_net=net, channels_bn=16,
                                       compression_level=2, kernel_size=3, bias=True,
                                       act_layer_type='GDN' if gdn else None))
    x = torch.rand(2, net, *hw, generator=torch.Generator().manual_seed(9)).cuda()
    _check_analysis(enc, x, f'conv_{net}_{"gdn" if gdn else "plain"}_{hw[0]}x{hw[1]}')


@pytest.mark.gpu
@pytest.mark.parametrize('precision', PRECISIONS)
def test_192_channels_each_way(built_lib, precision):
    """6 channel tiles: the convolution without the normalisation, then gdn_f16_kernel (beta from its LDS copy)"""
    enc = _distinct_channels(_analyzer(precision, seed=3, channels_org=3, channels_net=192, channels_bn=48,
                                       compression_level=3, kernel_size=3, bias=True, act_layer_type='GDN'))
    _check_analysis(enc, torch.rand(2, 3, 20, 36, generator=torch.Generator().manual_seed(10)).cuda(), 'conv_192')
    dec = _distinct_channels(_synthesizer(precision, seed=4, channels_org=3, channels_net=192, channels_bn=16,
                                          compression_level=2, kernel_size=3, bias=True, act_layer_type='GDN'))
    _check_synthesis(dec, _latents(2, 16, 9, 33, seed=12), 'deconv_192')


@pytest.mark.gpu
@pytest.mark.parametrize('precision', PRECISIONS)
def test_misaligned_host_vectors_are_handled(built_lib, precision):
    """cae_model_set_layer with bias and beta at host addresses 4 bytes off a 16-byte boundary: the layer computes,
    bit for bit, what it computed from aligned vectors (64 channels: two tiles, IGDN, the 9 x 33 case)"""
    from cnn_autoencoder_amd import _lib
    dec = _distinct_channels(_synthesizer(precision, seed=5, channels_org=3, channels_net=64, channels_bn=16,
                                          compression_level=2, kernel_size=3, bias=True, act_layer_type='GDN'))
    yq = _latents(2, 16, 9, 33, seed=13).cuda()
    with torch.no_grad():
        _, brg0 = dec(yq)
    torch.cuda.synchronize()
    u0 = dec._units()[0]
    wt, bt = u0.effective_main()
    be, ga = u0.gdn.effective()
    w = np.ascontiguousarray(wt.cpu().numpy(), dtype=np.float32)
    gamma = np.ascontiguousarray(ga.float().cpu().numpy())

    def off_by_4(t):
        v = t.detach().float().cpu().numpy()
        store = np.zeros(v.size + 8, np.float32)
        k = next(i for i in range(1, 5) if (store.ctypes.data + 4 * i) % 16 == 4)
        store[k:k + v.size] = v
        return store, store[k:k + v.size]

    keep_b, b = off_by_4(bt)
    keep_beta, beta = off_by_4(be)
    assert b.ctypes.data % 16 == 4 and beta.ctypes.data % 16 == 4
    hd = dec._sync()
    _lib.check(_lib.lib().cae_model_set_layer(hd.ptr, dec._track_id, 0, u0.main.in_channels, u0.main.out_channels,
                                              w.ctypes.data, b.ctypes.data, beta.ctypes.data, gamma.ctypes.data))
    with torch.no_grad():
        _, brg1 = dec(yq)
    torch.cuda.synchronize()
    assert dec.fp32_fallbacks == 0
    assert torch.equal(brg0[0], brg1[0])
    ref, B = R.replay_unit(u0, yq, 3, True, dec.precision_code() == 1, True)
    R.judge(brg1[0], ref, B, f'misaligned host vectors ({precision})')
