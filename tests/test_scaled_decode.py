"""Synthesis that stops at a level (cae_synthesis_scale): the image at 1 / 2^scale of the resolution, and the region /
scale reads of compressed slides built on it.  GPU tests, each on both arithmetic paths.

The colour layer of a scaled decode runs on color_small_kernel (<= 128 input, <= 4 image channels): fp32 FMA on the
level as the kernel reads it -- fp32 C8 rows, or hi + lo of the split rows on the f16x3 path -- with unsplit fp32 weights.
Its float64 replay is therefore the plain convolution of the observed input (the bridge of Synthesizer.forward, whose
units are launched identically) on BOTH paths, inside the convolution bound of tests/inference_replay.py
(C_CONV * 2^-24 * (|x| * |w| + |b|)).  Wider colour layers take the generic stride-1 launch + a uint8 conversion.
"""
import os

import numpy as np
import pytest
import torch

import inference_replay as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

RTOL = ATOL = 1e-4  # test_gpu_parity.test_variant_goldens


@pytest.fixture(params=['fp32', 'f16x3'], autouse=True)
def precision(request, monkeypatch):
    monkeypatch.setenv('CAE_PRECISION', request.param)
    return request.param


@pytest.fixture(scope='module')
def cae(built_lib):
    import cnn_autoencoder_amd as cae
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return cae


def multiscale_state(cfg, seed):
    """synth.synthetic_state + seeded colour layers (the synthetic state has none; a checkpoint must carry them)"""
    from cnn_autoencoder_amd import synth
    cfg = dict(cfg, multiscale_analysis=True)
    state = synth.synthetic_state(cfg, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    k, c_net, c_org = cfg.get('kernel_size', 3), cfg['channels_net'], cfg['channels_org']
    b = synth._xavier_bound(c_net, c_org, k)
    for i in range(cfg['compression_level'] - 1):
        state['decoder'][f'color_layers.{i}.0.weight'] = torch.from_numpy(
            rng.uniform(-b, b, (c_org, c_net, k, k)).astype(np.float32))
        if cfg.get('bias', False):
            state['decoder'][f'color_layers.{i}.0.bias'] = torch.from_numpy(
                rng.uniform(0.2, 0.6, (c_org,)).astype(np.float32))
    return state


def trunc_u8(x_nchw):
    return (x_nchw * 255.0).clip(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ reference goldens
@pytest.mark.parametrize('name', ['var_multiscale_gdn_k5_48x48', 'var_multiscale_lrelu_bias_40x56'])
def test_scaled_synthesis_matches_reference_golden(cae, name):
    from test_host import variant_modules
    g, cfg = load_golden(name)
    _, dec = variant_modules(cae, g, cfg)
    dec = dec.cuda()
    yq = torch.round(torch.from_numpy(g['y'])).cuda()
    for s in (1, 2):
        want = g[f'x_r_{s}']
        out = dec.forward_scale(yq, s)
        assert tuple(out.shape) == want.shape
        err = float(np.abs(out.cpu().numpy() - want).max())
        print(f'{name} scale {s}: max |err| {err:.3e}')
        np.testing.assert_allclose(out.cpu().numpy(), want, rtol=RTOL, atol=ATOL)
        # uint8 epilogue == truncating the same call's fp32 output, exactly
        u8 = dec.forward_scale_u8(yq, s)
        assert torch.equal(u8.cpu(), trunc_u8(out).cpu())
        # against the golden: within 1, and different only where 255 x sits within the 1e-4 tolerance of an integer
        v = 255.0 * want.astype(np.float64)
        ref = np.floor(np.clip(v, 0, 255)).transpose(0, 2, 3, 1)
        diff = np.abs(u8.cpu().numpy().astype(int) - ref.astype(int))
        near = (np.abs(v - np.rint(v)) <= 255.0 * 1e-4 * (1.0 + np.abs(want))).transpose(0, 2, 3, 1)
        print(f'{name} scale {s}: {int((diff > 0).sum())} uint8 values differ, {int(near.sum())} may')
        assert diff.max() <= 1
        assert not (diff > 0)[~near].any()


# ------------------------------------------------------------------------------------------------ float64 replay
def _colour_model(cae, c_org, c_net, k, bias, seed, L=2):
    torch.manual_seed(seed)
    dec = cae.Synthesizer(channels_org=c_org, channels_net=c_net, channels_bn=16, compression_level=L, kernel_size=k,
                          bias=bias, act_layer_type='GDN', multiscale_analysis=True)
    with torch.no_grad():
        for layer in list(dec.color_layers)[:-1]:
            if layer[0].bias is not None:
                layer[0].bias.uniform_(-0.5, 0.5)
    return dec.cuda().eval()


WORST = {}

# level sizes (rows, cols) = 2 x the latent's: at and around the 64 x 16 tile of color_small_kernel, several tiles, and
# the smallest levels (every level has even sizes: 2 x 6 and 4 x 6 stand for the 2 x 3 corner)
SIZES = [(8, 32), (7, 31), (9, 33), (16, 64), (17, 65), (1, 3), (2, 3)]


@pytest.mark.parametrize('k', [3, 5])
@pytest.mark.parametrize('bias', [False, True])
@pytest.mark.parametrize('c_org,c_net', [(1, 8), (3, 32), (4, 128), (3, 8), (1, 128), (4, 32), (3, 128)])
def test_colour_kernel_against_float64(cae, precision, k, bias, c_org, c_net):
    dec = _colour_model(cae, c_org, c_net, k, bias, seed=c_org * 1000 + c_net + k)
    conv = dec.color_layers[0][0]
    w, b = conv.dense_weight(), conv.bias
    gen = torch.Generator().manual_seed(k + c_net)
    for lh, lw in SIZES:
        if 2 * lh <= k // 2 or 2 * lw <= k // 2:
            continue
        for n in (1, 3):
            y = torch.round(4.0 * torch.randn(n, 16, lh, lw, generator=gen)).cuda()
            _, brg = dec(y)  # brg[0]: level 0 as the colour kernel reads it (f16x3: hi + lo of the split rows)
            ref, bound = R.conv_step(R.op_conv_s1(k), brg[0], w, b, False)
            # NaN-prefilled outputs: the allocator hands back the block just freed
            out = torch.full((n, c_org, 2 * lh, 2 * lw), float('nan'), device='cuda')
            del out
            got = dec.forward_scale(y, 1)
            assert tuple(got.shape) == (n, c_org, 2 * lh, 2 * lw)
            r = R.judge(got, ref, bound, f'colour k{k} {c_net}->{c_org} {2 * lh}x{2 * lw} n{n} {precision}')
            WORST[precision] = max(WORST.get(precision, 0.0), r)
            u8 = dec.forward_scale_u8(y, 1)
            assert torch.equal(u8.cpu(), trunc_u8(got).cpu())
            R.judge_u8(u8.permute(0, 3, 1, 2), ref, bound, 'colour u8')
    print(f'worst error / bound so far on {precision}: {WORST[precision]:.3f}')


def test_wide_colour_layer_takes_the_generic_launch(cae, precision):
    """192 input channels: not covered by color_small_kernel -> the generic colour launch of cae_synthesis_multiscale
    (bit-identical fp32 image: same kernel, same input) followed by the uint8 conversion kernel."""
    dec = _colour_model(cae, 3, 192, 3, True, seed=7)
    y = torch.round(4.0 * torch.randn(2, 16, 5, 9, generator=torch.Generator().manual_seed(1))).cuda()
    x_r, _ = dec(y)
    got = dec.forward_scale(y, 1)
    assert torch.equal(got, x_r[1]), 'path: generic colour launch'
    assert torch.equal(dec.forward_scale_u8(y, 1).cpu(), trunc_u8(got).cpu())
    print('wide colour layer: generic stride-1 launch + uint8 conversion kernel ran')


# ------------------------------------------------------------------------------------------------ consistency
def _small_codec(cae, tmp_path, seed=3, k=3, bias=True, L=3, c_net=32):
    cfg = dict(channels_org=3, channels_net=c_net, channels_bn=48, compression_level=L, kernel_size=k, bias=bias,
               act_layer_type='GDN')
    state = multiscale_state(cfg, seed)
    path = os.path.join(str(tmp_path), f'ckpt_{seed}.pth')
    torch.save(state, path)
    return cae.ConvolutionalAutoencoder(checkpoint=path), path, state


def test_scale_zero_symbols_and_workspace_reuse(cae, tmp_path):
    from cnn_autoencoder_amd.codec import _module
    codec, _, _ = _small_codec(cae, tmp_path)
    dec, eb = _module(codec._model['decoder']), _module(codec._model['fact_ent'])
    sym = torch.randint(-6, 7, (3, 48, 5, 7), dtype=torch.int32, generator=torch.Generator().manual_seed(0)).cuda()
    y = eb.dequantize_symbols(sym)
    base_u8 = dec.forward_u8(y).clone()
    # (the existing fp32 call with the same options: cae_synthesis without bridges -- asking for bridges, as
    #  Synthesizer.forward does, switches the f16x3 product-map form of the last two layers off)
    from cnn_autoencoder_amd import _lib
    full_f = lambda: dec._run(y, _lib.FMT_F32_NCHW, False)[0]
    base_f = full_f().clone()
    # scale 0 == the existing calls, bit for bit
    assert torch.equal(dec.forward_scale_u8(y, 0), base_u8)
    assert torch.equal(dec.forward_scale(y, 0), base_f)
    assert torch.equal(dec.forward_symbols_u8(sym, eb, scale=0), base_u8)
    L = 3
    for s in list(range(L)) + list(reversed(range(L))):
        u8 = dec.forward_scale_u8(y, s)
        assert tuple(u8.shape) == (3, 40 >> s, 56 >> s, 3)
        # the symbols entry == the latents entry on dequantised symbols
        assert torch.equal(dec.forward_symbols_u8(sym, eb, scale=s), u8)
        assert torch.equal(trunc_u8(dec.forward_scale(y, s)), u8)
        # a larger batch in between regrows the workspace for this scale only
        big = dec.forward_scale_u8(torch.cat([y, y, y]), s)
        assert torch.equal(big[3:6], u8)
        # ... and later scale-0 calls are unchanged
        assert torch.equal(dec.forward_u8(y), base_u8)
        assert torch.equal(full_f(), base_f)
    # scales agree with the colour outputs of the full multiscale call to summation order: 1e-4 relative with the
    # absolute floor scaled to the tensor, as test_variant_goldens states it (untrained IGDN stacks give |x| ~ 50, where
    # fp32 summation-order noise alone is ~1e-5 on elements that cancel to ~0)
    x_r, _ = dec(y)
    for s in (1, 2):
        want = x_r[s].cpu().numpy()
        np.testing.assert_allclose(dec.forward_scale(y, s).cpu().numpy(), want, rtol=RTOL,
                                   atol=ATOL * max(1.0, float(np.abs(want).max())))


def test_canonical_shape(cae, precision):
    from cnn_autoencoder_amd import synth
    from cnn_autoencoder_amd.codec import _module
    cfg = dict(synth.CANONICAL)
    state = multiscale_state(cfg, 0)
    model = cae.autoencoder_from_state_dict(state)
    dec = _module(model['decoder'])
    assert dec._dims[1:4] == (128, 192, 4)
    y = torch.round(3.0 * torch.randn(2, 192, 64, 64, generator=torch.Generator().manual_seed(5))).cuda()  # 2 x 1024^2
    x_r, brg = dec(y)
    for s in (1, 2, 3):
        got = dec.forward_scale(y, s)
        want = x_r[s]
        assert tuple(got.shape) == (2, 3, 1024 >> s, 1024 >> s)
        big = float(want.abs().max())
        print(f'canonical scale {s} {precision}: max |diff| {float((got - want).abs().max()):.3e}, max |x| {big:.3e}')
        conv = dec.color_layers[3 - s][0]
        ref, bound = R.conv_step(R.op_conv_s1(3), brg[3 - s], conv.dense_weight(), conv.bias, False)
        r = R.judge(got, ref, bound, f'canonical scale {s} {precision}')
        print(f'canonical scale {s} {precision}: error / bound {r:.3f}')
        # rtol 1e-4 against the generic launch's image.  The two kernels sum 1152 products in different orders, and the
        # synthetic state gives |x| up to ~2e3 with elements that cancel to ~0.1 (measured: max |diff| 5.9e-2 = 3e-5 of
        # the largest magnitude, on an element of 0.5), so the absolute floor is scaled to the tensor as
        # test_variant_goldens states it; every element is inside the float64 replay bound above.
        np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=RTOL, atol=ATOL * max(1.0, big))
        assert torch.equal(dec.forward_scale_u8(y, s).cpu(), trunc_u8(got).cpu())


def test_refusals(cae, tmp_path):
    from cnn_autoencoder_amd import synth
    from cnn_autoencoder_amd.codec import _module
    cfg = dict(channels_org=3, channels_net=32, channels_bn=48, compression_level=3, act_layer_type='GDN')
    plain = _module(cae.autoencoder_from_state_dict(synth.synthetic_state(cfg, seed=1))['decoder'])
    y = torch.round(4.0 * torch.randn(1, 48, 4, 4, generator=torch.Generator().manual_seed(2))).cuda()
    before = plain.forward_u8(y).clone()
    hd = plain._sync()
    prof_calls = lambda m: m.get_profile(reset=False)[1]
    plain.set_profiling(True)
    n0 = prof_calls(plain)
    with pytest.raises(ValueError, match='multiscale_analysis'):
        plain.forward_scale(y, 1)
    with pytest.raises(ValueError, match='outside 0..2'):
        plain.forward_scale_u8(y, 3)
    with pytest.raises(ValueError, match='outside 0..2'):
        plain.forward_scale(y, -1)
    # the library refuses by itself, before any launch (no profiled call is recorded)
    from cnn_autoencoder_amd import _lib
    out = torch.empty(1, 3, 16, 16, device='cuda')
    for s, msg in ((1, 'colour layer 1 not set'), (3, 'scale 3 outside'), (-1, 'scale -1 outside')):
        rc = _lib.lib().cae_synthesis_scale(hd.ptr, y.data_ptr(), 1, 4, 4, s, out.data_ptr(), _lib.FMT_F32_NCHW,
                                            _lib.stream_ptr())
        assert rc == -1 and msg in _lib.lib().cae_last_error().decode(), (s, _lib.lib().cae_last_error())
    assert prof_calls(plain) == n0, 'a refused call launched kernels'
    plain.set_profiling(False)
    assert torch.equal(plain.forward_u8(y), before)
    codec, _, _ = _small_codec(cae, tmp_path)
    dec = _module(codec._model['decoder'])
    y = torch.round(4.0 * torch.randn(1, 48, 4, 4, generator=torch.Generator().manual_seed(2))).cuda()
    before = dec.forward_u8(y).clone()
    for s in (3, -1, 1.5, True):
        with pytest.raises(ValueError):
            dec.forward_scale(y, s)
    with pytest.raises(ValueError):
        codec.decode_batch([b'\x00' * 32], scale=3)
    assert torch.equal(dec.forward_u8(y), before)


# ------------------------------------------------------------------------------------------------ slides
@pytest.fixture
def slide_store(cae, tmp_path, precision):
    from cnn_autoencoder_amd import synth, zarrio
    codec, path, state = _small_codec(cae, tmp_path, seed=11)
    P = 64
    h, w = 4 * P + 23, 2 * P + 40  # 5 x 3 chunks, ragged edges
    image = np.concatenate([np.concatenate([synth.histo_tile(P, 3 * i + j) for j in range(3)], 1)
                            for i in range(5)], 0)[:h, :w]
    store = os.path.join(str(tmp_path), 'slide.zarr')
    z = zarrio.compress_image('CAE', path, image, store, patch_size=P, batch_tiles=4)
    assert z.grid == (5, 3, 1)
    return store, path, state, image, P


ROIS = [(0, 64, 0, 64), (64, 128, 64, 128), (10, 200, 30, 150), (63, 65, 63, 65), (250, 279, 100, 168), (0, 279, 0, 168),
        (70, 71, 5, 160), (128, 128, 0, 10)]


def test_slide_regions_and_scales(cae, slide_store, precision, monkeypatch):
    from cnn_autoencoder_amd import zarrio
    store, path, state, image, P = slide_store
    z = zarrio.ZarrArray.open(store, '0/0')
    codec = z.codec
    whole = zarrio.decompress_image(store)
    assert whole.shape == image.shape
    L = 3
    reads = []
    real = zarrio.ZarrArray.read_chunk_bytes
    monkeypatch.setattr(zarrio.ZarrArray, 'read_chunk_bytes', lambda self, idx: (reads.append(tuple(idx)), real(self, idx))[1])
    for s in range(L):
        f = 2 ** s
        # mosaic of decode_batch(..., scale=s) tiles
        idxs = z.chunk_indices()
        tiles = codec.decode_batch([real(z, i) for i in idxs], scale=s)
        assert tiles.shape == (15, P // f, P // f, 3)
        mosaic = np.zeros((5 * P // f, 3 * P // f, 3), np.uint8)
        for (i, j, _), t in zip(idxs, tiles):
            mosaic[i * P // f:(i + 1) * P // f, j * P // f:(j + 1) * P // f] = t
        for roi in ROIS:
            y0, y1, x0, x1 = roi
            want = mosaic[y0 // f:max(y0 // f, -(-y1 // f)), x0 // f:max(x0 // f, -(-x1 // f))]
            reads.clear()
            got = zarrio.decompress_image(store, roi=roi, scale=s, batch_tiles=4)
            assert got.shape == want.shape and np.array_equal(got, want), (roi, s)
            touched = {(i, j, 0) for i in range(y0 // P, -(-y1 // P)) for j in range(x0 // P, -(-x1 // P))} \
                if y1 > y0 and x1 > x0 else set()
            assert sorted(reads) == sorted(touched), ('chunks decoded != chunks touched', roi, s)
            if s == 0:
                assert np.array_equal(got, whole[y0:y1, x0:x1]), roi
            dev = zarrio.decompress_image(store, roi=roi, scale=s, batch_tiles=4, coder='device')
            assert np.array_equal(dev, got), ('host and device coder differ', roi, s)
        # whole array at scale s, and read_region with a channel key
        assert np.array_equal(zarrio.decompress_image(store, scale=s),
                              mosaic[:-(-image.shape[0] // f), :-(-image.shape[1] // f)])
        assert np.array_equal(z.read_region((slice(10, 200), slice(30, 150), 1), scale=s),
                              mosaic[10 // f:-(-200 // f), 30 // f:-(-150 // f), 1])
    # region reads through __getitem__ (one chunk per decode call) give the same pixels
    assert np.array_equal(z[10:200, 30:150], whole[10:200, 30:150])


def test_bottleneck_store_regions_and_scales(cae, slide_store, precision):
    from cnn_autoencoder_amd import zarrio
    store, path, state, image, P = slide_store
    bn = store + '.bn'
    zarrio.compress_image('CAE', state, image, bn, patch_size=P, save_as_bottleneck=True, batch_tiles=4)
    for s in range(3):
        f = 2 ** s
        whole = zarrio.decompress_image(bn, checkpoint=state, scale=s, batch_tiles=4)
        assert whole.shape == (5 * P // f, 3 * P // f, 3)
        for roi in ROIS:
            y0, y1, x0, x1 = roi
            got = zarrio.decompress_image(bn, checkpoint=state, roi=roi, scale=s, batch_tiles=4)
            want = whole[y0 // f:max(y0 // f, -(-y1 // f)), x0 // f:max(x0 // f, -(-x1 // f))]
            assert got.shape == want.shape and np.array_equal(got, want), (roi, s)
