"""One handle, many calls: a result must not depend on what the handle's workspaces held before the call.

The workspaces of a model handle are never cleared; their rows have pitch that no kernel writes (C8S rows end in a
partly used 32-pixel group, C8SP rows in a partly used 64-pixel block) and the staging reads whole 256-byte runs and
16-channel chunks.  Every other GPU test runs one call on memory that nothing has used, which is usually zero: the one
value that hides a read of something the call did not write.

Each case here runs a clean call, then a dirtying call on the same module, then the clean call again:

    nan         the float entry with an all-NaN input at a covering shape (residue.covering_shape: every byte of a
                larger extent is written, with NaN)
    guard       (f16x3) an input that trips the range guard, so the workspaces end up in the fp32 repeat's layout
    other_path  a finite input at the covering shape on the other arithmetic path (the layers are re-packed twice)
    batch       three times the batch at the clean shape: only the sample stride moves

and asks that the clean call after it is bit-identical to the one before, finite, within the float64 bound of every unit
(test_inference_kernels._check_analysis / _check_synthesis, on the first call after a second dirtying call) and did not
fall back to fp32.  Three host paths (SlideCoder, the front door, cae_gdn_forward) get the same before / between / after.
"""
import numpy as np
import pytest
import torch

import test_inference_kernels as K
from residue import covering_shape

PRECISIONS = K.PRECISIONS
GDN = dict(act_layer_type='GDN')


def _kw(org, net, bn, L, k, **more):
    return dict(channels_org=org, channels_net=net, channels_bn=bn, compression_level=L, kernel_size=k, **more)


# (id, Analyzer kwargs, clean (n, h, w), entry, all four dirtying calls): sizes one pixel past / one short of a 32-pixel
# group and a 16-row tile; n = 2, so the last sample's over-read and the next sample's first plane are both in play
ANALYSIS = [
    ('gdn40_k3', _kw(3, 40, 16, 3, 3, **GDN), (2, 17, 33), 'levels', True),  # five planes: odd
    ('gdn72_k5', _kw(3, 72, 128, 3, 5, **GDN), (2, 12, 31), 'levels', False),  # nine planes
    ('gdn128_k3', _kw(3, 128, 40, 3, 3, **GDN), (2, 15, 65), 'levels', False),
    ('c192_k3', _kw(3, 192, 48, 3, 3, **GDN), (2, 16, 33), 'levels', True),  # stand-alone gdn_f16_kernel
    ('c192_k5_detour', _kw(3, 192, 48, 3, 5, **GDN), (2, 12, 17), 'levels', True),  # two layouts in one f16x3 call
    ('lrelu40_bias', _kw(3, 40, 16, 3, 3, act_layer_type='LeakyReLU', bias=True), (2, 17, 33), 'levels', True),
    ('res_gdn40', _kw(3, 40, 16, 3, 3, use_residual=True, **GDN), (2, 17, 32), 'levels', True),
    ('org1', _kw(1, 40, 16, 2, 3, **GDN), (2, 17, 33), 'levels', False),
    ('org4', _kw(4, 40, 16, 2, 3, **GDN), (2, 17, 33), 'levels', False),
    ('org8_converted', _kw(8, 40, 16, 2, 3, **GDN), (2, 17, 33), 'levels', False),
    ('gdn40_u8', _kw(3, 40, 16, 3, 3, **GDN), (2, 17, 33), 'u8', False),
    ('gdn32_u8_symbols', _kw(3, 32, 48, 2, 3, **GDN), (2, 17, 33), 'symbols', False),
]

# (id, Synthesizer kwargs, clean latents (n, lh, lw), entry, all four dirtying calls)
SYNTHESIS = [
    ('igdn40_k3', _kw(3, 40, 16, 3, 3, **GDN), (2, 4, 9), 'bridges', True),
    ('igdn40_k5', _kw(3, 40, 16, 3, 5, **GDN), (2, 2, 5), 'bridges', False),
    ('igdn128_k3', _kw(3, 128, 48, 2, 3, **GDN), (2, 8, 17), 'bridges', False),
    ('igdn128_k5', _kw(3, 128, 48, 3, 5, **GDN), (2, 4, 9), 'bridges', False),
    ('igdn192_k3', _kw(1, 192, 48, 2, 3, **GDN), (2, 8, 17), 'bridges', True),
    ('igdn192_k5', _kw(3, 192, 16, 2, 5, **GDN), (2, 2, 5), 'bridges', True),
    # stride-1 transposed convolutions with zero padding on C8SP rows: the most exposed
    ('lrelu40_bias', _kw(3, 40, 16, 3, 3, act_layer_type='LeakyReLU', bias=True), (2, 4, 9), 'bridges', True),
    ('res_gdn40', _kw(3, 40, 40, 2, 3, use_residual=True, **GDN), (2, 8, 17), 'bridges', True),
    ('res_relu40', _kw(3, 40, 16, 2, 3, act_layer_type='ReLU', use_residual=True, bias=True), (2, 2, 5), 'bridges', False),
    ('org4_edge', _kw(4, 40, 16, 2, 3, **GDN), (2, 4, 9), 'bridges', False),  # edge kernel without the product map
    ('product_map', _kw(3, 40, 16, 2, 3, **GDN), (2, 8, 17), 'no_bridges', False),
    ('colour_org3_k3', _kw(3, 32, 16, 3, 3, multiscale_analysis=True, **GDN), (2, 4, 9), 'bridges', False),
    ('colour_org1_k5', _kw(1, 40, 16, 3, 5, multiscale_analysis=True, **GDN), (2, 2, 5), 'bridges', False),
    ('scale1_u8', _kw(3, 32, 16, 3, 3, multiscale_analysis=True, **GDN), (2, 4, 9), 'scale1_u8', False),
    ('scale2_u8', _kw(3, 32, 16, 3, 3, multiscale_analysis=True, **GDN), (2, 2, 5), 'scale2_u8', False),
    ('symbols_u8', _kw(3, 32, 48, 2, 3, **GDN), (2, 8, 17), 'symbols_u8', False),
]

DIRTY = ('nan', 'guard', 'other_path', 'batch')


def _matrix(cases):
    """every model with `nan` on both paths; the other three dirtying calls on the models marked for them (guard: f16x3)"""
    out = []
    for case in cases:
        for dirty in DIRTY if case[4] else DIRTY[:1]:
            for precision in PRECISIONS:
                if dirty == 'guard' and precision != 'f16x3':
                    continue
                out.append(pytest.param(case, dirty, precision, id=f'{case[0]}-{dirty}-{precision}'))
    return out


def test_every_case_has_a_covering_shape():
    """(no GPU) the dirtying shape of every case below writes whole rows, is nowhere smaller than the clean call and has
    at least twice its bytes at every level: covering_shape asserts it"""
    for track, cases in (('analysis', ANALYSIS), ('synthesis', SYNTHESIS)):
        for name, kw, clean, _, _ in cases:
            dirty = covering_shape(track, clean, kw['compression_level'], kw['kernel_size'])
            assert dirty[0] == clean[0] and dirty[1] >= clean[1] and dirty[2] >= clean[2], name
            # a few MB at most: (n, channels, rows, columns) of the largest level in fp32
            last = 2 ** (kw['compression_level'] - 1) if track == 'synthesis' else 1
            assert dirty[0] * kw['channels_net'] * dirty[1] * dirty[2] * last * last * 4 <= 16 << 20, name
    assert len(_matrix(ANALYSIS)) + len(_matrix(SYNTHESIS)) >= 100


# ------------------------------------------------------------------------------------------------- the sequence
def _other(precision):
    return 'fp32' if precision == 'f16x3' else 'f16x3'


def _entropy(bn):
    from cnn_autoencoder_amd import entropy
    eb = entropy.EntropyBottleneck(bn).cuda()
    with torch.no_grad():
        eb.quantiles[:, 0, 1] += torch.linspace(-0.4, 0.4, bn, device=eb.quantiles.device)
    eb.update(force=True)
    return eb


def _flat(out):
    """every tensor of an entry's result, in order"""
    if isinstance(out, torch.Tensor):
        return [out]
    return [t for o in out if o is not None for t in _flat(o)]


def _sequence(mod, clean, dirty, check, guard):
    """clean, dirty, clean: bit-identical, finite, no fallback; dirty again, then the float64 bound of every unit on the
    first call after it"""
    with torch.no_grad():
        first = _flat(clean())
        assert mod.fp32_fallbacks == 0
        dirty()
        torch.cuda.synchronize()
        if guard:
            assert mod.fp32_fallbacks == 1, 'the dirtying call did not trip the range guard'
        mod.fp32_fallbacks = 0  # (an all-NaN input trips the guard as well)
        again = _flat(clean())
        torch.cuda.synchronize()
        assert mod.fp32_fallbacks == 0, 'the clean call fell back to fp32 after the dirtying call'
        assert len(again) == len(first)
        for i, (a, b) in enumerate(zip(first, again)):
            assert a.dtype == b.dtype and a.shape == b.shape
            assert not a.dtype.is_floating_point or bool(torch.isfinite(b).all()), f'output {i} is not finite'
            assert torch.equal(a, b), f'output {i} changed with the call before it ({int((a != b).sum())} elements)'
        dirty()
        mod.fp32_fallbacks = 0
    check()
    assert mod.fp32_fallbacks == 0


@pytest.mark.gpu
@pytest.mark.parametrize('case,dirty,precision', _matrix(ANALYSIS))
def test_analysis_does_not_depend_on_the_call_before(built_lib, case, dirty, precision):
    name, kw, (n, h, w), entry, _ = case
    enc = K._analyzer(precision, seed=len(name), **kw)
    c, L, ks = kw['channels_org'], kw['compression_level'], kw['kernel_size']
    g = torch.Generator().manual_seed(11)
    if entry == 'levels':
        x = torch.rand(n, c, h, w, generator=g).cuda()
        clean = lambda: enc.forward_levels(x)  # noqa: E731
    else:
        x = torch.randint(0, 256, (n, h, w, c), generator=g, dtype=torch.uint8).cuda()
        if entry == 'u8':
            clean = lambda: enc.forward_u8(x)  # noqa: E731
        else:
            eb = _entropy(kw['channels_bn'])
            clean = lambda: enc.forward_u8_symbols(x, eb)  # noqa: E731
    _, dh, dw = covering_shape('analysis', (n, h, w), L, ks)
    if dirty == 'batch':
        xd = torch.rand(3 * n, c, h, w, generator=g).cuda()
    else:
        xd = torch.rand(n, c, dh, dw, generator=g)
        if dirty == 'nan':
            xd.fill_(float('nan'))
        elif dirty == 'guard':
            xd[0, 0, 3, 4] = 7.0e4  # beyond the f16 range
        xd = xd.cuda()

    def dirtying():
        if dirty == 'other_path':
            enc.precision = _other(precision)
        try:
            enc(xd)
        finally:
            enc.precision = precision
    _sequence(enc, clean, dirtying, lambda: K._check_analysis(enc, x, f'{name} after {dirty}'), dirty == 'guard')


@pytest.mark.gpu
@pytest.mark.parametrize('case,dirty,precision', _matrix(SYNTHESIS))
def test_synthesis_does_not_depend_on_the_call_before(built_lib, case, dirty, precision):
    name, kw, (n, lh, lw), entry, _ = case
    dec = K._synthesizer(precision, seed=len(name), **kw)
    bn, L, ks = kw['channels_bn'], kw['compression_level'], kw['kernel_size']
    g = torch.Generator().manual_seed(12)
    yq = torch.randn(n, bn, lh, lw, generator=g) * 2
    yq_dev = yq.cuda()
    bridges = entry != 'no_bridges'
    if entry in ('bridges', 'no_bridges'):
        clean = lambda: dec(yq_dev, bridges=bridges)  # noqa: E731
    elif entry.startswith('scale'):
        clean = lambda: dec.forward_scale_u8(yq_dev, int(entry[5]))  # noqa: E731
    else:
        eb = _entropy(bn)
        sym = torch.round(yq).int().cuda()
        clean = lambda: dec.forward_symbols_u8(sym, eb)  # noqa: E731
    _, dh, dw = covering_shape('synthesis', (n, lh, lw), L, ks)
    if dirty == 'batch':
        yd = torch.randn(3 * n, bn, lh, lw, generator=g) * 2
    else:
        yd = torch.randn(n, bn, dh, dw, generator=g) * 2
        if dirty == 'nan':
            yd.fill_(float('nan'))
        elif dirty == 'guard':
            yd[0, 0, 1, 1] = 7.0e4
    yd = yd.cuda()

    def dirtying():
        if dirty == 'other_path':
            dec.precision = _other(precision)
        try:
            dec(yd, bridges=bridges)
        finally:
            dec.precision = precision
    colours = bool(kw.get('multiscale_analysis'))
    _sequence(dec, clean, dirtying, lambda: K._check_synthesis(dec, yq, f'{name} after {dirty}', colours),
              dirty == 'guard')


# ------------------------------------------------------------------------------------------------- host paths
@pytest.mark.gpu
def test_slide_coder_batches_do_not_depend_on_the_batch_before(built_lib):
    """SlideCoder.compress / decompress of a 3-tile batch of 64 x 96 before and after a 3-tile batch of 128 x 256 through
    the same coder: identical payloads, identical tiles"""
    import cnn_autoencoder_amd as cae
    from cnn_autoencoder_amd import slide, synth
    state = synth.synthetic_state(dict(synth.CANONICAL, channels_net=32, channels_bn=48), seed=6)
    coder = slide.SlideCoder(cae.ConvolutionalAutoencoder(checkpoint=state))
    small = torch.from_numpy(synth.uniform_tiles(3, 64, 96, seed=1)).cuda()
    large = torch.from_numpy(synth.uniform_tiles(3, 128, 256, seed=2)).cuda()
    p0 = [bytes(b) for b in coder.compress(small)]
    r0 = coder.decompress(p0, 64, 96).clone()
    pl = coder.compress(large)
    assert coder.decompress(pl, 128, 256).shape == (3, 128, 256, 3)
    p1 = [bytes(b) for b in coder.compress(small)]
    r1 = coder.decompress(p1, 64, 96)
    assert p1 == p0
    assert torch.equal(r1, r0)


@pytest.mark.gpu
def test_front_door_calls_do_not_depend_on_the_calls_before(built_lib):
    """codec.encode / decode of one 64 x 96 tile before and after a 128 x 256 tile and a tile that trips the range guard
    (an activation-free model with large first-layer weights, as tests/test_range_guard.py builds it: bright tiles
    overflow the f16 range, dark ones do not): identical bytes, identical pixels"""
    import cnn_autoencoder_amd as cae
    from cnn_autoencoder_amd import synth
    cfg = dict(synth.CANONICAL, channels_net=32, channels_bn=48, compression_level=3, act_layer_type=None)
    state = synth.synthetic_state(cfg, seed=15)
    state['encoder']['analysis_track.0.model.0.weight'] *= 5.0e4
    state['encoder']['analysis_track.2.model.0.weight'] *= 2.0e-5
    codec = cae.ConvolutionalAutoencoder(checkpoint=state)
    assert codec._model['encoder'].module.precision_code() == 1
    rng = np.random.default_rng(5)
    tile = rng.integers(0, 12, (64, 96, 3), dtype=np.uint8)
    dark = rng.integers(0, 12, (128, 256, 3), dtype=np.uint8)
    bright = rng.integers(200, 256, (128, 256, 3), dtype=np.uint8)
    repeats = lambda: int(codec._front_door().stats()['fp32_repeats'])  # noqa: E731
    try:
        b0 = codec.encode(tile)
        r0 = np.array(codec.decode(b0))
        codec.decode(codec.encode(dark))
        assert repeats() == 0
        codec.decode(codec.encode(bright))
        tripped = repeats()
        assert tripped >= 1, 'the bright tile did not trip the range guard'
        b1 = codec.encode(tile)
        r1 = np.array(codec.decode(b1))
        assert repeats() == tripped, 'the clean call fell back to fp32 after the guard-tripping one'
    finally:
        codec.close()
    assert b1 == b0
    assert np.array_equal(r1, r0)


@pytest.mark.gpu
@pytest.mark.parametrize('inverse', [False, True])
def test_gdn_forward_does_not_depend_on_the_call_before(built_lib, inverse):
    """cae_gdn_forward at 40 channels (five planes of a 64-channel layer): the same result before and after an all-NaN
    call at a covering shape, and within the existing 1e-4 of the oracle"""
    from oracle import cae_oracle as O
    kw = _kw(3, 40, 40, 2, 3, **GDN)
    mod = (K._synthesizer if inverse else K._analyzer)('fp32', seed=3, **kw)
    gdn = (mod.synthesis_track if inverse else mod.analysis_track)[0].model[1]
    shape = (2, 9, 13)
    x = torch.randn(shape[0], 40, *shape[1:], generator=torch.Generator().manual_seed(13))
    _, dh, dw = covering_shape('analysis', shape, 0, 1)
    with torch.no_grad():
        first = gdn(x.cuda())
        gdn(torch.full((shape[0], 40, dh, dw), float('nan')).cuda())
        again = gdn(x.cuda())
    assert bool(torch.isfinite(again).all())
    assert torch.equal(again, first)
    ref = O.gdn_forward(x, gdn.beta.detach(), gdn.gamma.detach(), inverse=inverse)
    np.testing.assert_allclose(again.cpu().numpy(), ref.numpy(), rtol=1e-4, atol=1e-4)
