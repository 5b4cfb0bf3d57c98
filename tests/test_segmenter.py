"""The segmentation head on the GPU (cnn_autoencoder_amd/segmenters.py, csrc/cae_kernels_seg.hpp).

Per step: every convolution is replayed alone in float64 from the kernel's own (tapped) input and the tapped (a, b)
pairs, inside inference_replay.conv_step's f16x3 bound with C_CONV as it stands; every (a, b) is judged by its effect
a x + b against float64 statistics of the tapped plane (segmenter_restatement.stat_ratio, C_STAT).
End to end: max|gpu - f64| <= 4 max|f32 restatement - f64| + 1e-6 max|f64| on the logits.
tests/test_segmenter_host.py shows that these bounds reject wrong kernels.  CAE_TEST_VERBOSE=1 prints every ratio.
"""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inference_replay as R
import segmenter_restatement as SR

pytestmark = pytest.mark.gpu

A = SR.GOLDEN_CONFIGS['a'][0]
CANON = dict(channels_bn=192, channels_net=128, seg_channels_net=64, seg_channels_expansion=2, seg_channels_bn=1024,
             compression_level=4, concat_bridges=True)
VERBOSE = bool(os.environ.get('CAE_TEST_VERBOSE'))


def _seg():
    from cnn_autoencoder_amd import segmenters
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return segmenters


def _tile():
    from cnn_autoencoder_amd import _lib
    tx, ty = ctypes.c_int(), ctypes.c_int()
    _lib.lib().cae_seg_tile(ctypes.byref(tx), ctypes.byref(ty))
    return tx.value, ty.value


def _model(cfg, seed=0):
    """a JNet on the device in eval mode: torch's default initialisation from the seed, gamma / beta drawn around 1 / 0"""
    S = _seg()
    torch.manual_seed(seed)
    m = S.JNet(**cfg)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.GroupNorm):
                mod.weight.copy_(1.0 + 0.5 * torch.randn(mod.weight.shape, generator=g))
                mod.bias.copy_(0.3 * torch.randn(mod.bias.shape, generator=g))
    return m.cuda().eval()


def _inputs(cfg, lh, lw, n, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    L = cfg['compression_level']
    y_q = torch.round(3.0 * torch.randn(n, cfg['channels_bn'], lh, lw, generator=g))
    ch = [cfg.get('channels_net', 64)] * (L - 1) + [cfg.get('channels_org', 3)]
    brg = [torch.rand(n, c, lh * 2 ** (i + 1), lw * 2 ** (i + 1), generator=g) for i, c in enumerate(ch)]
    return y_q.cuda(), ([b.cuda() for b in brg] if cfg.get('concat_bridges') else None)


def _check(m, cfg, y_q, brg, what):
    """one tapped call: every step, every (a, b), the logits end to end -> logits"""
    y0, b0 = y_q.clone(), [b.clone() for b in brg or []]
    with torch.no_grad():
        logits, taps = m(y_q, brg, taps=True)
    assert torch.equal(y_q, y0) and all(torch.equal(p, q) for p, q in zip(brg or [], b0)), 'the head wrote its inputs'
    plan, raw, ab, bab = taps['plan'], taps['raw'], taps['ab'], taps['bridge_ab']
    worst_stat = 0.0

    def stat(pairs, x, norm, name):
        nonlocal worst_stat
        c = x.shape[1]
        assert not bool(pairs[:, c:].abs().sum()) or norm is None  # padding channels: (0, 0)
        r = SR.stat_ratio(pairs[:, :c, 0], pairs[:, :c, 1], x, None if norm is None else norm.weight,
                          None if norm is None else norm.bias)
        if VERBOSE:
            print(f'{what} {name}: statistics ratio {r:.3f}')
        assert r <= SR.C_STAT, (what, name, r)
        worst_stat = max(worst_stat, r)

    for s, st in enumerate(plan):
        parts = []
        for src in st['srcs']:
            if src[0] == 'latent':
                parts.append(y_q.cpu())
            elif src[0] == 'bridge':
                i = src[1]
                c = brg[i].shape[1]
                bn1 = m.bridges_projection[i]._bn1
                stat(bab[i], brg[i], bn1 if cfg.get('batch_norm', True) else None, f'bridge {i}')
                parts.append(SR.staged(brg[i], bab[i][:, :c, 0], bab[i][:, :c, 1]))
            elif src[2]:
                c = raw[src[1]].shape[1]
                parts.append(SR.staged(raw[src[1]], ab[src[1]][:, :c, 0], ab[src[1]][:, :c, 1]))
            else:
                parts.append(raw[src[1]].cpu())
        v = torch.cat(parts, dim=1)
        if st['up']:
            op = lambda x, k: F.conv_transpose2d(x, k, stride=2)
        else:
            op = lambda x, k: F.conv2d(x, k, padding=k.shape[-1] // 2)
        ref, B = R.conv_step(op, v, st['weight'], st['bias'], f16=True)
        R.judge(raw[s], ref, B, f"{what} {st['name']}")
        if st['has_ab']:
            stat(ab[s], raw[s], st['norm'], st['name'])
    assert torch.equal(raw[-1], logits)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    f64, _ = SR.jnet(sd, cfg, y_q, brg, torch.float64)
    f32, _ = SR.jnet(sd, cfg, y_q, brg, torch.float32)
    err, bound = float((logits.cpu().double() - f64).abs().max()), SR.e2e_bound(f32, f64)
    if VERBOSE:
        print(f'{what}: logits err {err:.3e}, bound {bound:.3e}, worst statistics ratio {worst_stat:.3f}')
    assert err <= bound, (what, err, bound)
    return logits


# ---------------------------------------------------------------------------------------------------------- (A)
def test_golden_configuration():
    """(A): the reference's state dict and inputs (latents 3 x 5, batch 2); the logits also against the golden ones"""
    S = _seg()
    cfg, sd, y_q, brg, golden, _ = SR.load_golden('a')
    m = S.JNet(**cfg)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    logits = _check(m, cfg, y_q.cuda(), [b.cuda() for b in brg], 'A')
    f64, _ = SR.jnet(sd, cfg, y_q, brg, torch.float64)
    f32, _ = SR.jnet(sd, cfg, y_q, brg, torch.float32)
    assert float((logits.cpu().double() - golden.double()).abs().max()) <= 2 * SR.e2e_bound(f32, f64)  # both sides' error


# ---------------------------------------------------------------------------------------------------------- (B)
@pytest.mark.parametrize('snet', [5, 12])
def test_concat_boundaries_off_the_plane_grid(snet):
    """(B): seg_channels_net = 5 puts the concat boundaries at 20 | 20, 10 | 10 and 5 | 5; 12 at 48 | 48, 24 | 24, 12 | 12"""
    cfg = dict(A, seg_channels_net=snet)
    _check(_model(cfg, 1), cfg, *_inputs(cfg, 3, 5, 2, 1), f'B{snet}')


# ---------------------------------------------------------------------------------------------------------- (C)
@pytest.mark.parametrize('offset', [False, True])
def test_one_pixel_planes_and_offset_inputs(offset):
    """(C): latents 1 x 1, batch 3: one-pixel planes in the bottleneck (mean == x, var == 0), four-pixel planes above;
    with `offset` the latents carry a constant offset and the bridges have mean 100, standard deviation 0.01"""
    m = _model(A, 2)
    y_q, brg = _inputs(A, 1, 1, 3, 2)
    if offset:
        y_q = y_q + 50.0
        brg = [100.0 + 0.01 * torch.randn(b.shape, generator=torch.Generator().manual_seed(5)).cuda() for b in brg]
    with torch.no_grad():
        _, taps = m(y_q, brg, taps=True)
    # one-pixel planes: a = gamma / sqrt(eps), b = beta - x a, exactly
    bn1 = m.bottleneck._bn1
    x = taps['raw'][0][:, :, 0, 0]
    rstd = float(np.float32(1.0) / np.sqrt(np.float32(SR.EPS)))
    a = (bn1.weight.detach() * rstd).expand_as(x)
    c = x.shape[1]
    assert torch.equal(taps['ab'][0][:, :c, 0], a)
    assert torch.equal(taps['ab'][0][:, :c, 1], (bn1.bias.detach().double() - x.double() * a.double()).float())  # one fma
    _check(m, A, y_q, brg, f'C offset={offset}')


# ---------------------------------------------------------------------------------------------------------- (D)
@pytest.mark.parametrize('lh,lw', [(2, 2), (1, 3)])
def test_canonical_widths(lh, lw):
    """(D): 192 / 128 / 64 / 1024, four levels: many output-channel groups, contractions up to 2048 channels"""
    _check(_model(CANON, 3), CANON, *_inputs(CANON, lh, lw, 1, 3), f'D {lh}x{lw}')


# ---------------------------------------------------------------------------------------------------------- (E)
def _edge_sizes():
    """one level, so the full-resolution size is twice the latent size: latent sizes one below, at and one above the
    output tile (the bottleneck's planes) and half of it (the full-resolution planes: two pixels below / at / above)"""
    try:
        tx, ty = _tile()
    except Exception:  # the library is not built: the tests fail at import of the package, not at collection
        tx, ty = 16, 8
    return [(ty + d, tx + d) for d in (-1, 0, 1)] + [(ty // 2 + d, tx // 2 + d) for d in (-1, 0, 1)]


@pytest.mark.parametrize('lh,lw', _edge_sizes())
def test_sizes_around_the_output_tile(lh, lw):
    """(E)"""
    cfg = dict(channels_bn=12, channels_net=10, seg_channels_net=6, seg_channels_bn=20, compression_level=1, num_classes=2,
               concat_bridges=True)
    _check(_model(cfg, 4), cfg, *_inputs(cfg, lh, lw, 2, 4), f'E {lh}x{lw}')


# ---------------------------------------------------------------------------------------------------------- (F)
@pytest.mark.parametrize('concat', [False, True])
@pytest.mark.parametrize('bn', [False, True])
@pytest.mark.parametrize('classes', [1, 5])
def test_variants(concat, bn, classes):
    """(F)"""
    cfg = dict(A, concat_bridges=concat, batch_norm=bn, num_classes=classes)
    _check(_model(cfg, 5), cfg, *_inputs(cfg, 2, 3, 2, 5), f'F concat={concat} bn={bn} classes={classes}')


# ---------------------------------------------------------------------------------------------------------- (G)
def test_valid_range():
    """(G): a staged value beyond f16 fails the call loudly, its twin inside does not; NaN raises; gamma beyond f16 is
    refused at upload"""
    S = _seg()
    m = _model(A, 6)
    y_q, brg = _inputs(A, 3, 5, 2, 6)
    with torch.no_grad():
        bad = y_q.clone()
        bad[1, 7, 2, 3] = 1.1 * 65504.0
        with pytest.raises(FloatingPointError, match='65504'):
            m(bad, brg)
        ok = y_q.clone()
        ok[1, 7, 2, 3] = 0.9 * 65504.0
        out, _ = m(ok, brg)
        assert bool(torch.isfinite(out).all())
        nan = [b.clone() for b in brg]
        nan[1][0, 3, 5, 7] = float('nan')
        with pytest.raises(FloatingPointError):
            m(y_q, nan)
        out2, _ = m(y_q, brg)  # the handle is usable after a failed call
        assert bool(torch.isfinite(out2).all())
        big = _model(A, 6)
        big.synthesis_track[1]._bn1.weight.data[2] = 1.0e5
        with pytest.raises(ValueError, match='f16 range'):
            big(y_q, brg)


# ---------------------------------------------------------------------------------------------------------- (H)
def test_call_independence():
    """(H): clean / dirty / clean on one handle: bitwise equal logits with a call of another (larger) shape in between
    that leaves NaN in every workspace; the inputs are unchanged"""
    m = _model(A, 7)
    y_q, brg = _inputs(A, 3, 5, 2, 7)
    y0, b0 = y_q.clone(), [b.clone() for b in brg]
    with torch.no_grad():
        first, _ = m(y_q, brg)
        other, _ = m(*_inputs(A, 2, 2, 1, 8))  # another shape
        second, _ = m(y_q, brg)
        y_d, b_d = _inputs(A, 5, 7, 3, 9)  # larger at every level: covers what the clean call uses
        y_d[:] = float('nan')
        b_d = [torch.full_like(b, float('nan')) for b in b_d]
        with pytest.raises(FloatingPointError):
            m(y_d, b_d)
        third, _ = m(y_q, brg)
    assert torch.equal(first, second) and torch.equal(first, third) and bool(torch.isfinite(third).all())
    assert torch.equal(y_q, y0) and all(torch.equal(p, q) for p, q in zip(brg, b0))
    assert other.shape == (1, 3, 16, 16)


# ---------------------------------------------------------------------------------------------------------- (I)
def _codec(seed=0):
    import cnn_autoencoder_amd as cae
    from cnn_autoencoder_amd import synth
    cfg = dict(synth.CANONICAL, channels_net=40, channels_bn=48, compression_level=3)
    return cae, cae.ConvolutionalAutoencoder(checkpoint=synth.synthetic_state(cfg, seed=seed))


def test_force_torch_agrees():
    """(I): the torch-op form of the same head on the device, within the end-to-end bound"""
    m = _model(A, 10)
    y_q, brg = _inputs(A, 3, 5, 2, 10)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    f64, _ = SR.jnet(sd, A, y_q, brg, torch.float64)
    f32, _ = SR.jnet(sd, A, y_q, brg, torch.float32)
    with torch.no_grad():
        got, _ = m(y_q, brg)
        m.force_torch = True
        ref, aux = m(y_q, brg)
    assert aux is None and ref.shape == got.shape
    bound = SR.e2e_bound(f32, f64)
    assert float((ref.cpu().double() - f64).abs().max()) <= bound
    assert float((got.cpu().double() - f64).abs().max()) <= bound


def test_forward_func_and_segment_compressed():
    """(I): forward_func with 'seg_model' gives s_pred equal to the direct call; segment_compressed on encoded tiles
    equals decode-then-head"""
    from cnn_autoencoder_amd import criteria, synth
    from cnn_autoencoder_amd.codec import _module
    S = _seg()
    cae, codec = _codec()
    seg = _model(A, 11)
    model = dict(codec._model, seg_model=seg)
    x = torch.from_numpy(np.stack([synth.histo_tile(48, i, w=64) for i in range(2)])).permute(0, 3, 1, 2).float().div(255).cuda()
    fwd = criteria.setup_forward_func(('encoder', 'fact_ent', 'decoder', 'seg_model'))
    with torch.no_grad():
        out = fwd(x, model)
        direct, aux = seg(out['y_q'], fx_brg=out['fx_brg'])
    assert out['s_aux_pred'] is None and aux is None
    assert out['s_pred'].shape == (2, 3, 48, 64) and torch.equal(out['s_pred'], direct)
    assert criteria.setup_forward_func(('encoder', 'fact_ent', 'decoder'))(x, model)['s_pred'] is None

    tiles = np.stack([synth.histo_tile(48, i, w=64) for i in range(3)])
    bufs = codec.encode_batch(tiles)
    got = S.segment_compressed(bufs, codec, seg)
    enc, eb, dec = (_module(codec._model[k]) for k in ('encoder', 'fact_ent', 'decoder'))
    with torch.no_grad():
        y_q = eb.dequantize_symbols(enc.forward_u8_symbols(torch.from_numpy(tiles).cuda(), eb))
        _, brg = dec(y_q)
        want, _ = seg(y_q, fx_brg=brg)
    assert got.shape == (3, 3, 48, 64) and torch.equal(got, want)
    assert torch.equal(got, S.segment_compressed(bufs, codec._model, seg))
