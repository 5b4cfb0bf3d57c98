"""Buffers that the Python wrappers take from torch.empty / empty_like, poisoned and fenced (tests/residue.py).

Under the caching allocator such a buffer holds whatever the step before left there.  With the poisoned_alloc fixture it
holds NaN (bytes 0x7F for integers) and lies between two guard bands: a kernel that leaves part of its output unwritten,
or reads a scratch buffer before writing it, shows the poison in its result; a kernel that writes outside its buffer
breaks a band.  Inference wrappers are judged by bit-equality with an unpoisoned run, training paths by the existing
bounds of their own tests, whose bodies run here unchanged with the fixture active.

The first four tests need no GPU: they show that the fixture poisons, fences and restores, and that the method catches a
toy kernel that leaves its last ragged column unwritten.
"""
import numpy as np
import pytest
import torch

import residue
from residue import covering_shape, poisoned_alloc  # noqa: F401  (the fixture)

DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16, torch.int32, torch.int64, torch.uint8]


# ------------------------------------------------------------------------------------------------- the helpers (CPU)
def _is_poison(t):
    if t.dtype == torch.bfloat16:
        return bool((t.view(torch.int16) == 0x7FC0).all())
    if t.dtype.is_floating_point:
        return bool(torch.isnan(t).all())
    return bool((t.contiguous().view(torch.uint8) == 0x7F).all())


def test_fixture_poisons_every_call_form_and_restores_torch(request):
    real = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    pa = request.getfixturevalue('poisoned_alloc')
    assert torch.empty is not real[0] and torch.empty_like is not real[1] and torch.Tensor.new_empty is not real[2]
    for dt in DTYPES:
        a = torch.empty(3, 5, dtype=dt)                       # size as varargs
        b = torch.empty((3, 5), dtype=dt, device='cpu')       # size as a tuple, device keyword
        c = torch.empty_like(a)
        d = torch.empty_like(a, dtype=torch.float32)
        e = a.new_empty((2, 7))
        f = a.new_empty(2, 7, dtype=torch.int32)
        for t, shape, dtype in ((a, (3, 5), dt), (b, (3, 5), dt), (c, (3, 5), dt), (d, (3, 5), torch.float32),
                                (e, (2, 7), dt), (f, (2, 7), torch.int32)):
            assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous() and _is_poison(t), (dt, shape)
    cl = torch.empty((2, 3, 4, 5), memory_format=torch.channels_last)
    assert cl.is_contiguous(memory_format=torch.channels_last) and _is_poison(cl)
    assert _is_poison(torch.empty_like(cl)) and torch.empty_like(cl).stride() == cl.stride()
    assert torch.empty(4, requires_grad=True).requires_grad
    assert torch.empty(0).numel() == 0
    assert pa.count >= 6 * len(DTYPES) + 5
    # 0x7FC0 and the NaN of each float type, as bytes
    assert residue.guard_pattern(torch.bfloat16)[:2].tolist() == [0xC0, 0x7F]
    assert residue.guard_pattern(torch.float32)[:4].tolist() == [0, 0, 0xC0, 0x7F]
    assert residue.guard_pattern(torch.int32)[:4].tolist() == [0x7F] * 4
    request.getfixturevalue('monkeypatch').undo()
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == real
    assert not _is_poison(torch.zeros(3)) and torch.empty(2, 2).shape == (2, 2)


def test_check_fails_after_one_byte_in_a_guard_band(poisoned_alloc):
    poisoned_alloc.guard_host = True  # (device tensors are always fenced; this test has no device)
    for dt in (torch.uint8, torch.float32, torch.bfloat16):
        t = torch.empty((3, 7), dtype=dt)
        assert _is_poison(t) and t.data_ptr() - t._base.data_ptr() == residue.GUARD_BYTES
        t.zero_()  # the whole interior, and nothing else
        assert poisoned_alloc.check(release=False) >= 1
        whole = t._base.view(torch.uint8)
        end = residue.GUARD_BYTES + t.numel() * dt.itemsize
        for at in (end, residue.GUARD_BYTES - 1, whole.numel() - 1, 0):  # the bytes next to the buffer, the far ends
            keep = int(whole[at])
            whole[at] = keep ^ 1
            with pytest.raises(AssertionError, match='written (below|above) the buffer'):
                poisoned_alloc.check(release=False)
            whole[at] = keep
        assert poisoned_alloc.check() >= 1  # intact again; released
    assert poisoned_alloc.check() == 0


def test_covering_shape_refuses_pitch_slack_and_smaller_shapes():
    assert covering_shape('analysis', (2, 17, 33), 3, 3) == (2, 48, 256)
    assert covering_shape('synthesis', (2, 4, 9), 3, 3) == (2, 8, 64)
    with pytest.raises(AssertionError, match='unwritten pitch'):  # 96 = 3 x 32: whole C8S groups, half a C8SP block
        covering_shape('synthesis', (2, 4, 9), 3, 3, dirty=(2, 8, 96))
    assert covering_shape('analysis', (2, 17, 33), 0, 3, dirty=(2, 34, 96)) == (2, 34, 96)
    with pytest.raises(AssertionError, match='unwritten pitch'):  # 96 -> 48 at level 1: a ragged group
        covering_shape('analysis', (2, 17, 33), 1, 3, dirty=(2, 34, 96))
    with pytest.raises(AssertionError, match='smaller than clean'):
        covering_shape('synthesis', (2, 8, 17), 2, 3, dirty=(2, 7, 64))
    with pytest.raises(AssertionError, match='smaller than clean'):
        covering_shape('analysis', (2, 17, 130), 2, 3, dirty=(2, 40, 128))
    with pytest.raises(AssertionError, match='less than twice'):
        covering_shape('synthesis', (2, 8, 17), 2, 3, dirty=(2, 8, 64))
    with pytest.raises(AssertionError, match='dirty n'):
        covering_shape('synthesis', (2, 8, 17), 2, 3, dirty=(6, 16, 64))


def _toy_scale(x, leaky):
    """a "kernel" over 32-column tiles; the leaky one forgets the ragged tile at the end of a row"""
    out = torch.empty_like(x)
    w = x.shape[-1]
    for x0 in range(0, w if not leaky else w - w % 32, 32):
        out[..., x0:x0 + 32] = 2.0 * x[..., x0:x0 + 32]
    return out


def test_poison_catches_an_unwritten_ragged_column(poisoned_alloc):
    x = torch.rand(2, 3, 5, 33)
    assert torch.equal(_toy_scale(x, False), 2.0 * x)
    got = _toy_scale(x, True)
    assert torch.equal(got[..., :32], 2.0 * x[..., :32])
    assert not bool(torch.isfinite(got).all()) and bool(torch.isnan(got[..., 32]).all())
    assert bool(torch.isfinite(_toy_scale(torch.rand(2, 3, 5, 64), True)).all())  # (no ragged tile: nothing to forget)


# ------------------------------------------------------------------------------------------------- GPU: inference
def _cae():
    import cnn_autoencoder_amd as cae
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return cae


def _flat(out):
    if isinstance(out, torch.Tensor):
        return [out]
    if isinstance(out, (bytes, np.ndarray)):
        return [torch.from_numpy(np.frombuffer(out, dtype=np.uint8).copy() if isinstance(out, bytes) else out)]
    return [t for o in out if o is not None for t in _flat(o)]


def _same_under_poison(monkeypatch, run):
    """run() with the real allocator, then poisoned and fenced: bit-identical, finite, no band broken"""
    want = _flat(run())
    torch.cuda.synchronize()
    pa = residue.PoisonedAlloc()
    with monkeypatch.context() as m:
        m.setattr(torch, 'empty', pa.empty)
        m.setattr(torch, 'empty_like', pa.empty_like)
        m.setattr(torch.Tensor, 'new_empty', lambda self, *size, **kw: pa.new_empty(self, *size, **kw))
        got = _flat(run())
        torch.cuda.synchronize()
        assert pa.count > 0, 'the path took no buffer from torch.empty'
        pa.check()
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(want, got)):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert not b.dtype.is_floating_point or bool(torch.isfinite(b).all()), f'output {i} holds poison'
        assert torch.equal(a, b), f'output {i}: {int((a != b).sum())} elements differ under poison'


INFERENCE = ['analyzer', 'synthesizer', 'entropy', 'coders', 'metrics', 'ms_ssim', 'sampler']


@pytest.mark.gpu
@pytest.mark.parametrize('path', INFERENCE)
def test_inference_wrappers_write_all_of_their_buffers(built_lib, monkeypatch, path):
    import test_inference_kernels as K
    _cae()
    g = torch.Generator().manual_seed(21)
    if path == 'analyzer':
        enc = K._analyzer('f16x3', seed=1, channels_org=3, channels_net=40, channels_bn=16, compression_level=3,
                          kernel_size=3, act_layer_type='GDN')
        x = torch.rand(2, 3, 17, 33, generator=g).cuda()
        u8 = torch.randint(0, 256, (2, 17, 33, 3), generator=g, dtype=torch.uint8).cuda()
        with torch.no_grad():
            _same_under_poison(monkeypatch, lambda: (enc(x), enc.forward_levels(x), enc.forward_u8(u8)))
    elif path == 'synthesizer':
        dec = K._synthesizer('f16x3', seed=2, channels_org=3, channels_net=32, channels_bn=16, compression_level=3,
                             kernel_size=3, act_layer_type='GDN', multiscale_analysis=True)
        yq = (torch.randn(2, 16, 4, 9, generator=g) * 2).cuda()
        with torch.no_grad():
            _same_under_poison(monkeypatch, lambda: (dec(yq), dec.forward_u8(yq), dec.forward_scale(yq, 1),
                                                     dec.forward_scale(yq, 2)))
    elif path in ('entropy', 'coders'):
        from cnn_autoencoder_amd import entropy
        torch.manual_seed(5)
        eb = entropy.EntropyBottleneck(24).eval()
        eb.fit_quantiles()
        eb.update(force=True)
        eb = eb.cuda()
        y = (torch.randn(3, 24, 7, 5, generator=g) * 6).cuda()
        with torch.no_grad():
            if path == 'entropy':
                def run():
                    sym = eb.quantize_symbols(y)
                    return sym, eb.dequantize_symbols(sym), eb(y), eb.rate_bits(y)
            else:
                def run():
                    out = []
                    for coder in entropy.CODERS:
                        strings = [bytes(s) for s in eb.compress(y, coder=coder)]
                        out += strings + [eb.decompress(strings, (7, 5), coder=coder)]
                    return out
            _same_under_poison(monkeypatch, run)
    elif path in ('metrics', 'ms_ssim'):
        from cnn_autoencoder_amd import metrics
        shape = (2, 70, 101, 3) if path == 'metrics' else (1, 200, 171, 3)
        rng = np.random.default_rng(11)
        x = rng.integers(0, 256, shape, dtype=np.uint8)
        y = np.clip(x.astype(int) + rng.integers(-12, 13, shape), 0, 255).astype(np.uint8)
        xs, ys = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        if path == 'metrics':
            names = [k for k in metrics.metric_fun if k != 'ms-ssim']  # (ms-ssim needs sides above 160: the next case)
            assert {'dist', 'psnr', 'ssim', 'delta_cielab'} <= set(names)
        else:
            names = ['ms-ssim']
        run = lambda: [metrics.metric_fun[k](x=xs, x_r=ys, nbytes=[1000.0] * shape[0]) for k in names]  # noqa: E731
        _same_under_poison(monkeypatch, run)
    else:
        import test_sampler as S
        hw = np.array([[S.H, S.W], [10, 9]], dtype=np.int32)  # a ragged pool: tile 1 is 10 x 9 of 37 x 45
        tile, y0, x0 = S.placement(33)
        smp = S.sampler(_cae(), 3, 33, True, 0.05, tile_hw=hw)
        _same_under_poison(monkeypatch, lambda: smp.gather(tile, y0, x0, S.ANGLES))


# ------------------------------------------------------------------------------------------------- GPU: training
def _training_bodies():
    import msssim_restatement as M
    import test_msssim_loss as TM
    import test_train as TT
    import test_train_multiscale as TS
    mp = 'monkeypatch'
    track = TT.test_track_gradients_match_the_restatement.pytestmark[0].args[1][0]
    multi = TS.test_multiscale_decoder_gradients_match_the_restatement.pytestmark[0].args[1][0]
    return {
        'track_gradients': (TT.test_track_gradients_match_the_restatement, dict(cfgkw=track[0], shape=track[1])),
        'residual_gdn': (TT.test_residual_unit_gradients_match_the_restatement, dict(act='GDN', bias=False, ks=3)),
        'residual_lrelu': (TT.test_residual_unit_gradients_match_the_restatement, dict(act='LeakyReLU', bias=True, ks=3)),
        'gdn_32_unfused': (TT.test_gdn_kernels, dict(inverse=False, c=32, shape=(3, 8, 8), pad=1, fused=False, monkeypatch=mp)),
        'gdn_32_fused': (TT.test_gdn_kernels, dict(inverse=False, c=32, shape=(3, 8, 8), pad=1, fused=True, monkeypatch=mp)),
        'igdn_32_fused': (TT.test_gdn_kernels, dict(inverse=True, c=32, shape=(3, 8, 8), pad=1, fused=True, monkeypatch=mp)),
        # (the fused pair is built for at most 128 channels: 192 has the three-kernel form only)
        'gdn_192_unfused': (TT.test_gdn_kernels, dict(inverse=False, c=192, shape=(1, 9, 14), pad=0, fused=False, monkeypatch=mp)),
        'igdn_192_unfused': (TT.test_gdn_kernels, dict(inverse=True, c=192, shape=(1, 9, 14), pad=0, fused=False, monkeypatch=mp)),
        'batch_norm': (TT.test_batch_norm_units_train_on_batch_statistics, dict(residual=False, act='LeakyReLU')),
        'multiscale_decoder': (TS.test_multiscale_decoder_gradients_match_the_restatement,
                               dict(kw=multi[0], shape=multi[1], edge=multi[2], monkeypatch=mp)),
        'msssim_loss': (TM.test_loss_value_and_gradient, dict(zip(('patch', 'scale', 'hw'), M.CASES[3]), sigma=M.SIGMAS[0])),
        'clip_adam': (TT.test_fused_clip_adam_equals_the_torch_loop, dict(monkeypatch=mp)),
        'density_plain': (TT.test_fused_density_kernels_match_the_elementwise_graph, dict(form='plain', monkeypatch=mp)),
        'density_sign_trick': (TT.test_fused_density_kernels_match_the_elementwise_graph,
                               dict(form='sign_trick', monkeypatch=mp)),
    }


TRAINING = ['track_gradients', 'residual_gdn', 'residual_lrelu', 'gdn_32_unfused', 'gdn_32_fused', 'igdn_32_fused',
            'gdn_192_unfused', 'igdn_192_unfused', 'batch_norm', 'multiscale_decoder', 'msssim_loss', 'clip_adam',
            'density_plain', 'density_sign_trick']


def test_the_training_bodies_exist():
    """(no GPU) the names above are the table's, and every body is a plain function taking what it is given"""
    import inspect
    bodies = _training_bodies()
    assert sorted(bodies) == sorted(TRAINING)
    for name, (fn, kw) in bodies.items():
        assert set(inspect.signature(fn).parameters) == set(kw) | {'cae'}, name


@pytest.mark.gpu
@pytest.mark.parametrize('name', TRAINING)
def test_training_kernels_hold_their_bounds_on_poisoned_buffers(built_lib, poisoned_alloc, monkeypatch, name):
    """the body of an existing training test, unchanged, with every torch.empty buffer poisoned and fenced: its own bounds
    judge the result (NaN fails every one of them), then no guard band may be broken"""
    fn, kw = _training_bodies()[name]
    kw = {k: (monkeypatch if v == 'monkeypatch' else v) for k, v in kw.items()}
    fn(_cae(), **kw)
    assert poisoned_alloc.count > 0
    poisoned_alloc.check()


@pytest.mark.gpu
def test_two_training_steps_on_poisoned_buffers(built_lib, poisoned_alloc):
    """Two consecutive train.train_step of the 32-channel model at (2, 40, 56), every scratch buffer poisoned and fenced,
    against the same loop on the CPU restatement with the same noise, judged as
    test_train.test_twenty_training_steps_follow_the_restatement judges its steps (2e-3 on loss, rate and distortion, 1e-2
    on the first layer's weights afterwards).  The optimiser consumes the gradients inside the step, so their finiteness
    is read from every parameter after it: Adam carries a NaN gradient into the parameter."""
    import test_train as TT
    from cnn_autoencoder_amd import criteria, synth, train
    from oracle import train_oracle as T
    cae = _cae()
    cfg = dict(synth.CANONICAL, channels_net=32, channels_bn=48, compression_level=3)
    state, model, layers = TT._models(cae, cfg, seed=22)
    eb = model['fact_ent'].module
    n_filters = len(eb.filters)
    eb_ref = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in eb.named_parameters()}
    target = eb.target.detach().cpu()
    lam = 0.01
    criterion = criteria.GeneralLoss(distortion_lambda=lam)
    opts = train.setup_optim(model, learning_rate=1e-3, aux_learning_rate=1e-2)
    flat = lambda ls: [t for l in ls for t in l.values() if t is not None]  # noqa: E731
    ref_groups = dict(encoder=flat(layers['encoder']), decoder=flat(layers['decoder']),
                      fact_ent=[v for k, v in eb_ref.items() if 'quantiles' not in k], fact_ent_aux=[eb_ref['quantiles']])
    ref_opts = {k: torch.optim.Adam([dict(params=v, lr=1e-2 if k.endswith('_aux') else 1e-3)]) for k, v in ref_groups.items()}
    gen = torch.Generator().manual_seed(3)
    for step in range(2):
        x = torch.rand(2, 3, 40, 56, generator=gen)
        noise = torch.rand(2, 48, 5, 7, generator=gen) - 0.5
        eb.fixed_noise = noise
        ld = train.train_step(x.cuda(), model, criterion, opts)
        poisoned_alloc.check()  # (and the step's buffers go back to the allocator: the next step is handed them again)
        y = T.analysis(x, layers['encoder'])
        y_q, p_y = T.entropy_forward(eb_ref, y, noise, n_filters, form=eb.likelihood_form)
        x_r = T.synthesis(y_q, layers['decoder'])
        loss, rate, dist = T.rd_loss(x, x_r, p_y, lam)
        loss.backward()
        T.aux_loss(eb_ref, n_filters, target).backward()
        for opt in ref_opts.values():
            torch.nn.utils.clip_grad_norm_(opt.param_groups[0]['params'], max_norm=1.0)
            opt.step()
            opt.zero_grad()
        assert np.isfinite(float(ld['loss']))
        assert float(ld['loss']) == pytest.approx(float(loss), rel=2e-3), step
        assert float(ld['rate_loss']) == pytest.approx(float(rate), rel=2e-3), step
        assert float(ld['dist'][0]) == pytest.approx(float(dist), rel=2e-3), step
        for part in ('encoder', 'decoder', 'fact_ent'):
            for pname, p in model[part].named_parameters():
                assert bool(torch.isfinite(p).all()), (step, part, pname)
    w_ref = layers['encoder'][0]['weight'].detach()
    w_got = model['encoder'].module.analysis_track[0].model[0].weight.detach().cpu()
    assert TT.rel(w_got, w_ref) < 1e-2
    assert TT.rel(eb.quantiles.detach().cpu(), eb_ref['quantiles'].detach()) < 1e-3
