"""The MS-SSIM distortions (RateMSSSIM, RateMultiscaleMSSSIM; DistMSSSIMLoss / DistMSSSIMPyramidLoss of the reference,
_ratedist.py:10-43, 66-107) against tests/msssim_restatement.py.

Host part: the restatement is anchored to the committed float32 oracle; known answers; criteria on float64 CPU tensors
against the float64 restatement; the pinned refusals.

GPU part: the float32 torch restatement of the formula sits at a known distance
d32 = max|f32 restatement - f64 restatement| from float64, per case, on the value and on the gradient tensor; the kernels
must stay within 4 * d32 of float64 (the factor 4: this project's precedent for judging a kernel against a same-precision
restatement, tests/train_replay.py).  Each test prints its figures before it asserts.

Measured on an MI355X (error / d32, limit 4).  Values: at most 0.01 -- the kernels form the moments and the index maps of
the float32 images in float64.  Gradients (float32 coefficient maps and gather): worst 3.47 for the level kernels (win 7
on a 7 x 7 plane, a one-pixel map; 1.78 the next), 1.32 for the whole loss, 1.32 multiscale; in situ 0.06 of the bound."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import msssim_restatement as R

gpu = pytest.mark.gpu


class _Fe:
    def __init__(self):
        self.aux = torch.tensor(3.5, dtype=torch.float64)

    def loss(self):
        return self.aux


def rel(got, want) -> float:
    return abs(float(got) - float(want)) / max(abs(float(want)), 1e-300)


def ratio(err, d32) -> float:
    return err / d32 if d32 > 0 else (0.0 if err == 0 else float('inf'))


# ---------------------------------------------------------------------------------------------------------- host

def test_anchor_to_committed_oracle():
    from oracle import cae_oracle as O
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (176, 200, 3), dtype=np.uint8)
    b = np.clip(a.astype(int) + rng.integers(-20, 21, a.shape), 0, 255).astype(np.uint8)
    X = torch.from_numpy(np.moveaxis(b, -1, 0)[None]).float()
    Y = torch.from_numpy(np.moveaxis(a, -1, 0)[None]).float()
    want = O.ms_ssim_uint8(a, b)
    got = float(R.ms_ssim(X, Y, 255.0, 11, 1.5, torch.float32))
    assert rel(got, want) < 1e-6, (got, want)
    from cnn_autoencoder_amd import criteria
    assert rel(float(criteria.ms_ssim(X, Y, 255.0)), want) < 1e-6


def test_loss_of_identical_images_is_zero():
    from cnn_autoencoder_amd import criteria
    x = torch.rand(1, 3, 64, 64, dtype=torch.float64)
    for scale in range(4):
        d = criteria.DistMSSSIMLoss(patch_size=64, scale=scale)(x=x, x_r=[x.clone()])['dist']
        assert len(d) == 1 and abs(float(d[0])) < 1e-14, (scale, float(d[0]))


def test_padding_rule_and_windows():
    from cnn_autoencoder_amd import criteria
    assert [criteria.DistMSSSIMLoss(256, scale=s).padding for s in range(4)] == [0, 8, 24, 24]
    assert criteria.DistMSSSIMLoss(128, scale=0).padding == 24
    assert [R.loss_params(256, s)[2] for s in range(4)] == [0, 8, 24, 24] and R.loss_params(128, 0)[2] == 24
    for s, n in enumerate((11, 9, 7, 5)):
        d = criteria.DistMSSSIMLoss(256, scale=s)
        assert d.win_size == n and d.win_sigma == 1.5 / 2 ** s
        taps = criteria._gauss_taps(d.win_size, d.win_sigma, torch.float64)
        assert len(taps) == n and abs(float(taps.sum()) - 1) < 1e-15
        assert torch.allclose(taps, R.window(n, 1.5 / 2 ** s), rtol=0, atol=1e-16)
    assert criteria.DistMSSSIMLoss(64, normalize=True).data_range == 2 and criteria.DistMSSSIMLoss(64).data_range == 1


def test_size_assertion_of_ms_ssim():
    from cnn_autoencoder_amd import criteria
    x = torch.rand(1, 1, 160, 200)
    with pytest.raises(AssertionError):
        criteria.ms_ssim(x, x, 1.0, 11, 1.5)
    criteria.ms_ssim(torch.rand(1, 1, 161, 200), torch.rand(1, 1, 161, 200), 1.0, 11, 1.5)
    # through DistMSSSIMLoss a patch that is a multiple of 16 is padded to a side of at least 176 and passes
    criteria.DistMSSSIMLoss(16)(x=torch.rand(1, 1, 16, 16), x_r=[torch.rand(1, 1, 16, 16)])


def _host_case(L=4, patch=256):
    g = torch.Generator().manual_seed(7)
    x = torch.rand(1, 3, patch, patch, generator=g, dtype=torch.float64)
    x_r = [F.interpolate(x, scale_factor=0.5 ** s, mode='bilinear') if s else x.clone() for s in range(L)]
    x_r = [t + 0.05 * torch.randn(t.shape, generator=g, dtype=torch.float64) for t in x_r]
    p_y = torch.rand(1, 8, patch // 16, patch // 16, generator=g, dtype=torch.float64) * 0.9 + 0.05
    return x, x_r, p_y


@pytest.mark.parametrize('name,lam', [('RateMSSSIM', 0.7), ('RateMultiscaleMSSSIM', 0.7),
                                      ('RateMultiscaleMSSSIM', [0.7, 0.5, 0.3, 0.2])])
def test_criteria_on_float64_cpu_tensors(name, lam):
    from cnn_autoencoder_amd import criteria
    L, patch = 4, 256
    x, x_r, p_y = _host_case(L, patch)
    multi = 'Multiscale' in name
    crit = criteria.setup_loss(name, patch_size=patch, channels_org=3, compression_level=L, distortion_lambda=lam)
    assert crit._multiplier == 1
    leaves = [t.clone().requires_grad_(True) for t in x_r]
    ld = crit(inputs=x, outputs=dict(x_r=leaves if multi else [leaves[0], None, None, None], p_y=p_y),
              net={'fact_ent': _Fe()})
    assert len(ld['dist']) == (L if multi else 1)
    assert all(d.dtype == torch.float64 for d in ld['dist'])  # the CPU form keeps the dtype of its input
    ref_leaves = [t.clone().requires_grad_(True) for t in x_r]
    ref_dist = R.dist_msssim_pyramid(x, ref_leaves, patch) if multi else [R.dist_msssim(x, ref_leaves[0], patch)]
    lams = lam if isinstance(lam, list) else [lam]
    ref_dl = sum(d * w for d, w in zip(ref_dist, lams))  # a scalar lambda weights level 0 only
    ref_rate = -torch.sum(torch.log2(p_y)) / (patch * patch)
    for got, want in zip(ld['dist'], ref_dist):
        assert rel(got, want) < 1e-6
    assert rel(ld['dist_loss'], ref_dl) < 1e-6
    assert rel(ld['rate_loss'], ref_rate) < 1e-6
    assert rel(ld['loss'], ref_dl + ref_rate) < 1e-6
    if not isinstance(lam, list):
        assert rel(ld['dist_loss'], float(ld['dist'][0]) * lam) < 1e-12
    ld['loss'].backward()
    (ref_dl + ref_rate).backward()
    for s in range(len(lams)):
        want = ref_leaves[s].grad
        assert float((leaves[s].grad - want).abs().max()) <= 1e-9 * float(want.abs().max()), s
    for s in range(len(lams), L):
        assert leaves[s].grad is None or float(leaves[s].grad.abs().max()) == 0.0


def test_multiscale_msssim_rejects_a_model_without_colour_layers():
    from cnn_autoencoder_amd import criteria
    crit = criteria.setup_loss('RateMultiscaleMSSSIM', patch_size=32, channels_org=3, compression_level=3)
    x = torch.rand(1, 3, 32, 32)
    with pytest.raises(ValueError, match='multiscale_analysis'):
        crit(inputs=x, outputs=dict(x_r=[x, None, None], p_y=torch.rand(1, 4, 4, 4)), net={'fact_ent': _Fe()})


@pytest.mark.parametrize('name', ['RateMSSSIM', 'RateMultiscaleMSSSIM'])
def test_pinned_refusals(name):
    from cnn_autoencoder_amd import criteria
    with pytest.raises(NotImplementedError, match='patch_size'):
        criteria.setup_loss(name)
    with pytest.raises(NotImplementedError, match='patch_size'):
        criteria.setup_loss(name, channels_org=3, compression_level=3)
    assert isinstance(criteria.setup_loss(name, patch_size=64, channels_org=3, compression_level=3), criteria.GeneralLoss)
    with pytest.raises(NotImplementedError):
        criteria.setup_loss('RatePenaltyAMSE')


# ----------------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope='module')
def cae(built_lib):
    import cnn_autoencoder_amd as cae
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return cae


def _level_gpu(x_r, x, win, sigma, c1, c2, g_ssim, g_cs):
    """one scale on the kernels -> (ssim means, cs means, gradient), host tensors"""
    import ctypes
    from cnn_autoencoder_amd import _lib, criteria
    L, st = _lib.lib(), _lib.stream_ptr()
    n, c, h, w = x.shape
    planes = n * c
    taps = [float(t) for t in criteria._gauss_taps(win, sigma, torch.float64)]
    taps_c = (ctypes.c_double * win)(*taps)
    X, Y = x_r.float().cuda().contiguous(), x.float().cuda().contiguous()
    out = torch.empty((planes, 2), dtype=torch.float64, device='cuda')
    oh, ow = h - win + 1, w - win + 1
    ws = torch.empty(2 * planes * (-(-oh // 32)) * (-(-ow // 32)), dtype=torch.float64, device='cuda')
    _lib.check(L.cae_t_msssim_level_fwd(X.data_ptr(), Y.data_ptr(), planes, h, w, taps_c, win, c1, c2, out.data_ptr(),
                                        ws.data_ptr(), ws.numel(), st))
    gx = torch.zeros(planes, h, w, device='cuda')
    ws2 = torch.empty(3 * planes * oh * ow, dtype=torch.float32, device='cuda')
    gs, gc = g_ssim.double().reshape(-1).cuda(), g_cs.double().reshape(-1).cuda()
    args = (X.data_ptr(), Y.data_ptr(), planes, h, w, taps_c, win, c1, c2, gs.data_ptr(), gc.data_ptr(), gx.data_ptr(),
            ws2.data_ptr(), ws2.numel(), st)
    _lib.check(L.cae_t_msssim_level_bwd(*args))
    once = gx.clone()
    _lib.check(L.cae_t_msssim_level_bwd(*args))  # the backward ACCUMULATES: a second call doubles the buffer, exactly
    torch.cuda.synchronize()
    assert torch.equal(gx, 2 * once)
    return out[:, 0].reshape(n, c).cpu(), out[:, 1].reshape(n, c).cpu(), once.double().reshape(x.shape).cpu()


def _level_ref(x_r, x, win, sigma, c1, c2, g_ssim, g_cs, dtype):
    t = x_r.to(dtype).clone().requires_grad_(True)
    s, c = R.level(t, x.to(dtype), R.window(win, sigma, dtype), c1, c2)
    ((s * g_ssim.to(dtype)).sum() + (c * g_cs.to(dtype)).sum()).backward()
    return s.detach().double(), c.detach().double(), t.grad.double()


@gpu
@pytest.mark.parametrize('win', [11, 9, 7, 5])
@pytest.mark.parametrize('planes', [1, 6])
def test_level_kernels_against_float64(cae, win, planes):
    """sizes where the indexing changes: a side that is not a multiple of the tile, an odd side, the smallest legal side"""
    sigma = 1.5 / 2 ** ((11 - win) // 2)
    n, c = (1, 1) if planes == 1 else (2, 3)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    for h, w in ((70, 45), (win + 31, win + 32), (win, win), (win, 2 * win + 40)):
        g = torch.Generator().manual_seed(100 * win + h)
        x = torch.rand(n, c, h, w, generator=g)
        x_r = x + 0.05 * torch.randn(n, c, h, w, generator=g)
        g_ssim, g_cs = torch.randn(n, c, generator=g), torch.randn(n, c, generator=g)
        s64, c64, g64 = _level_ref(x_r, x, win, sigma, c1, c2, g_ssim, g_cs, torch.float64)
        s32, c32, g32 = _level_ref(x_r, x, win, sigma, c1, c2, g_ssim, g_cs, torch.float32)
        sk, ck, gk = _level_gpu(x_r, x, win, sigma, c1, c2, g_ssim, g_cs)
        dv = max(float((s32 - s64).abs().max()), float((c32 - c64).abs().max()))
        ev = max(float((sk - s64).abs().max()), float((ck - c64).abs().max()))
        dg, eg = float((g32 - g64).abs().max()), float((gk - g64).abs().max())
        print(f'level win {win} planes {planes} {h}x{w}: value err {ev:.3e} d32 {dv:.3e} ratio {ratio(ev, dv):.3f}; '
              f'grad err {eg:.3e} d32 {dg:.3e} ratio {ratio(eg, dg):.3f}')
        assert ev <= 4 * dv, (h, w, ev, dv)
        assert eg <= 4 * dg, (h, w, eg, dg)


@gpu
@pytest.mark.parametrize('planes,h,w', [(1, 7, 9), (3, 25, 50), (2, 23, 23), (5, 46, 13), (2, 1, 1), (4, 64, 33)])
def test_avgpool2_adjoint_on_odd_sizes(cae, planes, h, w):
    """cae_t_avgpool2_bwd alone against autograd of F.avg_pool2d(2, padding=s % 2) (padded samples counted), where a side
    is odd: the coarse size is (s + 1) / 2 there and the first fine row / column has a coarse sample of its own.  A quarter
    of one float is exact, so the two must be equal bit for bit; the forward kernel is checked on the same shapes."""
    from cnn_autoencoder_amd import _lib
    L, st = _lib.lib(), _lib.stream_ptr()
    gen = torch.Generator().manual_seed(planes * 1000 + h * 10 + w)
    x = torch.randn(1, planes, h, w, generator=gen).requires_grad_(True)
    y = R.pool(x)
    oh, ow = y.shape[-2:]
    assert (oh, ow) == ((h + 2 * (h % 2) - 2) // 2 + 1, (w + 2 * (w % 2) - 2) // 2 + 1)
    gy = torch.randn(y.shape, generator=gen)
    y.backward(gy)
    xd, gd = x.detach().cuda().contiguous(), gy.cuda().contiguous()
    yd = torch.full((planes, oh, ow), float('nan'), device='cuda')
    fine = torch.full((planes, h, w), float('nan'), device='cuda')  # the adjoint OVERWRITES
    _lib.check(L.cae_avgpool2(xd.data_ptr(), planes, h, w, yd.data_ptr(), st))
    _lib.check(L.cae_t_avgpool2_bwd(gd.data_ptr(), planes, h, w, fine.data_ptr(), st))
    torch.cuda.synchronize()
    assert float((yd.cpu() - y.detach()[0]).abs().max()) <= 1e-6 * float(y.detach().abs().max() + 1)
    assert torch.equal(fine.cpu(), x.grad[0])


def _ref_ms_ssim(x, x_r, win, sigma, dtype):
    t = x_r.clone().requires_grad_(True)
    v = R.ms_ssim(t, x, 1.0, win, sigma, dtype)
    v.backward()
    return float(v), t.grad.double()


@gpu
@pytest.mark.parametrize('sigma', R.SIGMAS)
@pytest.mark.parametrize('h,w', [(200, 184), (177, 203)])
def test_ms_ssim_with_odd_pooled_sides(cae, h, w, sigma):
    """criteria.ms_ssim where the pyramid meets odd sides (200 -> 100 -> 50 -> 25 -> 13, 184 -> 92 -> 46 -> 23 -> 12;
    177 -> 89 -> 45 -> 23 -> 12, 203 -> 102 -> 51 -> 26 -> 13): the zero-padded pooling and its adjoint inside the whole
    index, non-square, under the bound of the twelve cases.  Inputs of the same kind: field() at 208 pixels, cropped."""
    from cnn_autoencoder_amd import criteria
    x, xrs = R.field(208, 0, 208)
    x, x_r = x[..., :h, :w].contiguous(), xrs[sigma][..., :h, :w].contiguous()
    v64, g64 = _ref_ms_ssim(x, x_r, 11, 1.5, torch.float64)
    v32, g32 = _ref_ms_ssim(x, x_r, 11, 1.5, torch.float32)
    assert bool(torch.isfinite(g64).all())
    t = x_r.cuda().requires_grad_(True)
    v = criteria.ms_ssim(t, x.cuda(), 1.0, 11, 1.5)
    v.backward()
    ev, dv = abs(float(v) - v64), abs(v32 - v64)
    eg, dg = float((t.grad.double().cpu() - g64).abs().max()), float((g32 - g64).abs().max())
    print(f'odd sides {h}x{w} sigma {sigma}: value {v64:.6e} err {ev:.3e} d32 {dv:.3e} ratio {ratio(ev, dv):.3f}; '
          f'grad max {float(g64.abs().max()):.3e} err {eg:.3e} d32 {dg:.3e} ratio {ratio(eg, dg):.3f}')
    assert ev <= 4 * dv, (ev, dv)
    assert eg <= 4 * dg, (eg, dg)


@gpu
def test_fused_ms_ssim_checks_dtype_and_in_place_changes(cae):
    from cnn_autoencoder_amd import criteria
    x, xrs = R.field(192, 0, 192)
    with pytest.raises(TypeError, match='float32'):
        criteria.ms_ssim(xrs[0.1].double().cuda(), x.cuda())
    leaf = xrs[0.1].cuda().requires_grad_(True)
    t = leaf * 1.0
    v = criteria.ms_ssim(t, x.cuda())
    t.add_(1.0)  # level 0 of the saved pyramid is t itself
    with pytest.raises(RuntimeError, match='modified by an inplace operation'):
        v.backward()


def _ref_loss(x, x_r, patch, scale, dtype):
    t = x_r.clone().requires_grad_(True)
    v = R.dist_msssim(x, t, patch, scale, dtype=dtype)
    v.backward()
    return float(v), t.grad.double()


@gpu
@pytest.mark.parametrize('sigma', R.SIGMAS)
@pytest.mark.parametrize('patch,scale,hw', R.CASES)
def test_loss_value_and_gradient(cae, patch, scale, hw, sigma):
    from cnn_autoencoder_amd import criteria
    x, xrs = R.field(patch, scale, hw)
    x_r = xrs[sigma]
    v64, g64 = _ref_loss(x, x_r, patch, scale, torch.float64)
    v32, g32 = _ref_loss(x, x_r, patch, scale, torch.float32)
    assert bool(torch.isfinite(g64).all())
    t = x_r.cuda().requires_grad_(True)
    d = criteria.DistMSSSIMLoss(patch, scale=scale)(x=x.cuda(), x_r=[t])['dist'][0]
    d.backward()
    ev, dv = abs(float(d) - v64), abs(v32 - v64)
    eg, dg = float((t.grad.double().cpu() - g64).abs().max()), float((g32 - g64).abs().max())
    print(f'loss patch {patch} scale {scale} sigma {sigma}: value {v64:.6e} err {ev:.3e} d32 {dv:.3e} ratio {ratio(ev, dv):.3f}; '
          f'grad max {float(g64.abs().max()):.3e} err {eg:.3e} d32 {dg:.3e} ratio {ratio(eg, dg):.3f}')
    assert ev <= 4 * dv, (ev, dv)
    assert eg <= 4 * dg, (eg, dg)


@gpu
@pytest.mark.parametrize('sigma', R.SIGMAS)
def test_multiscale_loss_value_and_gradient(cae, sigma):
    """the four levels of patch 256 under GeneralLoss('MultiscaleMSSSIM'): x_r[s] = level s of the pyramid of x plus noise, so
    every level stays in the regime of the single-scale cases; the bound of each level is its own d32"""
    from cnn_autoencoder_amd import criteria
    L, patch = 4, 256
    x = R.field(patch, 0, 256)[0]
    gen, x_r, t = torch.Generator().manual_seed(11), [], x
    for s in range(L):
        x_r.append(t + sigma * torch.randn(t.shape, generator=gen))
        t = R.pyramid_down(t)
    crit = criteria.GeneralLoss('MultiscaleMSSSIM', None, patch_size=patch, channels_org=3, compression_level=L,
                                distortion_lambda=[1.0] * L)
    leaves = [t.cuda().requires_grad_(True) for t in x_r]
    ld = crit(inputs=x.cuda(), outputs=dict(x_r=leaves))
    assert len(ld['dist']) == L
    ld['loss'].backward()
    res = {}
    for dt in (torch.float64, torch.float32):
        ref = [t.clone().requires_grad_(True) for t in x_r]
        dist = R.dist_msssim_pyramid(x, ref, patch, dtype=dt)
        sum(dist).backward()
        res[dt] = ([float(d) for d in dist], [t.grad.double() for t in ref])
    assert all(bool(torch.isfinite(g).all()) for g in res[torch.float64][1])
    for s in range(L):
        v64, v32 = res[torch.float64][0][s], res[torch.float32][0][s]
        g64, g32 = res[torch.float64][1][s], res[torch.float32][1][s]
        ev, dv = abs(float(ld['dist'][s]) - v64), abs(v32 - v64)
        eg, dg = float((leaves[s].grad.double().cpu() - g64).abs().max()), float((g32 - g64).abs().max())
        print(f'multiscale sigma {sigma} level {s}: value {v64:.6e} err {ev:.3e} d32 {dv:.3e} ratio {ratio(ev, dv):.3f}; '
              f'grad err {eg:.3e} d32 {dg:.3e} ratio {ratio(eg, dg):.3f}')
        assert ev <= 4 * dv, (s, ev, dv)
        assert eg <= 4 * dg, (s, eg, dg)


@gpu
def test_bitwise_repeatability(cae):
    from cnn_autoencoder_amd import criteria
    x, xrs = R.field(192, 0, 192)
    xd = x.cuda()
    runs = []
    for _ in range(2):
        t = xrs[0.1].cuda().requires_grad_(True)
        d = criteria.DistMSSSIMLoss(192)(x=xd, x_r=[t])['dist'][0]
        d.backward()
        runs.append((d.detach().cpu(), t.grad.cpu()))
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])


def _small_model(cae, seed):
    from cnn_autoencoder_amd import synth
    cfg = dict(synth.CANONICAL, channels_net=32, channels_bn=48, compression_level=3)
    model = cae.autoencoder_from_state_dict(synth.synthetic_state(cfg, seed=seed), train=True)
    return cfg, model


@gpu
def test_in_situ_fused_against_torch_ops_and_three_steps(cae):
    """A GDN model (3 -> 32 -> 48, L = 3) under setup_loss('RateMSSSIM', patch_size=32) -- 32 is padded by 72 per side to
    176, the smallest side the size assertion admits -- through forward_func and loss.backward(), once with the fused
    loss and once with the torch-op form on the same device tensors.  Every parameter gradient must agree within
    4 * d32 of the loss gradient that feeds them, relative to the tensor's largest magnitude."""
    from cnn_autoencoder_amd import criteria, train
    patch, lam = 32, 1.0
    cfg, model = _small_model(cae, 3)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(2, 3, patch, patch, generator=g)
    ebm = model['fact_ent'].module
    ebm.fixed_noise = torch.rand(2, 48, patch // 8, patch // 8, generator=g) - 0.5
    fwd = criteria.setup_forward_func()
    xd = x.cuda()
    grads, x_rec = {}, None
    for form in ('fused', 'torch'):
        crit = criteria.setup_loss('RateMSSSIM', patch_size=patch, distortion_lambda=lam, force_torch=form == 'torch')
        for m in model.values():
            m.zero_grad(set_to_none=True)
        out = fwd(xd, model)
        ld = crit(inputs=xd, outputs=out, net=model)
        torch.mean(ld['loss']).backward()
        x_rec = out['x_r'][0].detach().cpu()
        grads[form] = {f'{k}.{n}': p.grad.detach().double().cpu() for k, m in model.items()
                       for n, p in m.named_parameters() if p.grad is not None}
    v64, g64 = _ref_loss(x, x_rec, patch, 0, torch.float64)
    v32, g32 = _ref_loss(x, x_rec, patch, 0, torch.float32)
    bound = 4 * float((g32 - g64).abs().max()) / float(g64.abs().max())
    assert sorted(grads['fused']) == sorted(grads['torch']) and grads['fused']
    worst = 0.0
    for name, want in grads['torch'].items():
        err = float((grads['fused'][name] - want).abs().max()) / max(float(want.abs().max()), 1e-300)
        worst = max(worst, err)
        print(f'in situ {name}: rel err {err:.3e} bound {bound:.3e}')
    print(f'in situ worst {worst:.3e} bound {bound:.3e} ratio {worst / bound:.3f}')
    for name, want in grads['torch'].items():
        err = float((grads['fused'][name] - want).abs().max()) / max(float(want.abs().max()), 1e-300)
        assert err <= bound, (name, err, bound)
    for m in model.values():
        m.zero_grad(set_to_none=True)
    crit = criteria.setup_loss('RateMSSSIM', patch_size=patch, distortion_lambda=lam)
    opts = train.setup_optim(model)
    losses = [float(train.train_step(xd, model, crit, opts)['loss']) for _ in range(3)]
    print('in situ losses', losses)
    assert all(np.isfinite(losses)) and losses[0] > losses[1] > losses[2], losses


@gpu
def test_multiscale_decoder_under_rate_multiscale_msssim(cae):
    from cnn_autoencoder_amd import criteria
    import torch.nn as nn
    patch, L = 32, 3
    cfg, model = _small_model(cae, 4)
    torch.manual_seed(0)
    kw = {k: cfg[k] for k in ('channels_org', 'channels_net', 'channels_bn', 'compression_level', 'kernel_size', 'bias',
                              'act_layer_type') if k in cfg}
    dec = cae.Synthesizer(multiscale_analysis=True, **kw).cuda()
    model['decoder'] = nn.DataParallel(dec, device_ids=[torch.cuda.current_device()]).train()
    crit = criteria.setup_loss('RateMultiscaleMSSSIM', patch_size=patch, channels_org=3, compression_level=L,
                               distortion_lambda=[1.0, 0.5, 0.25])
    x = torch.rand(2, 3, patch, patch, generator=torch.Generator().manual_seed(1)).cuda()
    ld = crit(inputs=x, outputs=criteria.setup_forward_func()(x, model), net=model)
    assert len(ld['dist']) == L and all(bool(torch.isfinite(d)) for d in ld['dist'])
    torch.mean(ld['loss']).backward()
    colour = [(n, p) for n, p in dec.named_parameters() if n.startswith('color_layers')]
    assert len({n.split('.')[1] for n, _ in colour}) == L - 1
    for n, p in colour:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n
