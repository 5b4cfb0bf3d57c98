"""The labelled device sampler (cae_t_sample_labeled_patches through sampler.LabeledPatchSampler.gather) against the
float64 restatement of its contract (tests/sampler_labeled_restatement.py).

Shapes.  A pool of 3 tiles of 37 x 45 whose valid sizes are 37 x 45, 10 x 9 (ragged) and 3 x 4 (smaller than every patch
here), 4 samples: inside tile 0, hanging over its top-left corner by 3 pixels, on the ragged tile, on the tiny tile.
Patch sizes 2 (taps reach beyond one reflection: reflections repeat), 5 (smaller than the 5-tap support), 8, 33 (odd, no
multiple of 4).  A pool of one 150 x 160 tile serves 128 (the largest plane kept in LDS; n = 2, C = 3) and 130 (the
global-memory variant; n = 1, C = 1).
Angles 0, 7.3 and 29.9 degrees; noise 0.05 makes the clamp active.

Image bound (DESIGN "Training input", labelled patches), with u = 2^-24, G = 4.8 the l1 gain of the prefilter along one
axis, A the largest interpolation coefficient of the batch in magnitude (from the restatement; A <= G^2 max|p|) and
|p| <= 1:
  prefilter    32 G^2 u      at most 16 roundings per value and axis, each relative u on a value that the rest of the
                             axis' steps carry to the output with the rest of the l1 gain G; the first axis' error
                             passes the second (G), the second axis' input is at most G;
  coordinates  20 A ps u     each source coordinate is 4 float32 operations on magnitudes of at most 1.21 ps (5 ps u), the
                             spline is 2 A-Lipschitz per axis (sum |w'| <= 2), two axes; it is continuous where the tap
                             window moves, so a window chosen differently in float32 costs nothing more;
  taps         40 A u        weights of a few ulp, 25 products and sums on |coef| <= A with unit-sum positive weights;
  noise        G^2 range (2^-23 + noise_std 2^-14), the patch's own bound (tests/test_sampler.py) through both axes.
Mask rule: t is compared exactly; a pixel is left out only where y + 0.5 or x + 0.5 of the float64 source point lies within
1e-4 of an integer, at most 1 % of a sample's pixels, none at angle 0.
"""
import functools

import numpy as np
import pytest
import torch

import sampler_labeled_restatement as L
import sampler_restatement as R
import segmenter_restatement as SR
from residue import poisoned_alloc  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

SEED = 0x5eed0123456789ab
TILE_HW = ((37, 45), (10, 9), (3, 4))
PLAIN, NOISY = (False, 0.0), (True, 0.05)  # (normalize, noise_std)


@pytest.fixture(scope='module', autouse=True)
def cae(built_lib):
    import cnn_autoencoder_amd as cae
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return cae


@functools.lru_cache(maxsize=None)
def pools(big, c, k):
    """(image pool, label pool, tile_hw or None)"""
    rng = np.random.default_rng(1000 * big + 10 * c + k)
    shape = (1, 150, 160) if big else (3, 37, 45)
    return (rng.integers(0, 256, shape + (c,), dtype=np.uint8), rng.integers(0, 2 if k > 1 else 4, shape + (k,), dtype=np.uint8),
            None if big else np.array(TILE_HW, dtype=np.int32))


def placement(big, n):
    """tile, y0, x0"""
    if big:
        return ((0, 0)[:n], (3, 10)[:n], (5, 20)[:n])
    return (0, 0, 1, 2), (2, -3, 1, -1), (4, -3, 2, 0)


@functools.lru_cache(maxsize=None)
def restated(big, c, k, ps, map_labels, normalize, noise_std, angles, n):
    """(x, t, coef_max) of the restatement, computed once per configuration and shared"""
    pool, labels, hw = pools(big, c, k)
    info = {}
    x, t = L.batch(pool, labels, *placement(big, n), ps, angle=angles, seed=SEED, noise_std=noise_std, normalize=normalize,
                   tile_hw=hw, map_labels=map_labels, info=info)
    x.setflags(write=False)
    t.setflags(write=False)
    return x, t, info['coef_max']


def sampler(big, c, k, ps, map_labels=False, normalize=False, noise_std=0.0, **kw):
    from cnn_autoencoder_amd.sampler import LabeledPatchSampler
    pool, labels, hw = pools(big, c, k)
    return LabeledPatchSampler(pool, labels, ps, add_noise=noise_std != 0.0, noise_std=noise_std, normalize=normalize, seed=SEED,
                               tile_hw=hw, map_labels=map_labels, **kw)


def bound(ps, coef_max, normalize, noise_std):
    u, g = 2.0 ** -24, L.L1_GAIN
    noise = (2.0 if normalize else 1.0) * (2.0 ** -23 + noise_std * 2.0 ** -14) if noise_std else 0.0
    return u * (32.0 * g * g + 20.0 * coef_max * ps + 40.0 * coef_max) + g * g * noise


def check_masks(got, want, ps, angles):
    """the mask rule of the module docstring"""
    for s, angle in enumerate(angles):
        skip = L.near_a_tie(ps, *R.cos_sin_f32(angle))
        if angle == 0.0:
            assert not skip.any()
        assert skip.mean() <= 0.01
        assert np.array_equal(got[s][:, ~skip], want[s][:, ~skip]), (s, angle)


# ------------------------------------------------------------------------------------------------------------ no rotation
@pytest.mark.parametrize('map_labels', [False, True])
@pytest.mark.parametrize('c,k', [(1, 1), (3, 3)])
@pytest.mark.parametrize('ps', [5, 33])
def test_without_rotation_x_is_the_unlabelled_patch_and_t_the_mask(ps, c, k, map_labels):
    from cnn_autoencoder_amd.sampler import PatchSampler
    s = sampler(False, c, k, ps, map_labels, *NOISY)
    tile, y0, x0 = placement(False, 4)
    x, t = s.gather(tile, y0, x0)
    assert x.shape == (4, c, ps, ps) and t.shape == (4, 1 if map_labels else k, ps, ps)
    assert x.dtype == t.dtype == torch.float32 and x.is_cuda and t.is_cuda
    pool, _, hw = pools(False, c, k)
    plain = PatchSampler(pool, ps, add_noise=True, noise_std=0.05, normalize=True, seed=SEED, tile_hw=hw)
    assert torch.equal(x, plain.gather(tile, y0, x0))
    want_t = restated(False, c, k, ps, map_labels, *NOISY, None, 4)[1]
    assert np.array_equal(t.cpu().numpy(), want_t)
    # the tiny tile holds 3 x 4 labels per channel
    assert want_t[0].max() >= 1.0 and (want_t[3] != 0).reshape(want_t.shape[1], -1).sum(1).max() <= 12


# --------------------------------------------------------------------------------------------------------------- rotation
ROTATED = [(False, c, k, ps, m, *cfg, (0.0, 7.3, 29.9, 7.3), 4)
           for ps in (2, 5, 8, 33) for c, k, m, cfg in ((3, 3, False, PLAIN), (1, 3, True, NOISY))]
ROTATED += [(True, 3, 2, 128, False, *PLAIN, (7.3, 29.9), 2), (True, 3, 2, 128, True, *NOISY, (0.0, 29.9), 2),
            (True, 1, 1, 130, False, *PLAIN, (0.0,), 1), (True, 1, 1, 130, False, *PLAIN, (7.3,), 1),
            (True, 1, 1, 130, True, *NOISY, (29.9,), 1)]


@pytest.mark.parametrize('case', ROTATED, ids=lambda v: 'ps{3}-c{1}-k{2}-map{4:d}-norm{5:d}-std{6}-{7}'.format(*v))
def test_rotation(case, poisoned_alloc):
    """x within the derived bound of the restatement, t by the mask rule; the outputs and the workspace come poisoned with
    NaN between guard bands, so an unwritten value or a write outside a buffer shows"""
    big, c, k, ps, map_labels, normalize, noise_std, angles, n = case
    want_x, want_t, coef_max = restated(*case)
    s = sampler(big, c, k, ps, map_labels, normalize, noise_std)
    x, t = s.gather(*placement(big, n), angles)
    poisoned_alloc.check()
    x, t = x.cpu().numpy(), t.cpu().numpy()
    assert x.shape == want_x.shape and t.shape == want_t.shape
    err, tol = float(np.abs(x.astype(np.float64) - want_x).max()), bound(ps, coef_max, normalize, noise_std)
    print(f'labelled rotation {case[1:]}: coef_max {coef_max:.3f} err {err:.3e} bound {tol:.3e} ratio {err / tol:.3f}')
    assert err <= tol  # also false for a NaN
    check_masks(t, want_t, ps, angles)
    assert coef_max <= L.L1_GAIN ** 2 + 1e-9


def test_repeatable_and_independent_of_the_split(poisoned_alloc):
    ps, angles = 33, (0.0, 7.3, 29.9, 7.3)
    tile, y0, x0 = placement(False, 4)
    s = sampler(False, 3, 3, ps, False, *NOISY)
    a, b = s.gather(tile, y0, x0, angles), s.gather(tile, y0, x0, angles)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    parts = [s.gather(tile[:1], y0[:1], x0[:1], angles[:1], sample_base=0),
             s.gather(tile[1:], y0[1:], x0[1:], angles[1:], sample_base=1)]
    assert torch.equal(torch.cat([p[0] for p in parts]), a[0]) and torch.equal(torch.cat([p[1] for p in parts]), a[1])
    assert not torch.equal(s.gather(tile, y0, x0, angles, noise_seed=SEED + 1)[0], a[0])  # the seed does key the noise
    poisoned_alloc.check()
    # the same through the workspace of the global-memory variant: poisoned on every call, the bits stay
    big = sampler(True, 1, 1, 130, False, *NOISY)
    tile, y0, x0 = placement(True, 2)
    a, b = big.gather(tile, y0, x0, (7.3, 29.9)), big.gather(tile, y0, x0, (7.3, 29.9))
    part = big.gather(tile[1:], y0[1:], x0[1:], (29.9,), sample_base=1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(part[0], a[0][1:])
    assert bool(torch.isfinite(a[0]).all())
    poisoned_alloc.check()


@pytest.mark.parametrize('ps,c,k,map_labels,cfg', [(5, 3, 3, False, PLAIN), (33, 1, 3, True, NOISY)])
def test_the_host_form_agrees_with_the_kernel(ps, c, k, map_labels, cfg):
    from cnn_autoencoder_amd.sampler import LabeledPatchSampler
    angles, (tile, y0, x0) = (0.0, 7.3, 29.9, 7.3), placement(False, 4)
    pool, labels, hw = pools(False, c, k)
    ref = LabeledPatchSampler(torch.from_numpy(pool).cuda(), labels, ps, add_noise=cfg[1] != 0.0, noise_std=cfg[1],
                              normalize=cfg[0], seed=SEED, tile_hw=hw, map_labels=map_labels, force_torch=True)
    rx, rt = ref.gather(tile, y0, x0, angles)
    gx, gt = sampler(False, c, k, ps, map_labels, *cfg).gather(tile, y0, x0, angles)
    assert rx.is_cuda and rx.shape == gx.shape and rt.shape == gt.shape
    coef_max = restated(False, c, k, ps, map_labels, *cfg, angles, 4)[2]
    err, tol = float((rx.double() - gx.double()).abs().max()), bound(ps, coef_max, *cfg)
    print(f'host form ps={ps}: err {err:.3e} bound {tol:.3e}')
    assert err <= tol
    check_masks(gt.cpu().numpy(), rt.cpu().numpy(), ps, angles)


def test_device_side_values_cannot_fault(poisoned_alloc):
    """a tile index, cos and sin that only the device sees: the patch of a tile outside the pool is padding, and NaN or
    huge cos / sin are clamped as coordinates before any cast; every output value is written and finite"""
    from cnn_autoencoder_amd import _lib
    pool, labels, _ = pools(False, 3, 3)
    pool_dev, labels_dev = torch.from_numpy(pool).cuda(), torch.from_numpy(labels).cuda()
    idx = torch.tensor([[0, 3, 0], [2, 2, 2], [4, 4, 4]], dtype=torch.int32).cuda()
    cos = torch.tensor([float('nan'), 1.0, 3.0e38], dtype=torch.float32).cuda()
    sin = torch.tensor([0.0, 0.0, -3.0e38], dtype=torch.float32).cuda()
    x, t = torch.empty(3, 3, 8, 8, device='cuda'), torch.empty(3, 3, 8, 8, device='cuda')
    rc = _lib.lib().cae_t_sample_labeled_patches(
        pool_dev.data_ptr(), labels_dev.data_ptr(), 3, 37, 45, 3, 3, None, idx[0].data_ptr(), idx[1].data_ptr(),
        idx[2].data_ptr(), None, cos.data_ptr(), sin.data_ptr(), 0, 0, 0.0, 0, 0, 3, 8, None, 0, x.data_ptr(), t.data_ptr(),
        _lib.stream_ptr())
    torch.cuda.synchronize()
    poisoned_alloc.check()
    assert rc == 0 and bool(torch.isfinite(x).all()) and bool(torch.isfinite(t).all())
    assert float(x[1].abs().max()) == 0.0 and float(t[1].abs().max()) == 0.0 and float(x[0].max()) > 0.0
    # the host copy of the indices is checked before anything is launched
    host = torch.tensor([0, 3, 0], dtype=torch.int32)
    x.fill_(7.0)
    rc = _lib.lib().cae_t_sample_labeled_patches(
        pool_dev.data_ptr(), labels_dev.data_ptr(), 3, 37, 45, 3, 3, None, idx[0].data_ptr(), idx[1].data_ptr(),
        idx[2].data_ptr(), host.data_ptr(), cos.data_ptr(), sin.data_ptr(), 0, 0, 0.0, 0, 0, 3, 8, None, 0, x.data_ptr(),
        t.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and bool((x == 7.0).all())


# ------------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize('loss,k,map_labels,dtype', [('BCELoss', 3, False, torch.float32), ('CELoss', 2, True, torch.int64)])
def test_a_sampled_batch_trains_the_head(cae, loss, k, map_labels, dtype):
    """one seg_train.train_step on a batch the iterator yields: codec and head of the golden configuration 'a' (three
    levels, three classes), 16 x 16 patches; the step runs, the loss is finite and every head parameter moves"""
    from cnn_autoencoder_amd import seg_train as T, synth
    from cnn_autoencoder_amd.sampler import LabeledPatchSampler
    cfg, sd, *_ = SR.load_golden('a')
    head = T.JNetTrain(**cfg)
    head.load_state_dict(sd, strict=True)
    head = head.cuda().train()
    codec = cae.ConvolutionalAutoencoder(checkpoint=synth.synthetic_state(
        dict(synth.CANONICAL, channels_net=cfg['channels_net'], channels_bn=cfg['channels_bn'],
             compression_level=cfg['compression_level']), seed=3))
    model = dict(codec._model, seg_model=head)
    pool, labels, hw = pools(False, 3, k)
    s = LabeledPatchSampler(pool, labels, 16, rotation=True, normalize=False, map_labels=map_labels, target_data_type=dtype,
                            tile_hw=hw, batch_size=2, steps_per_epoch=1)
    (x, t), = list(s)
    assert x.shape == (2, 3, 16, 16) and t.dtype == dtype and t.is_cuda
    assert t.shape == ((2, 16, 16) if loss == 'CELoss' else (2, 3, 16, 16))
    before = [p.detach().clone() for p in head.parameters()]
    out = T.train_step(x, t, model, T.SegLoss(loss), T.setup_optim(model, learning_rate=1e-3))
    assert np.isfinite(float(out['class_error']))
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, head.parameters()))
