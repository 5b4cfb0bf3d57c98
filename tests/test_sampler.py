"""The device patch sampler (cae_t_sample_patches through sampler.PatchSampler.gather) against the float64 restatement
of its contract (tests/sampler_restatement.py).

Shapes: a pool of 2 tiles of 37 x 45 with 1, 3 and 4 channels, 5 samples.  One sample lies inside the image (where the patch
fits), one hangs over the top-left corner by 3 pixels, one over the bottom-right corner, one starts at an odd column (an
unaligned byte read) and two use tile 1.  Patch sizes 8 (even centre), 33 (odd, dword stores with a tail) and 64 (larger
than the tile).

Bounds (range = 1, or 2 when normalised):
  plain      bit-identical: the float32 quotient and the exact (v - 0.5) / 0.5 leave nothing to round differently;
  rotation   range * 8 * ps * 2^-24: each source coordinate is three float32 operations on magnitudes of at most ps, bilinear
             interpolation is 1-Lipschitz per axis per unit of range, the four-tap arithmetic adds a few ulp;
  noise      range * (2^-23 + noise_std * 2^-14): |g| <= 6.7 for 32-bit uniforms, and a few-ulp float32 evaluation of it is
             below 2^-14; 0.05 makes the clamp active on many pixels;
  both       the sum of the two.
"""
import functools

import numpy as np
import pytest
import torch

import sampler_restatement as R

pytestmark = pytest.mark.gpu

T, H, W, N = 2, 37, 45, 5
ANGLES = (0.0, 30.0, -30.0, 90.0, 17.3)
SEED = 0x5eed0123456789ab


@pytest.fixture(scope='module')
def cae(built_lib):
    import cnn_autoencoder_amd as cae
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return cae


@functools.lru_cache(maxsize=None)
def pool(c):
    return np.random.default_rng(100 + c).integers(0, 256, (T, H, W, c), dtype=np.uint8)


def placement(ps):
    """tile, y0, x0 of the five samples"""
    return ((0, 0, 0, 1, 1),
            (2, -3, H - ps + 3, 1, 0),
            (4, -3, W - ps + 4, 7, 1))


@functools.lru_cache(maxsize=None)
def restated(c, ps, normalize, rotate, noise_std):
    """the restatement of the common batch, computed once per configuration and shared"""
    tile, y0, x0 = placement(ps)
    out = R.batch(pool(c), tile, y0, x0, ps, angle=ANGLES if rotate else None, seed=SEED, noise_std=noise_std,
                  normalize=normalize)
    out.setflags(write=False)
    return out


def sampler(cae, c, ps, normalize=False, noise_std=0.0, **kw):
    from cnn_autoencoder_amd.sampler import PatchSampler
    return PatchSampler(pool(c), ps, add_noise=noise_std != 0.0, noise_std=noise_std, normalize=normalize, seed=SEED, **kw)


def gathered(cae, c, ps, normalize, rotate, noise_std, **kw):
    tile, y0, x0 = placement(ps)
    return sampler(cae, c, ps, normalize, noise_std, **kw).gather(tile, y0, x0, ANGLES if rotate else None)


def bound(ps, normalize, rotate, noise_std):
    rng = 2.0 if normalize else 1.0
    return rng * ((8.0 * ps * 2.0 ** -24 if rotate else 0.0) + (2.0 ** -23 + noise_std * 2.0 ** -14 if noise_std else 0.0))


def max_err(got: torch.Tensor, want: np.ndarray) -> float:
    return float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())


SHAPES = [(c, ps) for c in (1, 3, 4) for ps in (8, 33, 64)]


@pytest.mark.parametrize('normalize', [False, True])
@pytest.mark.parametrize('c,ps', SHAPES)
def test_plain_patches_are_bit_identical(cae, c, ps, normalize):
    got = gathered(cae, c, ps, normalize, False, 0.0)
    assert got.shape == (N, c, ps, ps) and got.dtype == torch.float32 and got.is_cuda
    want = restated(c, ps, normalize, False, 0.0).astype(np.float32)
    assert np.array_equal(got.cpu().numpy(), want)
    assert len(np.unique(pool(c))) == 256  # every quotient u8 / 255 is in play


@pytest.mark.parametrize('normalize', [False, True])
@pytest.mark.parametrize('c,ps', SHAPES)
def test_rotation(cae, c, ps, normalize):
    got = gathered(cae, c, ps, normalize, True, 0.0)
    err, tol = max_err(got, restated(c, ps, normalize, True, 0.0)), bound(ps, normalize, True, 0.0)
    print(f'rotation c={c} ps={ps} normalize={normalize}: err {err:.3e} bound {tol:.3e}')
    assert err <= tol
    # the 0 degree row, given through the rotation pointers, against the output without them
    plain = gathered(cae, c, ps, normalize, False, 0.0)
    zero = float((got[0] - plain[0]).abs().max())
    print(f'  zero angle against no rotation: {zero:.3e}')
    assert zero <= tol


@pytest.mark.parametrize('noise_std', [0.001, 0.05])
@pytest.mark.parametrize('normalize', [False, True])
@pytest.mark.parametrize('c,ps', SHAPES)
def test_noise(cae, c, ps, normalize, noise_std):
    got = gathered(cae, c, ps, normalize, False, noise_std)
    want = restated(c, ps, normalize, False, noise_std)
    err, tol = max_err(got, want), bound(ps, normalize, False, noise_std)
    print(f'noise c={c} ps={ps} normalize={normalize} std={noise_std}: err {err:.3e} bound {tol:.3e}')
    assert err <= tol
    if noise_std == 0.05 and ps == 33:  # the clamp is active (sample 3 lies inside the image), and padding carries no noise
        lo = -1.0 if normalize else 0.0
        assert (want[3] == lo).any() and (want[3] == 1.0).any()
        assert (want[1, :, :3] == lo).all() and (got[1, :, :3] == lo).all()


@pytest.mark.parametrize('noise_std', [0.001, 0.05])
@pytest.mark.parametrize('normalize', [False, True])
@pytest.mark.parametrize('c,ps', SHAPES)
def test_noise_with_rotation(cae, c, ps, normalize, noise_std):
    got = gathered(cae, c, ps, normalize, True, noise_std)
    err, tol = max_err(got, restated(c, ps, normalize, True, noise_std)), bound(ps, normalize, True, noise_std)
    print(f'noise + rotation c={c} ps={ps} normalize={normalize} std={noise_std}: err {err:.3e} bound {tol:.3e}')
    assert err <= tol


@pytest.mark.parametrize('rotate', [False, True])
def test_repeatable_and_independent_of_the_split(cae, rotate):
    c, ps = 3, 33
    tile, y0, x0 = placement(ps)
    angle = ANGLES if rotate else None
    s = sampler(cae, c, ps, True, 0.05)
    a, b = s.gather(tile, y0, x0, angle), s.gather(tile, y0, x0, angle)
    assert torch.equal(a, b)
    parts = [s.gather(tile[:2], y0[:2], x0[:2], angle and angle[:2], sample_base=0),
             s.gather(tile[2:], y0[2:], x0[2:], angle and angle[2:], sample_base=2)]
    assert torch.equal(torch.cat(parts), a)
    assert not torch.equal(s.gather(tile, y0, x0, angle, noise_seed=SEED + 1), a)  # the seed does key the noise


def test_a_tile_outside_the_pool_is_refused_before_the_launch(cae):
    from cnn_autoencoder_amd import _lib
    s = sampler(cae, 3, 8)
    for bad in (T, -1):
        with pytest.raises(ValueError, match='tile'):
            s.gather((0, bad), (0, 0), (0, 0))
    # the entry point itself: CAE_ERR_ARG from the host copy of the indices, with real device pointers
    pool_dev, idx = torch.from_numpy(pool(3)).cuda(), torch.zeros(3, 2, dtype=torch.int32).cuda()
    out = torch.full((2, 3, 8, 8), 7.0, device='cuda')
    host = torch.tensor([0, T], dtype=torch.int32)
    rc = _lib.lib().cae_t_sample_patches(pool_dev.data_ptr(), T, H, W, 3, None, idx[0].data_ptr(), idx[1].data_ptr(),
                                         idx[2].data_ptr(), host.data_ptr(), None, None, 0, 0, 0.0, 0, 2, 8, out.data_ptr(),
                                         _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and bool((out == 7.0).all())  # nothing was written
    # an index that only the device sees selects no image pixel: the patch is padding, and nothing faults
    idx[0, 1] = T
    rc = _lib.lib().cae_t_sample_patches(pool_dev.data_ptr(), T, H, W, 3, None, idx[0].data_ptr(), idx[1].data_ptr(),
                                         idx[2].data_ptr(), None, None, None, 0, 0, 0.0, 0, 2, 8, out.data_ptr(),
                                         _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and bool((out[1] == 0.0).all()) and float(out[0].max()) > 0.0


def test_ragged_tiles_sample_no_padding(cae):
    """the valid size of a tile, not the pool's, is the image: what lies beyond it reads as pad_if_needed's zeros"""
    hw = np.array([[H, W], [10, 9]], dtype=np.int32)
    tile, y0, x0 = (1, 1, 0), (0, 5, 30), (0, 4, 40)
    s = sampler(cae, 3, 8, True, tile_hw=hw)
    want = R.batch(pool(3), tile, y0, x0, 8, normalize=True, tile_hw=hw).astype(np.float32)
    got = s.gather(tile, y0, x0).cpu().numpy()
    assert np.array_equal(got, want)
    assert (got[1, :, 5:] == -1.0).all() and (got[1, :, :, 5:] == -1.0).all() and (got[0] > -1.0).any()
    assert np.array_equal(sampler(cae, 3, 8, True, tile_hw=hw, force_torch=True).gather(tile, y0, x0).cpu().numpy(), want)


@pytest.mark.parametrize('normalize,rotate,noise_std', [(False, False, 0.0), (True, False, 0.0), (True, True, 0.0),
                                                        (False, False, 0.05), (True, True, 0.001), (True, True, 0.05)])
def test_the_torch_form_agrees_with_the_kernel(cae, normalize, rotate, noise_std):
    c, ps = 3, 33
    from cnn_autoencoder_amd.sampler import PatchSampler
    tile, y0, x0 = placement(ps)
    s = PatchSampler(torch.from_numpy(pool(c)).cuda(), ps, add_noise=noise_std != 0.0, noise_std=noise_std,
                     normalize=normalize, seed=SEED, force_torch=True)
    ref = s.gather(tile, y0, x0, ANGLES if rotate else None)
    got = gathered(cae, c, ps, normalize, rotate, noise_std)
    assert ref.is_cuda and ref.shape == got.shape
    err, tol = float((ref.double() - got.double()).abs().max()), bound(ps, normalize, rotate, noise_std)
    print(f'torch form normalize={normalize} rotate={rotate} std={noise_std}: err {err:.3e} bound {tol:.3e}')
    assert err <= tol


def test_sampled_batches_feed_training(cae):
    """train_step on sampler.sample(4) and on the float32-rounded restatement of the same draw (noise and rotation off) give
    exactly the same loss: the batch is in the form the training path takes, the same bits."""
    from cnn_autoencoder_amd import criteria, synth, train
    from cnn_autoencoder_amd.sampler import PatchSampler
    ps, n = 32, 4
    s = PatchSampler(pool(3), ps, data_mode='train')
    x = s.sample(n, torch.Generator().manual_seed(11))
    tile, y0, x0, angle = s.draw(n, torch.Generator().manual_seed(11))
    assert angle is None and x.shape == (n, 3, ps, ps)
    want = torch.from_numpy(R.batch(pool(3), tile.tolist(), y0.tolist(), x0.tolist(), ps).astype(np.float32))
    assert torch.equal(x.cpu(), want)
    cfg = dict(synth.CANONICAL, channels_net=32, channels_bn=48, compression_level=3)
    noise = torch.rand(n, 48, ps // 8, ps // 8, generator=torch.Generator().manual_seed(3)) - 0.5
    losses = []
    for batch in (x, want.cuda()):
        model = cae.autoencoder_from_state_dict(synth.synthetic_state(cfg, seed=22), train=True)
        model['fact_ent'].module.fixed_noise = noise
        ld = train.train_step(batch, model, criteria.GeneralLoss(distortion_lambda=0.01), train.setup_optim(model))
        losses.append(float(ld['loss']))
    assert np.isfinite(losses[0]) and losses[0] == losses[1]
    # and an epoch of batches stands where the reference's train_data stands
    s = PatchSampler(pool(3), ps, batch_size=3, steps_per_epoch=2, add_noise=True, rotation=True, normalize=True)
    batches = list(s)
    assert len(batches) == len(s) == 2 and all(a is b and a.shape == (3, 3, ps, ps) for a, b in batches)
    assert not torch.equal(batches[0][0], batches[1][0])
