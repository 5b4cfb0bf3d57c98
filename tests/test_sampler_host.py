"""Host side of the device patch sampler (cnn_autoencoder_amd/sampler.py, cae_t_sample_patches): the float64 restatement the
GPU tests judge the kernel by is itself checked here, against torch's bilinear resampler, a hand-made rotation answer, the
published Philox test vectors and the moments of a normal; then the draw policies and the entry point's argument checks.
No test here needs a GPU.
"""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sampler_restatement as R


@pytest.mark.parametrize('ps', [8, 33])
@pytest.mark.parametrize('angle', [30.0, -30.0, 17.3])
def test_restated_rotation_is_the_affine_grid_sample(ps, angle):
    """The four-tap rotation of the contract equals F.grid_sample(F.affine_grid(theta), bilinear, zeros,
    align_corners=False) in float64 to 1e-12, theta = [[cos, -sin, 0], [sin, cos, 0]] built from the same cos and sin.
    That is the composition torchvision's tensor `rotate` uses; torchvision is not installed, so parity with
    torchvision.transforms.RandomRotation itself is unpinned."""
    rng = np.random.default_rng(ps)
    p = rng.uniform(-1.0, 1.0, (3, ps, ps))
    c, s = R.cos_sin_f32(angle)
    want = R.rotate(p, c, s)
    theta = torch.tensor([[[float(c), -float(s), 0.0], [float(s), float(c), 0.0]]], dtype=torch.float64)
    grid = F.affine_grid(theta, [1, 3, ps, ps], align_corners=False)
    got = F.grid_sample(torch.from_numpy(p)[None], grid, mode='bilinear', padding_mode='zeros', align_corners=False)[0].numpy()
    assert np.abs(got - want).max() <= 1e-12


def test_a_positive_angle_turns_counter_clockwise():
    """One bright pixel 5 to the right of the centre of a 33 x 33 patch, turned by +90 degrees, lands 5 above the centre
    (a smaller row index, the same distance)."""
    ps, c = 33, 16
    p = np.zeros((1, ps, ps))
    p[0, c, c + 5] = 1.0
    out = R.rotate(p, *R.cos_sin_f32(90.0))
    assert np.unravel_index(np.argmax(out[0]), (ps, ps)) == (c - 5, c)
    assert out[0, c - 5, c] > 1.0 - 1e-6
    assert out.sum() < 1.0 + 1e-6


def test_philox_known_answers():
    """Philox4x32-10 against the test vectors published with Random123 (Salmon et al., SC'11; kat_vectors)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for counter, key, want in kat:
        assert tuple(int(w) for w in R.philox4x32_10(counter, key)) == want
    # the product's host generator (what force_torch uploads) is the same function
    from cnn_autoencoder_amd.sampler import philox_normals
    s, px = np.arange(3)[:, None], np.arange(50)
    assert np.array_equal(philox_normals(0x0123456789abcdef, s, px), R.normals(0x0123456789abcdef, s, px))


def test_noise_moments():
    """2 * 10^5 normals of the restatement: the sample mean within 5 / sqrt(N) and the sample variance within
    5 * sqrt(2 / N) of a standard normal's (five standard errors each)."""
    g = R.normals(20240229, np.arange(50)[:, None], np.arange(1000)).reshape(-1)
    n = g.size
    assert n == 200000
    assert abs(g.mean()) <= 5.0 / math.sqrt(n)
    assert abs(g.var() - 1.0) <= 5.0 * math.sqrt(2.0 / n)
    assert np.abs(g).max() <= math.sqrt(2.0 * 33.0 * math.log(2.0))  # u >= 2^-33


def _sampler(h, w, ps, mode, tiles=3, **kw):
    from cnn_autoencoder_amd.sampler import PatchSampler
    return PatchSampler(np.zeros((tiles, h, w, 3), dtype=np.uint8), ps, data_mode=mode, **kw)


def test_train_draws_stay_in_their_ranges():
    gen = torch.Generator().manual_seed(1)
    # both sides at least the patch: offsets in [0, dim - ps]
    tile, y0, x0, angle = _sampler(37, 45, 33, 'train').draw(4000, gen)
    assert angle is None and tile.dtype == y0.dtype == x0.dtype == torch.int32
    assert (int(tile.min()), int(tile.max())) == (0, 2)
    assert (int(y0.min()), int(y0.max())) == (0, 4) and (int(x0.min()), int(x0.max())) == (0, 12)
    # a side smaller than the patch: pad_if_needed pads both sides by ps - dim, offsets in [-(ps - dim), 0]
    tile, y0, x0, _ = _sampler(37, 45, 40, 'train').draw(4000, gen)
    assert (int(y0.min()), int(y0.max())) == (-3, 0) and (int(x0.min()), int(x0.max())) == (0, 5)
    # the valid size of a ragged tile, not the pool's, bounds the draw
    s = _sampler(37, 45, 8, 'train', tiles=2, tile_hw=[[37, 45], [10, 9]])
    tile, y0, x0, _ = s.draw(4000, gen)
    small = tile == 1
    assert int(y0[small].max()) == 2 and int(x0[small].max()) == 1 and int(y0[~small].max()) == 29
    # angles
    _, _, _, angle = _sampler(37, 45, 8, 'train', rotation=True, degrees=30.0).draw(4000, gen)
    assert angle.dtype == torch.float64 and -30.0 <= float(angle.min()) < -29.0 and 29.0 < float(angle.max()) <= 30.0


def test_centre_crop_offsets_and_tile_order():
    # dim - ps = 4, 5 (even, odd, dim larger) and -3, -4 (dim smaller): torchvision's center_crop
    for dim, ps, want in ((37, 33, 2), (38, 33, 2), (39, 32, 4), (37, 40, -1), (36, 40, -2), (35, 40, -2), (33, 33, 0)):
        s = _sampler(dim, 50, ps, 'test')
        tile, y0, x0, angle = s.draw(5)
        assert y0.tolist() == [want] * 5, (dim, ps)
        assert want == (int(round((dim - ps) / 2.0)) if dim >= ps else -((ps - dim) // 2))
        assert tile.tolist() == [0, 1, 2, 0, 1] and angle is None
        assert s.draw(2)[0].tolist() == [2, 0]  # in order, across draws


def test_the_same_generator_state_gives_the_same_draw():
    s = _sampler(37, 45, 16, 'train', rotation=True)
    a = s.draw(64, torch.Generator().manual_seed(7))
    b = s.draw(64, torch.Generator().manual_seed(7))
    c = s.draw(64, torch.Generator().manual_seed(8))
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert not torch.equal(a[1], c[1])
    assert s.batch_seed(0) != s.batch_seed(1) and s.batch_seed(3) == s.batch_seed(3)
    assert len(s) == 1 and s.batch_size == 16


def test_from_zarr_keeps_the_valid_size_of_ragged_tiles(tmp_path):
    from cnn_autoencoder_amd.sampler import PatchSampler
    from cnn_autoencoder_amd.zarrio import ZarrArray
    rng = np.random.default_rng(0)
    stores = []
    for k, shape in enumerate(((40, 70, 3), (32, 32, 3))):
        image = rng.integers(1, 256, shape, dtype=np.uint8)
        store = str(tmp_path / f's{k}.zarr')
        ZarrArray.create(store, '0/0', shape, (32, 32, 3), np.uint8)[:] = image
        stores.append((store, image))
    s = PatchSampler.from_zarr([st for st, _ in stores], '0/0', patch_size=8)
    assert tuple(s.pool.shape) == (7, 32, 32, 3)
    assert s.tile_hw.tolist() == [[32, 32], [32, 32], [32, 6], [8, 32], [8, 32], [8, 6], [32, 32]]
    assert np.array_equal(s.pool[2, :, :6].numpy(), stores[0][1][:32, 64:70])
    assert np.array_equal(s.pool[6].numpy(), stores[1][1])
    tile, y0, x0, _ = s.draw(2000, torch.Generator().manual_seed(0))
    hw = s.tile_hw[tile.long()]
    # a tile at least as large as the patch is sampled inside its valid part; a smaller one with the patch covering it
    assert bool(((y0 >= torch.clamp(hw[:, 0] - 8, max=0)) & (y0 <= torch.clamp(hw[:, 0] - 8, min=0))).all())
    assert bool(((x0 >= torch.clamp(hw[:, 1] - 8, max=0)) & (x0 <= torch.clamp(hw[:, 1] - 8, min=0))).all())


def test_bad_arguments_are_refused_on_the_host(built_lib):
    """c = 5, ps = 0 and a NULL output return CAE_ERR_ARG before anything touches a device (the pointers given here are
    never followed).  The checks that need real device memory are in the GPU tests."""
    from cnn_autoencoder_amd import _lib
    fn = _lib.lib().cae_t_sample_patches
    p = ctypes.c_void_p(4096)

    def call(c=3, ps=8, out=p, n=2, pool=p, tile_host=None, sin=None):
        return fn(pool, 2, 37, 45, c, None, p, p, p, tile_host, None, sin, 0, 0, 0.0, 0, n, ps, out, None)

    assert call(c=5) == -1 and call(c=0) == -1
    assert b'channels' in _lib.lib().cae_last_error()
    assert call(ps=0) == -1
    assert call(out=None) == -1 and call(pool=None) == -1
    assert call(sin=p) == -1  # a sine without a cosine
    assert call(n=-1) == -1
    tiles = (ctypes.c_int32 * 2)(0, 2)
    assert call(tile_host=ctypes.cast(tiles, ctypes.c_void_p)) == -1  # tile 2 of 2, seen in the host copy
    assert b'tile 2' in _lib.lib().cae_last_error()
    with pytest.raises(ValueError):
        _lib.check(call(c=5))
