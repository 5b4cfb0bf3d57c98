"""Host side of the labelled device sampler (sampler.LabeledPatchSampler, cae_t_sample_labeled_patches): the float64
restatement the GPU tests judge the kernels by (tests/sampler_labeled_restatement.py) is itself checked here, against
scipy.ndimage.rotate where scipy is exact and against the identity at angle 0 where it is not; then the draw policy, the
input checks, from_zarr and the entry point's argument checks.  No test here needs a GPU.
"""
import ctypes

import numpy as np
import pytest
import torch

import sampler_labeled_restatement as L
import sampler_restatement as R

ANGLES = (0.0, 7.3, 29.9)


def _cos_sin(angle):
    a = np.deg2rad(np.float64(angle))
    return np.cos(a), np.sin(a)


@pytest.mark.parametrize('angle', ANGLES)
@pytest.mark.parametrize('ps', [16, 33, 64])
def test_restated_image_rotation_is_scipys(ps, angle):
    """order 4, reshape=False, mode='reflect', to 1e-12 from 16 pixels per side on (below about 12 scipy's own start of
    the prefilter is approximate; the contract is the exact form)"""
    ndimage = pytest.importorskip('scipy.ndimage')
    p = np.random.default_rng(ps).uniform(-1.0, 1.0, (2, ps, ps))
    got = L.rotate_image(p, *_cos_sin(angle))
    want = np.stack([ndimage.rotate(q, angle, order=4, reshape=False, mode='reflect') for q in p])
    assert np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize('angle', ANGLES)
@pytest.mark.parametrize('ps', [2, 5, 8, 33])
def test_restated_mask_rotation_is_scipys(ps, angle):
    """order 0 exactly, at every size"""
    ndimage = pytest.importorskip('scipy.ndimage')
    m = np.random.default_rng(ps).integers(0, 4, (2, ps, ps)).astype(np.float64)
    got = L.rotate_mask(m, *_cos_sin(angle))
    want = np.stack([ndimage.rotate(q, angle, order=0, reshape=False, mode='reflect') for q in m])
    assert np.array_equal(got, want)


def test_scipy_rotates_an_hwc_array_plane_by_plane():
    """the reference hands scipy (H, W, C): the default axes turn the first two, each channel on its own"""
    ndimage = pytest.importorskip('scipy.ndimage')
    p = np.random.default_rng(3).uniform(-1.0, 1.0, (3, 16, 16))
    for order, mine in ((4, L.rotate_image), (0, L.rotate_mask)):
        want = ndimage.rotate(p.transpose(1, 2, 0), 7.3, order=order, reshape=False, mode='reflect').transpose(2, 0, 1)
        assert np.abs(mine(p, *_cos_sin(7.3)) - want).max() <= 1e-12


@pytest.mark.parametrize('ps', list(range(2, 20)) + [33, 64])
def test_angle_zero_reproduces_the_patch(ps):
    """the spline interpolates at every size from 2 up: the exactness scipy lacks below 12 pixels per side"""
    p = np.random.default_rng(ps).uniform(-1.0, 1.0, (1, ps, ps))
    assert np.abs(L.rotate_image(p, 1.0, 0.0) - p).max() <= 1e-12
    m = np.random.default_rng(ps).integers(0, 4, (2, ps, ps)).astype(np.float64)
    assert np.array_equal(L.rotate_mask(m, 1.0, 0.0), m)


def test_the_prefilter_l1_gain():
    """the l1 norm of the prefilter's impulse response along one axis is (prod (1 + |z|) / (1 - |z|))^2 = 4.8: what the
    bound of the GPU tests is built from"""
    e = np.zeros(65)
    e[32] = 1.0
    assert abs(np.abs(L.prefilter_line(e)).sum() - L.L1_GAIN) <= 1e-9 and abs(L.L1_GAIN - 4.8) <= 1e-9
    assert abs(L.GAIN - 384.0) <= 1e-9
    d = np.linspace(-0.5, 0.5, 101)[:, None] - np.arange(-2, 3)
    assert np.abs(L.weight(d).sum(axis=1) - 1.0).max() <= 1e-15 and (L.weight(d) >= 0.0).all()


def _sampler(ps=8, tiles=3, h=37, w=45, k=2, **kw):
    from cnn_autoencoder_amd.sampler import LabeledPatchSampler
    return LabeledPatchSampler(np.zeros((tiles, h, w, 3), dtype=np.uint8), np.zeros((tiles, h, w, k), dtype=np.uint8), ps, **kw)


def test_draw_turns_pairs_by_an_angle_in_zero_to_degrees():
    s = _sampler(rotation=True, degrees=30.0)
    tile, y0, x0, angle = s.draw(4000, torch.Generator().manual_seed(1))
    assert angle.dtype == torch.float64 and 0.0 <= float(angle.min()) < 1.0 and 29.0 < float(angle.max()) < 30.0
    assert tile.dtype == y0.dtype == x0.dtype == torch.int32
    assert (int(y0.min()), int(y0.max())) == (0, 29) and (int(x0.min()), int(x0.max())) == (0, 37)
    a = s.draw(64, torch.Generator().manual_seed(7))
    b = s.draw(64, torch.Generator().manual_seed(7))
    c = s.draw(64, torch.Generator().manual_seed(8))
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and not torch.equal(a[3], c[3])
    assert _sampler().draw(4)[3] is None
    # the unlabelled sampler keeps its symmetric policy
    from cnn_autoencoder_amd.sampler import PatchSampler
    plain = PatchSampler(np.zeros((3, 37, 45, 3), dtype=np.uint8), 8, rotation=True)
    assert float(plain.draw(4000, torch.Generator().manual_seed(1))[3].min()) < -29.0


def test_image_and_mask_share_the_offsets():
    """one draw addresses both pools: a label pool that copies an image channel comes back as 255 x that channel of x"""
    from cnn_autoencoder_amd.sampler import LabeledPatchSampler
    rng = np.random.default_rng(5)
    pool = rng.integers(0, 256, (3, 20, 24, 3), dtype=np.uint8)
    s = LabeledPatchSampler(pool, pool[..., 1], 16, force_torch=True, tile_hw=[[20, 24], [10, 9], [20, 24]])
    tile, y0, x0, angle = s.draw(32, torch.Generator().manual_seed(2))
    x, t = s.gather(tile, y0, x0, angle)
    assert angle is None and x.shape == (32, 3, 16, 16) and t.shape == (32, 1, 16, 16) and t.dtype == torch.float32
    assert torch.equal(t[:, 0], torch.round(x[:, 1] * 255.0))
    want_x, want_t = L.batch(pool, pool[..., 1:2], tile.tolist(), y0.tolist(), x0.tolist(), 16, tile_hw=s.tile_hw.tolist())
    assert np.array_equal(x.numpy(), want_x.astype(np.float32)) and np.array_equal(t.numpy(), want_t)
    # the ragged tile holds 10 x 9 pixels: nothing beyond them is sampled as label
    assert bool((tile == 1).any()) and int((t[tile == 1] != 0).flatten(1).sum(1).max()) <= 90


def test_the_host_form_is_the_restatement():
    """force_torch against the restatement, rotation, noise and normalisation on: the only differences are p rounded to
    float32 on the way in (its own error times the prefilter's gain) and the result rounded to float32"""
    from cnn_autoencoder_amd.sampler import LabeledPatchSampler
    rng = np.random.default_rng(0)
    pool, lab = rng.integers(0, 256, (2, 37, 45, 3), dtype=np.uint8), rng.integers(0, 2, (2, 37, 45, 3), dtype=np.uint8)
    tile, y0, x0 = (0, 1, 1), (2, -3, 10), (4, -3, 20)
    for ps, map_labels in ((5, False), (33, True)):
        s = LabeledPatchSampler(pool, lab, ps, force_torch=True, normalize=True, add_noise=True, noise_std=0.05,
                                map_labels=map_labels, seed=5, target_data_type=torch.int64)
        x, t = s.gather(tile, y0, x0, ANGLES)
        want_x, want_t = L.batch(pool, lab, tile, y0, x0, ps, ANGLES, seed=5, noise_std=0.05, normalize=True,
                                 map_labels=map_labels)
        assert t.dtype == torch.int64 and np.array_equal(t.numpy(), want_t.astype(np.int64))
        assert np.abs(x.numpy() - want_x).max() <= (L.L1_GAIN ** 2 + 4.0) * 2.0 ** -23


def test_bad_inputs_raise_before_any_library_call(monkeypatch):
    from cnn_autoencoder_amd import _lib
    from cnn_autoencoder_amd.sampler import LabeledPatchSampler
    monkeypatch.setattr(_lib, 'lib', lambda: pytest.fail('the library was called'))
    pool = np.zeros((3, 37, 45, 3), dtype=np.uint8)
    for labels in (np.zeros((3, 37, 44), dtype=np.uint8), np.zeros((2, 37, 45, 1), dtype=np.uint8),
                   np.zeros((3, 37, 45, 5), dtype=np.uint8), np.zeros((3, 37, 45), dtype=np.int64)):
        with pytest.raises(ValueError):
            LabeledPatchSampler(pool, labels, 8)
    with pytest.raises(ValueError, match='not supported'):
        LabeledPatchSampler(pool, np.zeros((3, 37, 45), dtype=np.uint8), 8, target_data_type=torch.float16)
    s = LabeledPatchSampler(pool, np.zeros((3, 37, 45), dtype=np.uint8), 8, force_torch=True)
    with pytest.raises(ValueError, match='tile'):
        s.gather((0, 3), (0, 0), (0, 0))
    assert s.workspace_bytes(4, True) == 0 and s.workspace_bytes(4, False) == 0
    assert _sampler(ps=130).workspace_bytes(4, True) == 4 * 3 * 130 * 130 * 4 and _sampler(ps=130).workspace_bytes(4, False) == 0


def test_iteration_yields_pairs_for_the_losses():
    from cnn_autoencoder_amd.sampler import LabeledPatchSampler
    rng = np.random.default_rng(1)
    pool, lab = rng.integers(0, 256, (4, 20, 24, 3), dtype=np.uint8), rng.integers(0, 2, (4, 20, 24, 2), dtype=np.uint8)
    kw = dict(force_torch=True, rotation=True, batch_size=3, steps_per_epoch=2)
    batches = list(LabeledPatchSampler(pool, lab, 16, **kw))
    assert len(batches) == 2 and all(x.shape == (3, 3, 16, 16) and t.shape == (3, 2, 16, 16) and t.dtype == torch.float32
                                     for x, t in batches)
    assert set(torch.cat([t for _, t in batches]).unique().tolist()) <= {0.0, 1.0}
    batches = list(LabeledPatchSampler(pool, lab, 16, map_labels=True, target_data_type=torch.int64, **kw))
    assert all(t.shape == (3, 16, 16) and t.dtype == torch.int64 and 0 <= int(t.min()) and int(t.max()) <= 2
               for _, t in batches)
    batches = list(LabeledPatchSampler(pool, lab, 16, target_data_type=torch.int64, **kw))
    assert all(t.shape == (3, 2, 16, 16) for _, t in batches)


def test_from_zarr_reads_both_arrays_and_keeps_ragged_tiles(tmp_path):
    from cnn_autoencoder_amd.sampler import LabeledPatchSampler
    from cnn_autoencoder_amd.zarrio import ZarrArray
    rng = np.random.default_rng(0)
    image, mask = rng.integers(1, 256, (40, 70, 3), dtype=np.uint8), rng.integers(1, 3, (40, 70), dtype=np.uint8)
    store = str(tmp_path / 's.zarr')
    ZarrArray.create(store, '0/0', image.shape, (32, 32, 3), np.uint8)[:] = image
    ZarrArray.create(store, 'labels/0/0', mask.shape, (32, 32), np.uint8)[:] = mask
    s = LabeledPatchSampler.from_zarr([store], '0/0', 'labels/0/0', patch_size=8, force_torch=True)
    assert tuple(s.pool.shape) == (6, 32, 32, 3) and tuple(s.labels.shape) == (6, 32, 32, 1)
    assert s.tile_hw.tolist() == [[32, 32], [32, 32], [32, 6], [8, 32], [8, 32], [8, 6]]
    assert np.array_equal(s.labels[5, :8, :6, 0].numpy(), mask[32:, 64:]) and np.array_equal(s.pool[5, :8, :6].numpy(), image[32:, 64:])
    x, t = s.gather((5,), (0,), (0,))
    assert float(t[0, 0, :, :6].min()) >= 1.0 and float(t[0, 0, :, 6:].max()) == 0.0 and float(x[0, :, :, 6:].max()) == 0.0
    # labels of another Y / X shape, or of another chunking, are refused
    ZarrArray.create(store, 'labels/1/0', (40, 64), (32, 32), np.uint8)[:] = mask[:, :64]
    ZarrArray.create(store, 'labels/2/0', mask.shape, (16, 32), np.uint8)[:] = mask
    for group in ('labels/1/0', 'labels/2/0'):
        with pytest.raises(ValueError, match='agree'):
            LabeledPatchSampler.from_zarr(store, '0/0', group, patch_size=8)


def test_bad_arguments_are_refused_on_the_host(built_lib):
    """CAE_ERR_ARG before anything touches a device (the pointers given here are never followed)"""
    from cnn_autoencoder_amd import _lib
    fn = _lib.lib().cae_t_sample_labeled_patches
    p = ctypes.c_void_p(4096)

    def call(c=3, k=2, ps=8, n=2, pool=p, labels=p, x=p, t=p, tile_host=None, cos=None, sin=None, ws=None, ws_bytes=0):
        return fn(pool, labels, 2, 37, 45, c, k, None, p, p, p, tile_host, cos, sin, 0, 0, 0.0, 0, 0, n, ps, ws, ws_bytes, x, t,
                  None)

    err = _lib.lib().cae_last_error
    assert call(c=5) == -1 and call(k=0) == -1 and call(k=5) == -1 and b'label channels' in err()
    assert call(ps=0) == -1 and call(ps=16385) == -1 and b'patch size' in err()
    for name in ('pool', 'labels', 'x', 't'):
        assert call(**{name: None}) == -1 and b'NULL' in err()
    assert call(sin=p) == -1 and call(n=-1) == -1
    tiles = (ctypes.c_int32 * 2)(0, 2)
    assert call(tile_host=ctypes.cast(tiles, ctypes.c_void_p)) == -1 and b'tile 2' in err()
    # rotated patches above 128 need n c ps^2 floats of workspace; the message names the bytes
    need = 2 * 3 * 130 * 130 * 4
    assert call(ps=130, cos=p, sin=p) == -1 and str(need).encode() in err()
    assert call(ps=130, cos=p, sin=p, ws=p, ws_bytes=need - 1) == -1 and str(need).encode() in err()
    assert call(n=0) == 0 and call(ps=130, n=0, cos=p, sin=p) == 0
    with pytest.raises(ValueError):
        _lib.check(call(k=5))
