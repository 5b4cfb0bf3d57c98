"""The border weight map on the device (cae_seg_object_distances and cae_seg_weight_map through segmenters.object_distances
and sampler.WeightsDistances) against the reference's procedure in numpy / scipy (tests/seg_weight_map_oracle.py).

Squared distances are integers and are compared exactly.  The weight is judged per pixel against the float64 oracle.
Its exponential part e = exp(-arg), arg = (d_0 + d_1)^2 / (2 sigma^2) (one object: d_0^2 / (2 sigma^2)), is read off a
map with class weights 0 and w_0 = 1, where product and sum are exact, and must lie within
    (8 arg + 4) 2^-24 e + 2^-126
of the oracle's (seg_weight_map_oracle.bound: five fp32 roundings on the way to arg, each arg 2^-24 relative in e, a few
ulps of expf, about 2x headroom; tests/test_seg_weight_map_host.py shows that the reference's own float32 evaluation uses
about half of it).  The class-weight part is read off a map with w_0 = 0 and is exact, as is the copied target plane.  A
full map cw + w_0 e adds the rounding of its product and of its sum: w_0 times the bound above plus
2^-23 (cw + w_0 e) (1 + 2^-10).

Shapes: the hand-made planes are a few pixels wide; 1 x 1, 1 x 40, 300 x 2, 3 x 1030 (crosses the row pass's chunk of 256
columns four times, with a last chunk of 6), 7 x 257 (one column into a second block of 256), 160 x 160; widths up to 64
take the row pass's 64-lane blocks, wider ones its 256-lane blocks.
"""
import functools

import numpy as np
import pytest
import torch

import seg_weight_map_oracle as WO
import segmenter_restatement as SR
from residue import poisoned_alloc  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def cae(built_lib):
    import cnn_autoencoder_amd as cae
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return cae


def _seg():
    from cnn_autoencoder_amd import segmenters
    return segmenters


def _wd(*a, **kw):
    from cnn_autoencoder_amd.sampler import WeightsDistances
    return WeightsDistances(*a, **kw)


def _plane(rows):
    return np.array([[int(c) for c in r] for r in rows], dtype=np.uint8)


HAND = {
    'empty': np.zeros((5, 7), dtype=np.uint8),
    'one pixel': _plane(['00000', '00000', '00100', '00000']),
    'full': np.ones((6, 5), dtype=np.uint8),
    'two diagonal pixels': _plane(['0100', '1000', '0000']),
    'equidistant': _plane(['00000', '10001', '00000']),
    'four borders': _plane(['0011100', '0000000', '1000001', '1000001', '0000000', '0001000']),
    # column 2: the nearest pixels above and below the middle rows belong to one object (joined through column 0), a
    # third object lies farther down the column, a second one beside it
    'same label above and below': _plane(['11100', '10000', '10001', '10000', '11100', '00000', '00100']),
}
SHAPES = ((1, 1), (1, 40), (300, 2), (3, 1030), (7, 257), (160, 160))


@functools.lru_cache(maxsize=None)
def mask_of(kind, h, w, density, seed):
    if kind == 'blobs':
        m = WO.blobs(h, w, density, seed)
    else:
        m = (np.random.default_rng(seed).random((h, w)) < density).astype(np.uint8)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def oracle_of(kind, h, w, density, seed):
    """(count, d2) of a mask, computed once and shared"""
    count, d2 = WO.squared(mask_of(kind, h, w, density, seed))
    d2.setflags(write=False)
    return count, d2


def device_d2(planes, by_value=False):
    """planes (n, h, w) uint8 on the host -> (labels, count, d2) of the device, on the host"""
    S = _seg()
    labels, count = S.components(torch.from_numpy(np.array(planes)).cuda(), by_value=by_value)
    d2 = S.object_distances(labels)
    return labels.cpu().numpy(), count.cpu().numpy(), d2.cpu().numpy()


def assert_weights(planes, sigma, counts=None):
    """the three maps of the module docstring for planes (n, h, w) of 0 / 1 labels, per pixel against the oracle"""
    t = torch.from_numpy(np.array(planes)).cuda()[:, None].float()
    e_dev = _wd([0.0, 0.0], sigma=sigma, w_0=1)(t).cpu().numpy()
    cw_dev = _wd([0.75, 3.0], sigma=sigma, w_0=0)(t).cpu().numpy()
    full_dev = _wd([0.75, 3.0], sigma=sigma, w_0=10)(t).cpu().numpy()
    worst = 0.0
    for i, plane in enumerate(planes):
        o = WO.weight_map(plane, [0.75, 3.0], sigma=sigma, w_0=10)
        if counts is not None:
            assert o['count'] == counts[i]
        cw = np.where(plane > 0, np.float32(3.0), np.float32(0.75))
        assert np.array_equal(cw_dev[i, 0], cw)
        for got in (e_dev, cw_dev, full_dev):
            assert np.array_equal(got[i, 1], plane.astype(np.float32))
        if o['count'] == 0:
            assert np.array_equal(e_dev[i, 0], np.zeros_like(cw)) and np.array_equal(full_dev[i, 0], cw)
            continue
        tol = WO.bound(o['arg'], o['e'])
        err = np.abs(e_dev[i, 0].astype(np.float64) - o['e'])
        worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), (i, float((err / tol).max()))
        tol_full = 10.0 * tol + 2.0 ** -23 * o['w64'] * (1.0 + 2.0 ** -10)
        assert (np.abs(full_dev[i, 0].astype(np.float64) - o['w64']) <= tol_full).all(), i
    print(f'sigma {sigma}: worst exponential error / bound {worst:.3f}')


# ------------------------------------------------------------------------------------------------------ distances
@pytest.mark.parametrize('name', list(HAND))
def test_hand_made_planes(name):
    plane = HAND[name]
    count, want = WO.squared(plane)
    _, got_count, got = device_d2(plane[None])
    assert got_count.tolist() == [count]
    assert np.array_equal(got[0], want)
    if name == 'empty':
        assert (got == -1).all()
    if name in ('one pixel', 'full', 'two diagonal pixels'):
        assert count == 1 and (got[0, 1] == -1).all() and (got[0, 0] >= 0).all()
    if name == 'full':
        assert (got[0, 0] == 0).all()
    if name == 'equidistant':
        assert got[0, :, :, 2].tolist() == [[5, 4, 5], [5, 4, 5]]  # the middle column: both planes hold the same value
    if name == 'same label above and below':
        assert count == 3 and got[0, :, 2, 2].tolist() == [4, 4]  # above and below at 2 rows: one object; the next: (2, 4)
    assert_weights(plane[None], 1.5, [count])


@pytest.mark.parametrize('h,w', SHAPES)
def test_shapes_off_every_grid(h, w):
    # independent pixels at density 0.3 (the one pixel of 1 x 1 set); blobs on the square, where they keep the oracle's
    # one distance transform per object at about a hundred
    case = ('blobs' if h * w > 10000 else 'random', h, w, 0.3 if h * w > 1 else 1.0, h * 10000 + w)
    mask = mask_of(*case)
    count, want = oracle_of(*case)
    assert count >= 1
    _, got_count, got = device_d2(mask[None])
    assert got_count.tolist() == [count]
    assert np.array_equal(got[0], want)


@pytest.mark.parametrize('kind,density', [('random', 0.02), ('random', 0.5), ('random', 0.9), ('blobs', 0.02), ('blobs', 0.3),
                                          ('blobs', 0.9)])
def test_random_and_blob_masks(kind, density):
    h, w = 61, 83
    mask = mask_of(kind, h, w, density, 11)
    count, want = oracle_of(kind, h, w, density, 11)
    _, got_count, got = device_d2(mask[None])
    assert got_count.tolist() == [count]
    assert np.array_equal(got[0], want)
    if kind == 'blobs':
        assert_weights(mask[None], 5, [count])


def batch_of_three():
    many = mask_of('blobs', 160, 160, 0.25, 7)
    one = np.zeros_like(many)
    one[40:50, 100:130] = 1
    return np.stack([np.zeros_like(many), one, many])


def test_a_batch_of_planes_with_no_one_and_many_objects():
    """planes do not see each other, and each takes the form of its own object count"""
    planes = batch_of_three()
    _, got_count, got = device_d2(planes)
    many_count, many_d2 = oracle_of('blobs', 160, 160, 0.25, 7)
    assert got_count.tolist() == [0, 1, many_count] and many_count > 20
    assert (got[0] == -1).all()
    assert np.array_equal(got[1], WO.squared(planes[1])[1]) and (got[1, 1] == -1).all()
    assert np.array_equal(got[2], many_d2)
    for sigma in (1, 5, 20):
        assert_weights(planes, sigma, [0, 1, many_count])


def test_results_do_not_depend_on_what_the_buffers_held(poisoned_alloc):
    """output and workspace come poisoned (torch.empty under the fixture), between guard bands; twice the same bits"""
    S = _seg()
    planes = np.stack([mask_of('blobs', 7, 257, 0.3, 3), mask_of('random', 7, 257, 0.1, 4)])
    want = np.stack([oracle_of('blobs', 7, 257, 0.3, 3)[1], oracle_of('random', 7, 257, 0.1, 4)[1]])
    labels, _ = S.components(torch.from_numpy(planes).cuda())
    first = S.object_distances(labels)
    second = S.object_distances(labels)
    assert poisoned_alloc.check() >= 4
    assert torch.equal(first, second)
    assert np.array_equal(first.cpu().numpy(), want)
    t = torch.from_numpy(planes).cuda()[:, None].float()
    a, b = _wd([1.0, 2.0], 3, 10)(t), _wd([1.0, 2.0], 3, 10)(t)
    assert poisoned_alloc.check() >= 2
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())


def test_labels_by_value_are_accepted():
    """touching regions of different values are objects of their own: distinct labels are all that matter"""
    rng = np.random.default_rng(9)
    plane = (mask_of('blobs', 40, 70, 0.5, 5) * rng.integers(1, 4, (40, 70))).astype(np.uint8)
    labels, count, got = device_d2(plane[None], by_value=True)
    want_count, want = WO.squared(None, labels=labels[0])
    assert count.tolist() == [want_count] and want_count > int(device_d2(plane[None])[1][0])
    assert np.array_equal(got[0], want)
    assert (got[0, 1][plane > 0] > 0).all()  # the second distance of a foreground pixel is to another object


# ------------------------------------------------------------------------------------------------------ the map
def test_a_label_outside_the_table_gives_nan_and_the_flag():
    plane = mask_of('blobs', 21, 70, 0.3, 2).astype(np.float32)
    ys, xs = np.nonzero(plane)
    bad = plane.copy()
    bad[ys[0], xs[0]], bad[ys[1], xs[1]], bad[ys[2], xs[2]] = 2.0, np.nan, -1.0  # still foreground: the objects stay
    wd = _wd([1.0, 2.0], sigma=4, w_0=10)
    clean = wd(torch.from_numpy(plane).cuda()[None, None]).cpu().numpy()
    got = wd.apply(torch.from_numpy(bad).cuda()[None, None], check=False).cpu().numpy()
    hit = np.zeros(plane.shape, dtype=bool)
    hit[ys[:3], xs[:3]] = True
    assert np.isnan(got[0, 0][hit]).all()
    assert np.array_equal(got[0, 0][~hit], clean[0, 0][~hit])
    assert np.array_equal(got[0, 1], bad, equal_nan=True)
    with pytest.raises(IndexError, match='outside the 2 class weights'):
        wd(torch.from_numpy(bad).cuda()[None, None])
    assert np.array_equal(wd(torch.from_numpy(plane).cuda()[None, None]).cpu().numpy(), clean)  # and the next call is clean


def test_int64_targets_and_the_host_procedure():
    planes = batch_of_three()[:, 30:70, 90:150]
    t = torch.from_numpy(np.array(planes)).cuda()[:, None]
    wd = _wd([0.75, 3.0], sigma=5, w_0=10)
    got = wd(t.long())
    assert got.dtype == torch.float32 and got.shape == (3, 2, 40, 60) and torch.equal(got, wd(t.float()))
    host = _wd([0.75, 3.0], sigma=5, w_0=10, force_torch=True)(t.float())
    assert host.is_cuda and torch.equal(host[:, 1], got[:, 1])
    for i, plane in enumerate(planes):
        o = WO.weight_map(plane, [0.75, 3.0], sigma=5, w_0=10)
        if o['count'] == 0:
            assert torch.equal(host[i], got[i])
            continue
        tol = 10.0 * WO.bound(o['arg'], o['e']) + 2.0 ** -23 * o['w64'] * (1.0 + 2.0 ** -10)
        for v in (host, got):
            assert (np.abs(v[i, 0].cpu().numpy().astype(np.float64) - o['w64']) <= tol).all()
    with pytest.raises(ValueError, match='one target channel'):
        wd(torch.cat([t, t], dim=1).float())


# --------------------------------------------------------------------------------------------------- the sampler
def _labeled(**kw):
    from cnn_autoencoder_amd.sampler import LabeledPatchSampler
    rng = np.random.default_rng(21)
    pool = rng.integers(0, 256, (3, 64, 72, 3), dtype=np.uint8)
    labels = np.stack([WO.blobs(64, 72, 0.3, 30 + i, smooth=1.5) for i in range(3)])
    return LabeledPatchSampler(pool, labels, 32, rotation=True, seed=7, batch_size=4, steps_per_epoch=1, **kw)


THREE = dict(class_weights=[1.0, 2.0], weights_map_sigma=5, weights_map_w=10)


def test_the_sampler_puts_the_map_in_front_of_its_labels():
    gen = lambda: torch.Generator().manual_seed(3)  # noqa: E731
    x0, t0 = _labeled().sample(4, gen())
    x1, t1 = _labeled(**THREE).sample(4, gen())
    assert torch.equal(x0, x1)
    assert t1.dtype == torch.float32 and t1.shape == (4, 2, 32, 32) and t0.shape == (4, 1, 32, 32)
    assert torch.equal(t1[:, 1:], t0)
    assert torch.equal(t1, _wd([1.0, 2.0], sigma=5, w_0=10)(t0))
    assert 0 < int((t0 != 0).sum()) < t0.numel()
    # the host procedure on the same labels, per pixel within the map's bound
    host = _wd([1.0, 2.0], sigma=5, w_0=10, force_torch=True)(t0)
    for i in range(4):
        o = WO.weight_map(t0[i, 0].cpu().numpy(), [1.0, 2.0], sigma=5, w_0=10)
        assert o['count'] >= 1
        tol = 10.0 * WO.bound(o['arg'], o['e']) + 2.0 ** -23 * o['w64'] * (1.0 + 2.0 ** -10)
        for v in (host, t1):
            assert (np.abs(v[i, 0].cpu().numpy().astype(np.float64) - o['w64']) <= tol).all()
    # an int64 sampler hands out the same fp32 pair
    _, t2 = _labeled(target_data_type=torch.int64, **THREE).sample(4, gen())
    assert torch.equal(t2, t1)


def test_a_weighted_batch_trains_the_head(cae):
    """one seg_train.train_step with SegLoss('WeightedBCELoss') on a batch the iterator yields: the one-class golden head"""
    from cnn_autoencoder_amd import seg_train as T, synth
    cfg, sd, *_ = SR.load_golden('nobn')
    head = T.JNetTrain(**cfg)
    head.load_state_dict(sd, strict=True)
    head = head.cuda().train()
    codec = cae.ConvolutionalAutoencoder(checkpoint=synth.synthetic_state(
        dict(synth.CANONICAL, channels_net=cfg['channels_net'], channels_bn=cfg['channels_bn'],
             compression_level=cfg['compression_level']), seed=3))
    model = dict(codec._model, seg_model=head)
    (x, t), = list(_labeled(**THREE))
    assert x.shape == (4, 3, 32, 32) and t.shape == (4, 2, 32, 32) and t.is_cuda
    before = [p.detach().clone() for p in head.parameters()]
    out = T.train_step(x, t, model, T.SegLoss('WeightedBCELoss'), T.setup_optim(model, learning_rate=1e-3))
    assert np.isfinite(float(out['class_error']))
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, head.parameters()))
