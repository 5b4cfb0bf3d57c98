"""The elastic deformation on the device (cae_t_elastic_deform through sampler.elastic_deform and both samplers) against
the float64 restatement of its contract (tests/sampler_elastic_restatement.py).

Shapes (patch side, samples, image channels, mask channels, sigma of the displacement draw):
  2 and 5 with sigma 1.5   taps and displaced points cross an edge, at 2 more than once (a tap index beyond one
                           reflection), and the clamp stays inactive (both asserted; the generator seeds of these two
                           draws were searched for that on the inputs alone);
  8 with sigma 10          the clamp to [-ps, 2 ps] is active (asserted) and is restated;
  33 with sigma 10         odd, no multiple of 4;
  128, n = 2, c = 3, kt = 3   the largest plane kept in LDS;
  130, n = 1, c = 1, kt = 1   the global-memory variant (8 whole strips of 16 rows and one of 2);
  33 and 130 with kt = 0      the image-only form.
Images are uniform in [-1, 1], masks hold the integers 0..3, displacement grids are N(0, sigma^2) from a seeded generator.

Image bound, with u = 2^-24, G = 3 the l1 gain of the prefilter along one axis, X = max|x_in|, A the largest interpolation
coefficient of the batch in magnitude and F the largest field coefficient in magnitude (A, X, F from the restatement):
  prefilter    16 G^2 X u    at most 8 roundings per value and axis (scale, two per step of either recursion, the end
                             value's factor), each relative u on a value that the rest of the axis' steps carry to the output
                             with the rest of the l1 gain G; the first axis' error passes the second (G), the second axis'
                             input is at most G X.  The dropped start terms weigh below 2^-41 and are covered by the slack.
  coordinates  4 A delta     delta = (2 ps + 96 F) u bounds the error of either source coordinate:
                             - u_i = fl(fl(i) fl(2 / (ps - 1))) is within 4 u of its value (two relative roundings, u_i <= 2);
                             - one beta: its argument u_i - k adds a rounding (5 u in all), |beta'| <= 3/4 carries that as
                               3.75 u, and its four polynomial roundings on magnitudes up to 4/3 add 5.4 u: below 10 u;
                             - W_0 and W_2 are one beta; W_1 is a sum of three of which at most two are non-zero at a time
                               (20 u) and two additions of values up to 1 (2 u): 22 u; the three together 42 u;
                             - D = sum W_a W_b coef with sum W = 1 and |coef| <= F: 2 x 42 F u from the weights, 12 F u from
                               its nine products and eight sums: 96 F u;
                             - i + D rounds once on a magnitude the clamp keeps within 2 ps: 2 ps u; the clamp is
                               1-Lipschitz and exact.
                             The spline is 2 A-Lipschitz per axis (sum |beta'| <= 3/2 < 2) and continuous where the tap window
                             moves, so a window chosen differently in float32 costs nothing more; two axes.
  taps         32 A u        weights of a few ulp (9 u per product of two), 16 products and sums on |cf| <= A with unit-sum
                             positive weights.
A sample whose field coefficients are NaN or beyond 1e20 has exact coordinates (the clamp's bound itself) and does not count
into F.
Mask rule: t is compared exactly; a pixel is left out only where y + 0.5 or x + 0.5 of the float64 source point lies within
delta + 2 ps u (the coordinate error plus the rounding of the sum y + 0.5) of an integer: at most 1 % of a sample's pixels,
none at zero displacement.  Both are asserted.
"""
import functools

import numpy as np
import pytest
import torch

import sampler_elastic_restatement as E
import sampler_labeled_restatement as L
import sampler_restatement as R
import seg_weight_map_oracle as WO
import segmenter_restatement as SR
from residue import poisoned_alloc  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# (ps, n, c, kt, sigma)
CASES = [(2, 4, 3, 3, 1.5), (5, 4, 3, 3, 1.5), (8, 2, 3, 2, 10.0), (33, 2, 3, 1, 10.0), (128, 2, 3, 3, 10.0),
         (130, 1, 1, 1, 10.0), (33, 2, 3, 0, 10.0), (130, 1, 1, 0, 10.0)]
IDS = ['ps{}-n{}-c{}-kt{}-sigma{}'.format(*v) for v in CASES]
UNCLAMPED_DRAW = {2: 13, 5: 0}  # patch side -> seed of a displacement draw that leaves every source point inside (-ps, 2 ps)


@pytest.fixture(scope='module', autouse=True)
def cae(built_lib):
    import cnn_autoencoder_amd as cae
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return cae


@pytest.fixture(autouse=True)
def global_generators_stay():
    """the tests here leave torch's global generators as they found them (samplers iterated without a generator and freshly
    built modules draw from them), so the tests that run after this file see the states they saw before it existed"""
    with torch.random.fork_rng():
        yield


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(x float32, t float32 or None, displacement float64) of a case"""
    ps, n, c, kt, sigma = case
    rng = np.random.default_rng([ps, n, c, kt])
    x = rng.uniform(-1.0, 1.0, (n, c, ps, ps)).astype(np.float32)
    t = rng.integers(0, 4, (n, kt, ps, ps)).astype(np.float32) if kt else None
    d = rng.standard_normal((n, 2, 3, 3)) * sigma
    if ps in UNCLAMPED_DRAW:
        d = np.random.default_rng(UNCLAMPED_DRAW[ps]).standard_normal((n, 2, 3, 3)) * sigma
    for v in (x, t, d):
        if v is not None:
            v.setflags(write=False)
    return x, t, d


@functools.lru_cache(maxsize=None)
def restated(case):
    """(x', t', info) of the restatement, computed once per case and shared"""
    x, t, d = inputs(case)
    info = {}
    want_x, want_t = E.deform(x, t, E.coefficients_f32(d), info=info)
    want_x.setflags(write=False)
    if want_t is not None:
        want_t.setflags(write=False)
    return want_x, want_t, info


def delta(ps, info):
    """the coordinate error of the module docstring"""
    return (2.0 * ps + 96.0 * info['field_max']) * U


def bound(ps, info):
    g, a = E.L1_GAIN, info['coef_max']
    return U * (16.0 * g * g * info['x_max'] + 32.0 * a) + 4.0 * a * delta(ps, info)


def margin(ps, info):
    return delta(ps, info) + 2.0 * ps * U


def check_masks(got, want, coef, ps, info, still=False):
    """the mask rule of the module docstring"""
    for s in range(len(got)):
        skip = E.near_a_tie(*E.source_points(coef[s], ps), margin(ps, info))
        if still:
            assert not skip.any()
        assert skip.mean() <= 0.01, (s, float(skip.mean()))
        assert np.array_equal(got[s][:, ~skip], want[s][:, ~skip]), s


def deform_on_device(x, d, t=None, **kw):
    from cnn_autoencoder_amd.sampler import elastic_deform
    out = elastic_deform(torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(d)),
                         None if t is None else torch.from_numpy(np.array(t)).cuda(), **kw)
    return (out, None) if t is None else out


# ------------------------------------------------------------------------------------------------------ the entry point
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_deformation(case, poisoned_alloc):
    """x within the derived bound of the restatement, t by the mask rule; the outputs and the workspace come poisoned with
    NaN between guard bands, so an unwritten value or a write outside a buffer shows; a second call gives the same bits"""
    ps, n, c, kt, sigma = case
    x, t, d = inputs(case)
    want_x, want_t, info = restated(case)
    got_x, got_t = deform_on_device(x, d, t)
    again_x, again_t = deform_on_device(x, d, t)
    poisoned_alloc.check()
    assert got_x.shape == want_x.shape and got_x.dtype == torch.float32 and got_x.is_cuda
    assert torch.equal(got_x, again_x) and (kt == 0 or torch.equal(got_t, again_t))
    err, tol = float(np.abs(got_x.cpu().numpy().astype(np.float64) - want_x).max()), bound(ps, info)
    print(f'elastic {IDS[CASES.index(case)]}: A {info["coef_max"]:.3f} F {info["field_max"]:.2f} err {err:.3e} '
          f'bound {tol:.3e} ratio {err / tol:.4f}')
    assert err <= tol  # also false for a NaN
    assert info['coef_max'] <= E.L1_GAIN ** 2 * info['x_max'] + 1e-9
    coef = E.coefficients_f32(d)
    if kt:
        assert got_t.shape == want_t.shape
        check_masks(got_t.cpu().numpy(), want_t, coef, ps, info)
    raw = np.stack([np.arange(ps)[:, None] + E.field(cf, ps)[0] for cf in coef])  # the row coordinates before the clamp
    if ps == 8:  # the clamp is active
        assert raw.min() < -ps or raw.max() > 2 * ps
    if ps in UNCLAMPED_DRAW:  # inactive in both coordinates, and beyond an edge
        cols = np.stack([np.arange(ps)[None, :] + E.field(cf, ps)[1] for cf in coef])
        assert min(raw.min(), cols.min()) > -ps and max(raw.max(), cols.max()) < 2 * ps
        assert raw.min() < -0.5 and raw.max() > ps - 0.5
    if ps == 2:  # taps reach beyond one reflection on both sides
        assert np.floor(raw.min()) - 1 < -ps and np.floor(raw.max()) + 2 >= 2 * ps


@pytest.mark.parametrize('ps,kt', [(1, 1), (5, 3), (33, 0), (128, 1), (130, 2)])
def test_zero_displacement_is_the_identity(ps, kt, poisoned_alloc):
    rng = np.random.default_rng(ps)
    x = rng.uniform(-1.0, 1.0, (2, 2, ps, ps)).astype(np.float32)
    t = rng.integers(0, 4, (2, kt, ps, ps)).astype(np.float32) if kt else None
    got_x, got_t = deform_on_device(x, np.zeros((2, 2, 3, 3)), t)
    poisoned_alloc.check()
    info = dict(coef_max=float(np.abs(E.prefilter(x.astype(np.float64))).max()), x_max=1.0, field_max=0.0)
    assert float(np.abs(got_x.cpu().numpy().astype(np.float64) - x).max()) <= bound(ps, info)
    if kt:
        assert np.array_equal(got_t.cpu().numpy(), t)
        check_masks(got_t.cpu().numpy(), t, np.zeros((2, 2, 3, 3), dtype=np.float32), ps, info, still=True)


@pytest.mark.parametrize('case', [CASES[1], CASES[3], CASES[5]], ids=[IDS[1], IDS[3], IDS[5]])
def test_the_host_form_agrees_with_the_kernel(case):
    ps, n, c, kt, sigma = case
    x, t, d = inputs(case)
    info = restated(case)[2]
    gx, gt = deform_on_device(x, d, t)
    hx, ht = deform_on_device(x, d, t, force_torch=True)
    assert hx.is_cuda and hx.shape == gx.shape and ht.shape == gt.shape
    err = float((hx.double() - gx.double()).abs().max())
    print(f'host form ps={ps}: err {err:.3e} bound {bound(ps, info):.3e}')
    assert err <= bound(ps, info) + 2.0 ** -24 * E.L1_GAIN ** 2  # the host form rounds its result to float32 once
    check_masks(gt.cpu().numpy(), ht.cpu().numpy(), E.coefficients_f32(d), ps, info)


@pytest.mark.parametrize('ps', [8, 130])
def test_coefficients_that_are_nan_or_huge_only_move_clamped_coordinates(ps, poisoned_alloc):
    """the entry point with coefficients only the device sees: sample 0 all NaN (every source point becomes (-ps, -ps)),
    sample 1 all 1e30 ((2 ps, 2 ps)), sample 2 an ordinary draw; no error status, every value written and restated"""
    from cnn_autoencoder_amd import _lib
    rng = np.random.default_rng(ps)
    x = rng.uniform(-1.0, 1.0, (3, 2, ps, ps)).astype(np.float32)
    t = rng.integers(0, 4, (3, 1, ps, ps)).astype(np.float32)
    coef = E.coefficients_f32(rng.standard_normal((3, 2, 3, 3)) * 3.0)
    coef[0], coef[1] = np.nan, 1e30
    info = {}
    want_x, want_t = E.deform(x, t, coef, info=info)
    xd, td, cd = (torch.from_numpy(v).cuda() for v in (x, t, coef))
    xo, to = torch.empty_like(xd), torch.empty_like(td)
    ws_bytes = _lib.lib().cae_t_elastic_deform_workspace(3, 2, ps)
    assert ws_bytes == (3 * 2 * ps * ps * 4 if ps > 128 else 0)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device='cuda')
    rc = _lib.lib().cae_t_elastic_deform(xd.data_ptr(), td.data_ptr(), cd.data_ptr(), 3, 2, 1, ps,
                                         ws.data_ptr() if ws_bytes else None, ws_bytes, xo.data_ptr(), to.data_ptr(),
                                         _lib.stream_ptr())
    torch.cuda.synchronize()
    poisoned_alloc.check()
    assert rc == 0 and bool(torch.isfinite(xo).all())
    assert float(np.abs(xo.cpu().numpy().astype(np.float64) - want_x).max()) <= bound(ps, info)
    check_masks(to.cpu().numpy(), want_t, coef, ps, info)
    # the source points of the first two samples are the clamp's bounds: one value each
    assert len(np.unique(to[0].cpu().numpy())) == 1 and len(np.unique(to[1].cpu().numpy())) == 1


# ---------------------------------------------------------------------------------------------------------- the samplers
THREE = dict(class_weights=[1.0, 2.0], weights_map_sigma=5, weights_map_w=10)


def _labeled(**kw):
    from cnn_autoencoder_amd.sampler import LabeledPatchSampler
    rng = np.random.default_rng(21)
    pool = rng.integers(0, 256, (3, 64, 72, 3), dtype=np.uint8)
    labels = np.stack([WO.blobs(64, 72, 0.3, 30 + i, smooth=1.5) for i in range(3)])
    return pool, labels, LabeledPatchSampler(pool, labels, 32, rotation=True, seed=7, batch_size=4, steps_per_epoch=1,
                                             elastic_deformation=True, **kw)


def test_a_labelled_batch_is_rotation_deformation_and_weight_map_chained(poisoned_alloc):
    """x within the rotation's bound (tests/test_sampler_labeled.py) carried through the deformation, whose l-infinity gain
    is at most G^2, plus the deformation's own; labels by both mask rules (a pixel whose source pixel was a tie of the
    rotation is left out too); weights against the oracle on the planes whose labels agree everywhere"""
    import test_sampler_labeled as TL
    ps, n = 32, 4
    pool, labels, s = _labeled(**THREE)
    gen = torch.Generator().manual_seed(3)
    tile, y0, x0, angle = s.draw(n, gen)
    disp = s.draw_displacement(n, gen)
    assert disp.shape == (n, 2, 3, 3) and disp.dtype == torch.float64
    x, t = s.gather(tile, y0, x0, angle, displacement=disp)
    poisoned_alloc.check()
    assert x.shape == (n, 3, ps, ps) and t.shape == (n, 2, ps, ps) and t.dtype == torch.float32
    rot = {}
    x_rot, t_rot = L.batch(pool, labels[..., None], tile.tolist(), y0.tolist(), x0.tolist(), ps, angle=angle.tolist(), info=rot)
    coef, info = E.coefficients_f32(disp.numpy()), {}
    want_x, want_t = E.deform(x_rot, t_rot, coef, info=info)
    tol = bound(ps, info) + E.L1_GAIN ** 2 * TL.bound(ps, rot['coef_max'], False, 0.0)
    err = float(np.abs(x.cpu().numpy().astype(np.float64) - want_x).max())
    print(f'chained batch: err {err:.3e} bound {tol:.3e} ratio {err / tol:.4f}')
    assert err <= tol
    got, compared = t.cpu().numpy(), 0
    for i in range(n):
        y, xx = E.source_points(coef[i], ps)
        ny, nx = (E.reflect(np.floor(v + 0.5).astype(np.int64), ps) for v in (y, xx))
        skip = E.near_a_tie(y, xx, margin(ps, info)) | L.near_a_tie(ps, *R.cos_sin_f32(float(angle[i])))[ny, nx]
        assert skip.mean() <= 0.02
        assert np.array_equal(got[i, 1][~skip], want_t[i, 0][~skip]), i
        if np.array_equal(got[i, 1], want_t[i, 0]):
            o = WO.weight_map(want_t[i, 0], [1.0, 2.0], sigma=5, w_0=10)
            w_tol = (10.0 * WO.bound(o['arg'], o['e']) if o['count'] else 0.0) + 2.0 ** -23 * o['w64'] * (1.0 + 2.0 ** -10)
            assert (np.abs(got[i, 0].astype(np.float64) - o['w64']) <= w_tol).all(), i
            compared += 1
    assert compared >= 1
    # sample() draws the same: tiles and angles, then the displacements
    x2, t2 = s.sample(n, torch.Generator().manual_seed(3))
    assert torch.equal(x2, x) and torch.equal(t2, t)


def test_an_unlabelled_batch_is_the_rotated_batch_deformed():
    from cnn_autoencoder_amd.sampler import PatchSampler, elastic_deform
    pool = np.random.default_rng(2).integers(0, 256, (3, 40, 48, 3), dtype=np.uint8)
    kw = dict(rotation=True, normalize=True, seed=5, batch_size=4, steps_per_epoch=1)
    on, off = PatchSampler(pool, 16, elastic_deformation=True, elastic_sigma=4.0, **kw), PatchSampler(pool, 16, **kw)
    gen = torch.Generator().manual_seed(9)
    tile, y0, x0, angle = on.draw(4, gen)
    disp = on.draw_displacement(4, gen)
    assert float(disp.abs().max()) < 4.0 * 6.0
    got = on.sample(4, torch.Generator().manual_seed(9))
    assert torch.equal(got, elastic_deform(off.gather(tile, y0, x0, angle, noise_seed=off.batch_seed(0)), disp))
    assert not torch.equal(got, off.sample(4, torch.Generator().manual_seed(9)))
    (a, b), = list(on)
    assert a is b and a.shape == (4, 3, 16, 16)


def test_a_deformed_weighted_batch_trains_the_head(cae):
    """one seg_train.train_step with SegLoss('WeightedBCELoss') on the chained batch the iterator yields"""
    from cnn_autoencoder_amd import seg_train as T, synth
    cfg, sd, *_ = SR.load_golden('nobn')
    head = T.JNetTrain(**cfg)
    head.load_state_dict(sd, strict=True)
    head = head.cuda().train()
    codec = cae.ConvolutionalAutoencoder(checkpoint=synth.synthetic_state(
        dict(synth.CANONICAL, channels_net=cfg['channels_net'], channels_bn=cfg['channels_bn'],
             compression_level=cfg['compression_level']), seed=3))
    model = dict(codec._model, seg_model=head)
    (x, t), = list(_labeled(**THREE)[2])
    assert x.shape == (4, 3, 32, 32) and t.shape == (4, 2, 32, 32) and t.is_cuda
    before = [p.detach().clone() for p in head.parameters()]
    out = T.train_step(x, t, model, T.SegLoss('WeightedBCELoss'), T.setup_optim(model, learning_rate=1e-3))
    assert np.isfinite(float(out['class_error']))
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, head.parameters()))
