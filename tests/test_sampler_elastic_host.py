"""Host side of the elastic deformation (sampler.elastic_deform, cae_t_elastic_deform): the float64 restatement the GPU
tests judge the kernels by (tests/sampler_elastic_restatement.py) is itself checked here against scipy.ndimage -- the
field against map_coordinates(order=3, mode='mirror'), the whole transform against spline_filter + map_coordinates where
scipy's prefilter is exact, and the stated gap where it is not.  Then the bound of the GPU tests: the float32 walk of the
kernels' arithmetic lies inside it at every GPU shape, and five planted misreadings of the contract lie outside.  Then the
host form, the draws and every refusal.  No test here needs a GPU.
"""
import ctypes

import numpy as np
import pytest
import torch

import sampler_elastic_restatement as E
import test_sampler_elastic as G


@pytest.fixture(autouse=True)
def global_generators_stay():
    """the tests here leave torch's global generators as they found them (samplers iterated without a generator and freshly
    built modules draw from them), so the tests that run after this file see the states they saw before it existed"""
    with torch.random.fork_rng():
        yield


def _grids(n, sigma, seed):
    return np.random.default_rng(seed).standard_normal((n, 2, 3, 3)) * sigma


@pytest.mark.parametrize('ps', [2, 5, 8, 33, 128, 130])
def test_restated_field_is_scipys_mirror_spline(ps):
    ndimage = pytest.importorskip('scipy.ndimage')
    d = _grids(1, 10.0, ps)[0]
    u = 2.0 * np.arange(ps) / (ps - 1)
    ui, uj = np.meshgrid(u, u, indexing='ij')
    got = E.field(E.coefficients(d[None])[0], ps)
    for k in range(2):
        want = ndimage.map_coordinates(d[k], [ui, uj], order=3, mode='mirror')
        assert np.abs(got[k] - want).max() <= 1e-12
    # the control points themselves are interpolated
    if ps % 2:
        assert np.abs(got[:, ::(ps - 1) // 2, ::(ps - 1) // 2] - d).max() <= 1e-12


@pytest.mark.parametrize('ps', [16, 33])
def test_restated_transform_is_scipys(ps):
    """spline_filter + map_coordinates(order=3 / 0, mode='reflect') at the restated source points, from 16 pixels per
    side on, where scipy's start of the prefilter is exact to rounding"""
    ndimage = pytest.importorskip('scipy.ndimage')
    rng = np.random.default_rng(ps)
    x, t = rng.uniform(-1.0, 1.0, (2, 2, ps, ps)), rng.integers(0, 4, (2, 1, ps, ps)).astype(np.float64)
    coef = E.coefficients(_grids(2, 3.0, ps))
    got_x, got_t = E.deform(x, t, coef)
    for s in range(2):
        y, xx = E.source_points(coef[s], ps)
        assert y.min() > -ps and y.max() < 2 * ps and (y.min() < -0.5 or y.max() > ps - 0.5)  # beyond an edge, unclamped
        for ch in range(2):
            cf = ndimage.spline_filter(x[s, ch], order=3, mode='reflect')
            want = ndimage.map_coordinates(cf, [y, xx], order=3, mode='reflect', prefilter=False)
            assert np.abs(got_x[s, ch] - want).max() <= 1e-9
        assert np.array_equal(got_t[s, 0], ndimage.map_coordinates(t[s, 0], [y, xx], order=0, mode='reflect'))


def test_where_scipys_prefilter_parts_from_the_contract():
    """the exact start against scipy's spline_filter1d(order=3, mode='reflect') on lines in [-1, 1]: up to 6e-4 at n = 2,
    1e-6 at 5, 4e-10 at 8 (measured over 20 lines each; the gap scales with the line), equal to rounding from 16; the
    exact form interpolates the line at every n"""
    ndimage = pytest.importorskip('scipy.ndimage')
    for n, lo, hi in ((2, 1e-7, 1e-3), (5, 1e-9, 2e-6), (8, 1e-12, 1e-9), (16, 0.0, 1e-13), (33, 0.0, 1e-13)):
        line = np.random.default_rng(n).uniform(-1.0, 1.0, n)
        c = E.prefilter_line(line)
        gap = np.abs(c - ndimage.spline_filter1d(line, order=3, mode='reflect')).max()
        assert lo <= gap <= hi, (n, gap)
        ext = np.concatenate([c[:1], c, c[-1:]])  # the reflected line
        assert np.abs((ext[:-2] + 4.0 * ext[1:-1] + ext[2:]) / 6.0 - line).max() <= 4e-16 * 4
    e = np.zeros(65)
    e[32] = 1.0
    assert abs(np.abs(E.prefilter_line(e)).sum() - 3.0) <= 1e-9 and abs(E.L1_GAIN - 3.0) <= 1e-12 and abs(E.GAIN - 6.0) <= 1e-12


@pytest.mark.parametrize('ps', list(range(1, 20)) + [33])
def test_zero_displacement_reproduces_the_batch(ps):
    rng = np.random.default_rng(ps)
    x, t = rng.uniform(-1.0, 1.0, (1, 2, ps, ps)), rng.integers(0, 4, (1, 2, ps, ps)).astype(np.float64)
    got_x, got_t = E.deform(x, t, np.zeros((1, 2, 3, 3)))
    assert np.abs(got_x - x).max() <= 1e-12 and np.array_equal(got_t, t)
    fx, ft = E.deform_f32(x, t, np.zeros((1, 2, 3, 3)))
    info = dict(coef_max=float(np.abs(E.prefilter(x)).max()), x_max=1.0, field_max=0.0)
    assert np.abs(fx - x).max() <= G.bound(ps, info) + 2.0 ** -24 and np.array_equal(ft, t)


# ---------------------------------------------------------------------------------------------- the bound of the GPU tests
@pytest.mark.parametrize('case', G.CASES, ids=G.IDS)
def test_the_float32_arithmetic_lies_inside_the_bound(case):
    ps, n, c, kt, sigma = case
    x, t, d = G.inputs(case)
    want_x, want_t, info = G.restated(case)
    coef = E.coefficients_f32(d)
    got_x, got_t = E.deform_f32(x, t, coef)
    err, tol = float(np.abs(got_x.astype(np.float64) - want_x).max()), G.bound(ps, info)
    print(f'float32 walk {G.IDS[G.CASES.index(case)]}: err {err:.3e} bound {tol:.3e} ratio {err / tol:.4f} '
          f'margin {G.margin(ps, info):.2e}')
    assert err <= tol
    if kt:
        G.check_masks(got_t, want_t, coef, ps, info)  # also: the margin leaves out at most 1 % of a sample's pixels


@pytest.mark.parametrize('defect', E.DEFECTS)
@pytest.mark.parametrize('case', [G.CASES[2], G.CASES[3]], ids=[G.IDS[2], G.IDS[3]])
def test_a_planted_defect_falls_outside_the_bound(case, defect):
    ps = case[0]
    x, t, d = G.inputs(case)
    want_x, _, info = G.restated(case)
    bad_x, _ = E.deform(x, t, E.coefficients_f32(d), defect=defect)
    err = float(np.abs(bad_x - want_x).max())
    print(f'{defect} at ps {ps}: err {err:.3e} bound {G.bound(ps, info):.3e}')
    assert err > G.bound(ps, info)


# ------------------------------------------------------------------------------------------------------- the host form
@pytest.mark.parametrize('case', [G.CASES[1], G.CASES[2], G.CASES[3], G.CASES[6]], ids=[G.IDS[i] for i in (1, 2, 3, 6)])
def test_the_host_form_is_the_restatement(case):
    """force_torch against the restatement: the only difference is the result rounded to float32"""
    from cnn_autoencoder_amd.sampler import elastic_deform
    x, t, d = G.inputs(case)
    want_x, want_t, info = G.restated(case)
    out = elastic_deform(torch.from_numpy(np.array(x)), torch.from_numpy(np.array(d)),
                         None if t is None else torch.from_numpy(np.array(t)), force_torch=True)
    got_x, got_t = out if t is not None else (out, None)
    assert got_x.dtype == torch.float32 and not got_x.is_cuda
    assert np.abs(got_x.numpy() - want_x).max() <= 2.0 ** -24 * max(1.0, float(np.abs(want_x).max())) + 1e-12
    if t is not None:
        assert got_t.dtype == torch.float32 and np.array_equal(got_t.numpy(), want_t)
    # float32 displacements on the way in are taken as they are
    again = elastic_deform(torch.from_numpy(np.array(x)), torch.from_numpy(np.array(d)).float().double(), force_torch=True)
    assert torch.equal(again, elastic_deform(torch.from_numpy(np.array(x)), torch.from_numpy(np.array(d)).float(),
                                             force_torch=True))


# ------------------------------------------------------------------------------------------------------------ the draws
def _pools():
    rng = np.random.default_rng(4)
    return rng.integers(0, 256, (3, 20, 24, 3), dtype=np.uint8), rng.integers(0, 3, (3, 20, 24), dtype=np.uint8)


def test_with_the_keyword_off_results_and_generator_states_stay():
    from cnn_autoencoder_amd.sampler import LabeledPatchSampler, PatchSampler
    pool, labels = _pools()
    kw = dict(rotation=True, force_torch=True)
    for make in (lambda **k: PatchSampler(pool, 8, **kw, **k), lambda **k: LabeledPatchSampler(pool, labels, 8, **kw, **k)):
        plain, off = make(), make(elastic_deformation=False, elastic_sigma=3.0)
        g0, g1, g2 = (torch.Generator().manual_seed(11) for _ in range(3))
        want = plain.gather(*plain.draw(4, g0))
        got = off.sample(4, g1)
        assert torch.equal(g0.get_state(), g1.get_state())
        for a, b in zip(want if isinstance(want, tuple) else (want,), got if isinstance(got, tuple) else (got,)):
            assert torch.equal(a, b)
        # on: the draw is the same, the displacement comes after it from the same generator
        on = make(elastic_deformation=True, elastic_sigma=3.0)
        draw = on.draw(4, g2)
        assert all(torch.equal(a, b) for a, b in zip(draw, plain.draw(4, torch.Generator().manual_seed(11))))
        disp = on.draw_displacement(4, g2)
        assert disp.shape == (4, 2, 3, 3) and disp.dtype == torch.float64 and 0.5 < float(disp.std()) / 3.0 < 1.5
        g3 = torch.Generator().manual_seed(11)
        bent = on.sample(4, g3)
        assert torch.equal(g2.get_state(), g3.get_state()) and not torch.equal(g3.get_state(), g1.get_state())
        again = on.gather(*draw, noise_seed=on.batch_seed(0), displacement=disp)
        for a, b in zip(bent if isinstance(bent, tuple) else (bent,), again if isinstance(again, tuple) else (again,)):
            assert torch.equal(a, b)


def test_the_labelled_sampler_deforms_the_pair_before_the_weight_map_and_the_cast():
    from cnn_autoencoder_amd.sampler import LabeledPatchSampler, WeightsDistances, elastic_deform
    pool, labels = _pools()
    kw = dict(rotation=True, force_torch=True, elastic_deformation=True, elastic_sigma=2.0)
    s = LabeledPatchSampler(pool, labels, 8, target_data_type=torch.int64, **kw)
    gen = torch.Generator().manual_seed(5)
    tile, y0, x0, angle = s.draw(3, gen)
    disp = s.draw_displacement(3, gen)
    x, t = s.gather(tile, y0, x0, angle, displacement=disp)
    x0_, t0_ = s.gather(tile, y0, x0, angle)
    wx, wt = elastic_deform(x0_, disp, t0_.float(), force_torch=True)
    assert t.dtype == torch.int64 and torch.equal(x, wx) and torch.equal(t, wt.long())
    assert set(t.unique().tolist()) <= {0, 1, 2} and not torch.equal(t, t0_)
    w = LabeledPatchSampler(pool, labels, 8, class_weights=[1.0, 2.0, 3.0], weights_map_sigma=5, weights_map_w=10, **kw)
    _, tw = w.gather(tile, y0, x0, angle, displacement=disp)
    assert tw.shape == (3, 2, 8, 8) and torch.equal(tw[:, 1:], wt)
    assert torch.equal(tw, WeightsDistances([1.0, 2.0, 3.0], 5, 10, force_torch=True)(wt))


# --------------------------------------------------------------------------------------------------------- the refusals
def test_bad_inputs_raise_before_any_library_call(monkeypatch):
    from cnn_autoencoder_amd import _lib
    from cnn_autoencoder_amd.sampler import LabeledPatchSampler, PatchSampler, elastic_deform
    monkeypatch.setattr(_lib, 'lib', lambda: pytest.fail('the library was called'))
    x, d, t = torch.zeros(2, 3, 8, 8), torch.zeros(2, 2, 3, 3, dtype=torch.float64), torch.zeros(2, 1, 8, 8)
    for bad_x in (x[0], x.double(), torch.zeros(2, 3, 8, 9), torch.zeros(2, 5, 8, 8), x.numpy()):
        with pytest.raises(ValueError):
            elastic_deform(bad_x, d, force_torch=True)
    for bad_d in (d[0], d[:1], torch.zeros(2, 2, 3, 4, dtype=torch.float64), d.to(torch.float16), d.long()):
        with pytest.raises(ValueError, match='displacement'):
            elastic_deform(x, bad_d, force_torch=True)
    for bad_t in (t[0], t.long(), t[:1], torch.zeros(2, 1, 8, 9), torch.zeros(2, 5, 8, 8), t.numpy()):
        with pytest.raises(ValueError, match='masks'):
            elastic_deform(x, d, bad_t, force_torch=True)
    pool, labels = _pools()
    for sigma in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='elastic_sigma'):
            PatchSampler(pool, 8, elastic_deformation=True, elastic_sigma=sigma)
        with pytest.raises(ValueError, match='elastic_sigma'):
            LabeledPatchSampler(pool, labels, 8, elastic_sigma=sigma)
    # there is no CPU fallback
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(RuntimeError, match='no HIP device'):
        elastic_deform(x, d, t)
    with pytest.raises(RuntimeError, match='no HIP device'):
        PatchSampler(pool, 8, elastic_deformation=True).sample(2)


def test_bad_arguments_are_refused_on_the_host(built_lib):
    """CAE_ERR_ARG before anything touches a device (the pointers given here are never followed)"""
    from cnn_autoencoder_amd import _lib
    fn, query, err = _lib.lib().cae_t_elastic_deform, _lib.lib().cae_t_elastic_deform_workspace, _lib.lib().cae_last_error
    p, q, r, s = (ctypes.c_void_p(4096 * k) for k in (1, 2, 3, 4))

    def call(n=2, c=3, kt=1, ps=8, x_in=p, t_in=q, coef=p, x_out=r, t_out=s, ws=None, ws_bytes=0):
        return fn(x_in, t_in, coef, n, c, kt, ps, ws, ws_bytes, x_out, t_out, None)

    assert call(c=0) == -1 and call(c=5) == -1 and b'channels' in err()
    assert call(kt=-1) == -1 and call(kt=5) == -1 and b'mask channels' in err()
    assert call(ps=0) == -1 and call(ps=16385) == -1 and b'patch size' in err()
    assert call(n=-1) == -1 and b'n = -1' in err()
    for name in ('x_in', 'x_out', 'coef'):
        assert call(**{name: None}) == -1 and b'NULL' in err()
    assert call(t_in=None) == -1 and call(t_out=None) == -1 and b'NULL mask' in err()
    assert call(kt=0) == -1 and call(kt=0, t_in=None) == -1 and call(kt=0, t_out=None) == -1 and b'without mask' in err()
    assert call(kt=0, t_in=None, t_out=None, n=0) == 0
    assert call(x_out=p) == -1 and call(t_out=q) == -1 and call(t_out=p) == -1 and call(x_out=q) == -1 and b'also an input' in err()
    # patches above 128 need n c ps^2 floats of workspace; the message names the bytes
    need = 2 * 3 * 130 * 130 * 4
    assert query(2, 3, 130) == need and query(2, 3, 128) == 0 and query(0, 3, 130) == 0 and query(2, 5, 130) == 0
    assert call(ps=130) == -1 and str(need).encode() in err()
    assert call(ps=130, ws=p, ws_bytes=need - 1) == -1 and str(need).encode() in err()
    # more than 2^31 - 1 blocks: 2^29 planes of 16384^2 would take 2^29 x 8192 strips of rows
    assert call(n=1 << 29, c=1, ps=16384, ws=p, ws_bytes=1 << 62) == -1 and b'split the batch' in err()
    assert call(n=0) == 0 and call(n=0, ps=130) == 0
    with pytest.raises(ValueError):
        _lib.check(call(c=5))
