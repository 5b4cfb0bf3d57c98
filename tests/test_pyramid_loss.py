"""The multiscale objective on the host: criteria.pyramid_down (CPU form) and GeneralLoss('MultiscaleMSE') against the
reference's values (tests/golden/ref_loss_pyramid.npz, written by tools/gen_golden_pyramid.py from the reference's
setup_loss('RateMultiscaleMSE'), _ratedist.py:10-43, 88-93, _lossutils.py:5-151)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLD


def _fixture():
    g = np.load(os.path.join(GOLD, 'ref_loss_pyramid.npz'))
    return g, json.loads(bytes(g['cases_json']).decode())


class _Fe:
    def __init__(self):
        self.aux = torch.tensor(3.5)

    def loss(self):
        return self.aux


def rel(got, want) -> float:
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / max(float(np.abs(want).max()), 1e-30))


def test_cpu_pyramid_matches_the_reference_targets():
    from cnn_autoencoder_amd import criteria
    g, cases = _fixture()
    for ci, case in enumerate(cases):
        t = torch.from_numpy(g[f'c{ci}_x'])
        for s in range(1, case['compression_level']):
            t = criteria.pyramid_down(t)
            want = g[f'c{ci}_target{s}']
            assert t.shape == want.shape, (ci, s)
            assert rel(t.numpy(), want) < 1e-6, (ci, s)


@pytest.mark.parametrize('tag', ['scalar', 'list'])
def test_multiscale_loss_matches_the_reference(tag):
    """dist lists every level x 255^2; dist_loss = sum over zip(dist, lambda): a scalar lambda weights level 0 only."""
    from cnn_autoencoder_amd import criteria
    g, cases = _fixture()
    for ci, case in enumerate(cases):
        L, c = case['compression_level'], case['channels_org']
        crit = criteria.setup_loss('RateMultiscaleMSE', channels_org=c, compression_level=L,
                                   distortion_lambda=case['lambdas'][tag])
        x_r = [torch.from_numpy(g[f'c{ci}_x_r{s}']) for s in range(L)]
        ld = crit(inputs=torch.from_numpy(g[f'c{ci}_x']), outputs=dict(x_r=x_r, p_y=torch.from_numpy(g[f'c{ci}_p_y'])),
                  net={'fact_ent': _Fe()})
        assert len(ld['dist']) == L
        assert rel([float(d) for d in ld['dist']], g[f'c{ci}_dist_{tag}']) < 1e-6, ci
        assert rel(float(ld['dist_loss']), g[f'c{ci}_dist_loss_{tag}']) < 1e-6, ci
        assert rel(float(ld['loss']), g[f'c{ci}_loss_{tag}']) < 1e-6, ci
        if tag == 'scalar':  # (zip truncation: only level 0 enters dist_loss)
            assert float(ld['dist_loss']) == pytest.approx(float(ld['dist'][0]) * case['lambdas'][tag], rel=1e-6)


def test_multiscale_loss_rejects_a_model_without_colour_layers():
    from cnn_autoencoder_amd import criteria
    crit = criteria.setup_loss('RateMultiscaleMSE', channels_org=3, compression_level=3)
    x = torch.rand(1, 3, 16, 16)
    with pytest.raises(ValueError, match='multiscale_analysis'):
        crit(inputs=x, outputs=dict(x_r=[x, None, None], p_y=torch.rand(1, 4, 2, 2)), net={'fact_ent': _Fe()})


@pytest.mark.parametrize('name', ['RateMultiscaleMSSSIM', 'RateMSSSIM'])
def test_msssim_criteria_still_raise(name):
    from cnn_autoencoder_amd import criteria
    with pytest.raises(NotImplementedError):
        criteria.setup_loss(name, channels_org=3, compression_level=3)
