"""Host side of the border weight map (csrc/cae_seg_distances.hip, sampler.WeightsDistances): the oracle the GPU tests
judge the kernels by (tests/seg_weight_map_oracle.py) is itself checked here, against a brute-force search and against
the bound that the GPU tests apply; then the ABI's refusals and workspace queries, and the argument errors of the Python
surface.  No test here needs a GPU.
"""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import seg_weight_map_oracle as WO


# ------------------------------------------------------------------------------------------------------ the oracle
def test_the_oracles_distances_are_a_brute_force_search():
    """one distance transform per object and a sort, against the smallest squared distance over all pixel pairs"""
    from scipy import ndimage
    rng = np.random.default_rng(0)
    seen = set()
    for k in range(40):
        h, w = (int(v) for v in rng.integers(1, 13, 2))
        mask = rng.random((h, w)) < rng.choice([0.02, 0.1, 0.3, 0.6, 0.9])
        labels, count = ndimage.label(mask, structure=WO.EIGHT)
        got_count, got = WO.squared(mask)
        assert got_count == count
        assert np.array_equal(got, WO.brute(labels)), (h, w)
        seen.add(min(count, 2))
        # one object per distinct value, touching objects included
        values = (rng.integers(0, 4, (h, w)) * mask).astype(np.int32)
        assert np.array_equal(WO.squared(None, labels=values)[1], WO.brute(values)), (h, w)
    assert seen == {0, 1, 2}


def test_hand_made_distances():
    plane = np.zeros((3, 5), dtype=np.uint8)
    assert (WO.squared(plane)[1] == -1).all()
    plane[1, 0] = plane[1, 4] = 1  # two objects, the middle column at equal distance to both
    count, d2 = WO.squared(plane)
    assert count == 2
    assert d2[0, 1].tolist() == [0, 1, 4, 1, 0] and d2[1, 1].tolist() == [16, 9, 4, 9, 16]
    assert d2[0, 0].tolist() == [1, 2, 5, 2, 1] and d2[1, 0].tolist() == [17, 10, 5, 10, 17]
    plane[:] = 0
    plane[0, 1] = plane[1, 0] = 1  # two diagonal pixels: one object
    count, d2 = WO.squared(plane)
    assert count == 1 and (d2[1] == -1).all() and d2[0, 2].tolist() == [1, 2, 5, 8, 13]


@pytest.mark.parametrize('sigma', [1, 5, 20])
def test_the_bound_admits_the_reference_and_nothing_looser(sigma):
    """the reference's own float32 numpy evaluation on a 160 x 160 blob mask lies within the bound the GPU tests apply to
    the kernel, and uses a good part of it: the bound is no wider than a float32 evaluation needs"""
    target = WO.blobs(160, 160, 0.25, 7)
    o = WO.weight_map(target, [1.0, 2.0], sigma=sigma, w_0=1)
    assert o['count'] > 20
    ratio = np.abs(o['e32'].astype(np.float64) - o['e']) / WO.bound(o['arg'], o['e'])
    print(f'sigma {sigma}: {o["count"]} objects, worst error / bound {ratio.max():.3f}')
    assert ratio.max() <= 1.0
    assert ratio.max() >= 0.25
    # the class-weight part: exact
    assert np.array_equal(WO.weight_map(target, [1.0, 2.0], sigma=sigma, w_0=0)['w32'], np.where(target > 0, 2.0, 1.0).astype(np.float32))


def test_the_host_procedure_is_the_oracles():
    """sampler.WeightsDistances(force_torch=True) against the oracle's float32 evaluation, bit for bit: the same
    procedure written twice"""
    from cnn_autoencoder_amd.sampler import WeightsDistances
    planes = np.stack([WO.blobs(21, 30, 0.3, 1), np.zeros((21, 30), dtype=np.uint8), np.zeros((21, 30), dtype=np.uint8)])
    planes[2, 5:8, 5:9] = 1
    planes[0] *= np.random.default_rng(1).integers(1, 3, (21, 30)).astype(np.uint8)
    cw = [0.5, 1.0, 2.0]
    for dtype in (torch.float32, torch.int64):
        got = WeightsDistances(cw, sigma=3, w_0=7, force_torch=True)(torch.from_numpy(planes)[:, None].to(dtype))
        assert got.dtype == torch.float32 and got.shape == (3, 2, 21, 30)
        for i in range(3):
            assert np.array_equal(got[i, 0].numpy(), WO.weight_map(planes[i], cw, sigma=3, w_0=7)['w32'])
            assert np.array_equal(got[i, 1].numpy(), planes[i].astype(np.float32))


# ------------------------------------------------------------------------------------------------------ the ABI
NEW_SYMBOLS = ('cae_seg_object_distances', 'cae_seg_object_distances_workspace', 'cae_seg_weight_map')


def test_the_new_symbols_are_bound(built_lib):
    from cnn_autoencoder_amd import _lib
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is not None, name


def test_workspace_queries(built_lib):
    from cnn_autoencoder_amd import _lib
    L = _lib.lib()
    for n, h, w in ((0, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, 0), (1, -3, 4), (1, 32769, 4), (1, 4, 32769), (1, 1 << 30, 4)):
        assert L.cae_seg_object_distances_workspace(n, h, w) == 0, (n, h, w)
    for n, h, w in ((1, 1, 1), (3, 7, 9), (3, 264, 265), (4, 1024, 1024), (16, 256, 256), (1, 32768, 32768), (1, 32768, 3)):
        need = L.cae_seg_object_distances_workspace(n, h, w)
        assert need >= 8 * n * h * w and need % 8 == 0, (n, h, w)


def test_abi_refuses_without_a_device(built_lib):
    """bad arguments are refused before anything touches a device; n == 0 is nothing to do"""
    from cnn_autoencoder_amd import _lib
    L = _lib.lib()
    p = 1 << 20  # a pointer-like value that is aligned to everything; never dereferenced: every call here is refused
    big = 1 << 40
    dist = lambda labels=p, n=1, h=4, w=4, d2=p, ws=p, nbytes=big: L.cae_seg_object_distances(  # noqa: E731
        labels, n, h, w, d2, ws, nbytes, None)
    assert dist(n=0) == 0 and dist(n=0, labels=None, d2=None, ws=None, nbytes=0) == 0
    need = L.cae_seg_object_distances_workspace(1, 4, 4)
    for kw in (dict(n=-1), dict(h=0), dict(w=0), dict(h=-2), dict(h=32769), dict(w=32769), dict(h=1 << 30), dict(labels=None),
               dict(d2=None), dict(ws=None), dict(nbytes=0), dict(nbytes=need - 1), dict(labels=p + 2), dict(d2=p + 1),
               dict(ws=p + 4)):
        assert dist(**kw) == -1, kw
    assert dist(n=0, h=0) == -1 and dist(n=0, w=32769) == -1  # a bad shape is a bad shape with no planes too
    wmap = lambda target=p, d2=p, count=p, cw=p, ncw=2, sigma_2=50.0, n=1, hw=16, out=p, flag=p: L.cae_seg_weight_map(  # noqa: E731
        target, d2, count, cw, ncw, sigma_2, 10.0, n, hw, out, flag, None)
    assert wmap(n=0) == 0 and wmap(n=0, target=None, d2=None, count=None, cw=None, out=None, flag=None) == 0
    for kw in (dict(n=-1), dict(hw=0), dict(ncw=0), dict(ncw=-1), dict(sigma_2=0.0), dict(sigma_2=-1.0), dict(sigma_2=math.inf),
               dict(sigma_2=math.nan), dict(target=None), dict(d2=None), dict(count=None), dict(cw=None), dict(out=None),
               dict(flag=None)):
        assert wmap(**kw) == -1, kw
    assert wmap(n=0, sigma_2=0.0) == -1


def test_the_new_kernels_use_no_scratch(built_lib):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import scratch_check
    mine = re.compile(r'\d+wd_(column|row|map)_kernel')  # (the digits: the mangled length, so no fwd_ / bwd_ kernel)
    table = {k: v for k, v in scratch_check.kernel_table(built_lib).items() if mine.search(k)}
    assert len(table) == 4, sorted(table)  # the column pass, the row pass at two block sizes, the map
    assert all(v == (0, 0) for v in table.values()), table


# -------------------------------------------------------------------------------------------------- Python surface
def test_object_distances_refuses_bad_arguments(monkeypatch):
    from cnn_autoencoder_amd import segmenters as S
    i32 = torch.zeros((2, 4, 6), dtype=torch.int32)
    for bad in (i32.long(), i32[0], i32.numpy()):
        with pytest.raises(ValueError, match='int32'):
            S.object_distances(bad)
    with pytest.raises(ValueError, match='too large'):
        S.object_distances(torch.zeros((1, 32769, 2), dtype=torch.int32, device='meta'))
    with pytest.raises(ValueError, match='empty'):
        S.object_distances(torch.zeros((1, 0, 2), dtype=torch.int32))
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)  # (so on a machine that has one, too)
    with pytest.raises(RuntimeError, match='no HIP device'):
        S.object_distances(i32)


def test_weights_distances_argument_errors(monkeypatch):
    from cnn_autoencoder_amd.sampler import WeightsDistances
    wd = WeightsDistances([1.0, 2.0])
    assert wd.sigma_2 == 50 and wd.w_0 == 10  # the reference's constructor and attributes
    with pytest.raises(ValueError, match='one target channel'):
        wd(torch.zeros((2, 3, 4, 4)))
    for bad in (torch.zeros((2, 4, 4)), torch.zeros((2, 1, 4, 4), dtype=torch.uint8), np.zeros((2, 1, 4, 4), dtype=np.float32)):
        with pytest.raises(ValueError, match='label planes'):
            wd(bad)
    with pytest.raises(ValueError, match='class_weights'):
        WeightsDistances([])
    for sigma in (0, math.inf, math.nan):
        with pytest.raises(ValueError, match='sigma'):
            WeightsDistances([1.0], sigma=sigma)
    # the host procedure raises as numpy.take does
    with pytest.raises(IndexError):
        WeightsDistances([1.0, 2.0], force_torch=True)(torch.full((1, 1, 4, 4), 2.0))
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(RuntimeError, match='no HIP device'):
        wd(torch.zeros((2, 1, 4, 4)))


def _pools(k):
    rng = np.random.default_rng(k)
    return rng.integers(0, 256, (2, 20, 24, 3), dtype=np.uint8), rng.integers(0, 2, (2, 20, 24, k), dtype=np.uint8)


def test_the_sampler_checks_its_weight_map_keywords():
    from cnn_autoencoder_amd.sampler import LabeledPatchSampler
    pool, labels = _pools(3)
    three = dict(class_weights=[1.0, 2.0, 3.0, 4.0], weights_map_sigma=5, weights_map_w=10)
    with pytest.raises(ValueError, match='one target channel'):
        LabeledPatchSampler(pool, labels, 8, **three)
    for missing in three:
        with pytest.raises(ValueError, match='together'):
            LabeledPatchSampler(pool, labels, 8, map_labels=True, **{k: v for k, v in three.items() if k != missing})
    s = LabeledPatchSampler(pool, labels, 8, map_labels=True, **three)
    assert s.weights is not None and s.weights.sigma_2 == 50 and s.weights.w_0 == 10
    # the largest label value of the pool must index the table: with map_labels the largest channel sum
    assert int(labels.sum(-1).max()) == 3
    with pytest.raises(IndexError, match='largest label value 3'):
        LabeledPatchSampler(pool, labels, 8, map_labels=True, **dict(three, class_weights=[1.0, 2.0, 3.0]))
    with pytest.raises(IndexError, match='largest label value 1'):
        LabeledPatchSampler(pool, labels[..., :1], 8, **dict(three, class_weights=[1.0]))
    assert LabeledPatchSampler(pool, labels[..., :1], 8, **dict(three, class_weights=[1.0, 2.0])).weights is not None


@pytest.mark.parametrize('dtype', [torch.float32, torch.int64])
def test_the_samplers_batches_on_the_host_path(dtype):
    """force_torch on the host: without the keywords t has its old shape and type; with them it is fp32 [n, 2, ps, ps],
    the host weight map of the same labels and then the labels"""
    from cnn_autoencoder_amd.sampler import LabeledPatchSampler, WeightsDistances
    pool, labels = _pools(1)
    kw = dict(rotation=True, target_data_type=dtype, batch_size=3, steps_per_epoch=1, force_torch=True)
    three = dict(class_weights=[1.0, 2.0], weights_map_sigma=2, weights_map_w=4)
    torch.manual_seed(5)
    (x0, t0), = list(LabeledPatchSampler(pool, labels, 8, **kw))
    assert t0.dtype == dtype and t0.shape == ((3, 8, 8) if dtype == torch.int64 else (3, 1, 8, 8))
    torch.manual_seed(5)
    (x1, t1), = list(LabeledPatchSampler(pool, labels, 8, **kw, **three))
    assert torch.equal(x0, x1)
    assert t1.dtype == torch.float32 and t1.shape == (3, 2, 8, 8)
    assert torch.equal(t1[:, 1], t0.reshape(3, 8, 8).to(torch.float32))
    assert torch.equal(t1, WeightsDistances([1.0, 2.0], 2, 4, force_torch=True)(t1[:, 1:]))
    assert float(t1[:, 0].min()) >= 1.0 and float(t1[:, 0].max()) <= 6.0
