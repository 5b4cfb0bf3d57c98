"""Host side of the segmentation head (cnn_autoencoder_amd/segmenters.py): the restatement against the reference's
golden stages, the module surface (state dict keys, kwargs, errors), the library's stage plan against the module's (stages,
weight order, workspace sizes, refused configs), the weight packers with hand-worked answers, the judge of the GPU tests'
bounds, and the packers under AddressSanitizer + UBSan."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import inference_replay as R
import segmenter_restatement as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _seg():
    from cnn_autoencoder_amd import segmenters
    return segmenters


# ----------------------------------------------------------------------------------------------- restatement / goldens
@pytest.mark.parametrize('name', sorted(SR.GOLDEN_CONFIGS))
def test_float32_restatement_reproduces_the_reference_stages(name):
    """logits and every hooked stage of the reference's JNet, to 1e-6 of the stage's largest magnitude"""
    cfg, sd, y_q, brg, logits, stages = SR.load_golden(name)
    out, mine = SR.jnet(sd, cfg, y_q, brg, torch.float32)
    assert set(mine) == set(stages)
    assert out.shape == logits.shape
    for key, want in dict(stages, logits=logits).items():
        got = out if key == 'logits' else mine[key]
        assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max()), key


@pytest.mark.parametrize('name', sorted(SR.GOLDEN_CONFIGS))
def test_reference_logits_meet_the_end_to_end_requirement(name):
    """the bar the kernels are held to (tests/test_segmenter.py) holds for the reference's own float32 result"""
    cfg, sd, y_q, brg, logits, _ = SR.load_golden(name)
    f64, _ = SR.jnet(sd, cfg, y_q, brg, torch.float64)
    f32, _ = SR.jnet(sd, cfg, y_q, brg, torch.float32)
    assert float((logits.double() - f64).abs().max()) <= SR.e2e_bound(f32, f64)


@pytest.mark.parametrize('name', sorted(SR.GOLDEN_CONFIGS))
def test_state_dict_keys_shapes_and_strict_load(name):
    S = _seg()
    cfg, sd, *_ = SR.load_golden(name)
    m = S.JNet(**cfg)
    own = m.state_dict()
    assert list(own) == list(sd)  # the reference's keys in the reference's order
    assert all(own[k].shape == sd[k].shape for k in sd)
    m.load_state_dict(sd, strict=True)
    m2 = S.segmenter_from_state_dict(dict(cfg, segment_model_type='JNet', seg_model=sd, save_bridges=True, channels_prg=3))
    assert isinstance(m2, S.JNet) and not m2.training
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in m2.state_dict().items())
    assert 'bottleneck._c1.weight' in own and ('synthesis_track.0._up_sample.bias' in own)
    if cfg['concat_bridges'] and cfg['batch_norm']:
        assert 'bridges_projection.1._bn2.weight' in own


def test_defaults_and_swallowed_kwargs():
    S = _seg()
    m = S.JNet(save_bridges=False, channels_prg=3, project_bridges_from_channels=192, anything_else=1)
    sd = m.state_dict()
    # the reference's defaults: channels_bn=320, 64 / 2 / 1024, four levels, no bridges, one class
    assert sd['bottleneck._c1.weight'].shape == (1024, 320, 1, 1)
    assert sd['bottleneck._up_sample.weight'].shape == (1024, 512, 2, 2)
    assert [sd[f'synthesis_track.{i}._c1.weight'].shape[:2] for i in range(4)] == [(512, 512), (256, 256), (128, 128), (64, 64)]
    assert sd['fc.weight'].shape == (1, 64, 1, 1) and not any(k.startswith('bridges_projection') for k in sd)
    assert 'synthesis_track.3._up_sample.weight' not in sd
    assert S.SEG_MODELS == {'UNet': S.UNet, 'JNet': S.JNet}
    assert isinstance(S.setup_modules('JNet', channels_bn=8, seg_channels_bn=8, seg_channels_net=4, compression_level=1), S.JNet)


def test_value_errors_and_not_implemented():
    S = _seg()
    from cnn_autoencoder_amd import criteria
    cfg = SR.GOLDEN_CONFIGS['a'][0]
    m = S.JNet(**cfg).eval()
    y = torch.zeros(2, 48, 3, 5)
    brg = [torch.zeros(2, 40, 6, 10), torch.zeros(2, 40, 12, 20), torch.zeros(2, 3, 24, 40)]
    with torch.no_grad():
        for bad_y in (torch.zeros(48, 3, 5), torch.zeros(2, 47, 3, 5)):
            with pytest.raises(ValueError):
                m(bad_y, brg)
        for bad in (None, brg[:2], [brg[0], brg[1], torch.zeros(2, 4, 24, 40)], [brg[0], torch.zeros(2, 40, 12, 21), brg[2]],
                    [brg[0], brg[1], torch.zeros(1, 3, 24, 40)], [brg[0][0], brg[1], brg[2]]):
            with pytest.raises(ValueError):
                m(y, bad)
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError, match='no HIP device'):  # no CPU fallback
                m(y, brg)
    with pytest.raises(NotImplementedError, match='no_grad'):  # autograd is recording
        m(y, brg)
    with pytest.raises(NotImplementedError, match='training'):
        with torch.no_grad():
            S.JNet(**cfg).train()(y, brg)
    with pytest.raises(NotImplementedError, match='analysis track'):
        S.UNet(channels_org=3)
    with pytest.raises(NotImplementedError, match='analysis track'):
        S.setup_modules('UNet')
    with pytest.raises(NotImplementedError, match='train'):
        S.segmenter_from_state_dict(dict(cfg, segment_model_type='JNet'), train=True)
    with pytest.raises(ValueError):
        S.segmenter_from_state_dict(dict(cfg, segment_model_type='VNet'))
    with pytest.raises(NotImplementedError):
        m.bottleneck(y)
    # forward_func: 'seg_model' is accepted; with autograd recording it raises, other names still do at set-up
    fwd = criteria.setup_forward_func(('seg_model',))
    with pytest.raises(NotImplementedError, match='seg_model'):
        fwd(y, dict(seg_model=m))
    with pytest.raises(NotImplementedError):
        criteria.setup_forward_func(('class_model',))
    out = criteria.setup_forward_func(())(y, {})
    assert out['s_pred'] is None and out['s_aux_pred'] is None


# ----------------------------------------------------------------------------------------------- the stage plan
class _StageInfo(ctypes.Structure):  # cae_seg_stage_info
    _fields_ = [(k, ctypes.c_int) for k in ('ks', 'cin_a', 'cin_b', 'cout', 'up', 'biased', 'norm', 'bridge', 'src_a_stage',
                                            'src_b_stage', 'src_a_transformed', 'n_weights')]


CAE_ERR_ARG = -1
_SMALL = dict(channels_bn=12, channels_net=10, seg_channels_net=3, seg_channels_bn=20, num_classes=2)
PLAN_CONFIGS = dict({name: c[0] for name, c in SR.GOLDEN_CONFIGS.items()}, defaults={},
                    **{f'L{L}-concat{int(cat)}-bn{int(bn)}': dict(_SMALL, compression_level=L, concat_bridges=cat, batch_norm=bn)
                       for L in (1, 8) for cat in (False, True) for bn in (False, True)})
_PLANNED = {}


def _planned(name):
    """-> (the JNet of PLAN_CONFIGS[name], its cae_seg_config, the library's stage records), built once"""
    if name not in _PLANNED:
        from cnn_autoencoder_amd import _lib
        m = _seg().JNet(**PLAN_CONFIGS[name])
        cfg = m._config()
        L = _lib.lib()
        n = L.cae_seg_plan(ctypes.byref(cfg), None, 0)
        assert n > 0
        out = (_StageInfo * n)()
        assert L.cae_seg_plan(ctypes.byref(cfg), out, n) == n
        short = (_StageInfo * 2)()  # a smaller capacity: the count all the same, the first records only
        assert L.cae_seg_plan(ctypes.byref(cfg), short, 2) == n and bytes(short) == bytes(out)[:ctypes.sizeof(short)]
        _PLANNED[name] = (m, cfg, list(out))
    return _PLANNED[name]


def _weight_shape(r):
    return (r.cin_a, r.cout, 2, 2) if r.up else (r.cout, r.cin_a + r.cin_b, r.ks, r.ks)


@pytest.mark.parametrize('name', sorted(PLAN_CONFIGS))
def test_library_plan_is_the_modules_stage_plan(name):
    """cae_seg_plan (csrc/cae_seg.hip, no device) against JNet.stage_plan(), stage by stage"""
    m, cfg, recs = _planned(name)
    plan = m.stage_plan()
    assert len(recs) == len(plan)
    for s, (r, st) in enumerate(zip(recs, plan)):
        what = (name, s, st['name'])
        assert r.ks == st['ks'] and bool(r.up) == st['up'] and (r.cin_b == 0 or not r.up), what
        assert _weight_shape(r) == tuple(st['weight'].shape), what
        assert bool(r.biased) == (st['bias'] is not None), what
        assert bool(r.norm) == st['has_ab'] and (bool(r.norm) and bool(cfg.batch_norm)) == (st['norm'] is not None), what
        srcs = []
        if r.src_a_stage != -2:
            srcs.append(('bridge', r.bridge) if r.bridge >= 0 else ('latent',) if r.src_a_stage == -1 else
                        ('raw', r.src_a_stage, bool(r.src_a_transformed)))
        if r.src_b_stage != -2:
            srcs.append(('raw', r.src_b_stage, False))
        assert srcs == [tuple(sr) for sr in st['srcs']], what
        assert (r.src_a_stage == -2) == (r.cin_a == 0) and (r.src_b_stage == -2) == (r.cin_b == 0), what
        assert r.bridge == (st['srcs'][0][1] if st['srcs'][0][0] == 'bridge' else -1), what
        assert r.bridge < 0 or (r.src_a_stage == -1 and r.src_a_transformed == 1), what
        for stage, cin in ((r.src_a_stage, r.cin_a), (r.src_b_stage, r.cin_b)):
            assert not 0 <= stage < s or recs[stage].cout == cin, what  # a source has its producer's channels
            assert stage < s, what


@pytest.mark.parametrize('name', sorted(PLAN_CONFIGS))
def test_weight_order_follows_the_plan(name):
    """each stage owns n_weights consecutive entries of _weight_list(): [bn1 gamma beta] weight [bias] [gamma beta]"""
    from cnn_autoencoder_amd import _lib
    m, cfg, recs = _planned(name)
    weights, plan, bn, pos = m._weight_list(), m.stage_plan(), bool(cfg.batch_norm), 0
    for r, st in zip(recs, plan):
        mine = weights[pos:pos + r.n_weights]
        pos += r.n_weights
        want = [(r.cin_a,)] * 2 if (r.bridge >= 0 and bn) else []
        want += [_weight_shape(r)] + [(r.cout,)] * int(r.biased) + [(r.cout,)] * (2 if (r.norm and bn) else 0)
        assert [tuple(w.shape) for w in mine] == want, (name, st['name'])
        assert mine[2 if (r.bridge >= 0 and bn) else 0] is st['weight'], (name, st['name'])
        if r.bridge >= 0 and bn:
            bn1 = m.bridges_projection[r.bridge]._bn1
            assert mine[0] is bn1.weight and mine[1] is bn1.bias
        if r.biased:
            assert mine[-1] is st['bias']
        if r.norm and bn:
            assert mine[-2] is st['norm'].weight and mine[-1] is st['norm'].bias
    assert pos == len(weights) == _lib.lib().cae_seg_weight_count(ctypes.byref(cfg))


def _workspace_before_the_plan(c, n, lh, lw, tx, ty):
    """cae_seg_forward's own pass over the levels as it stood before it read the plan: bytes of X0 T1 T2 U BC RP AB STATS"""
    X0, T1, T2, U, BC, RP, AB, STATS = range(8)
    c8 = lambda ch, hw: n * ((ch + 7) // 8) * hw * 32
    tiles_of = lambda hh, ww: ((hh + ty - 1) // ty) * ((ww + tx - 1) // tx)
    need, cpmax, hw0 = [0] * 8, (c.seg_channels_bn + 7) // 8 * 8, lh * lw
    need[X0] = c8(c.channels_bn, hw0)
    need[T1] = need[T2] = c8(c.seg_channels_bn, hw0)
    need[STATS] = tiles_of(lh, lw) * n * cpmax * 12
    for i in range(c.levels):
        hw, ch = hw0 << (2 * (i + 1)), c.level_channels[i]
        for b in (U, T1, T2):
            need[b] = max(need[b], c8(ch, hw))
        cpl = (ch + 7) // 8 * 8
        if c.concat_bridges:
            need[BC] = max(need[BC], c8(c.bridge_channels[i], hw))
            need[RP] = max(need[RP], c8(ch, hw))
            cpmax = max(cpmax, (c.bridge_channels[i] + 7) // 8 * 8)
        cpmax = max(cpmax, cpl)
        need[STATS] = max(need[STATS], tiles_of(lh << (i + 1), lw << (i + 1)) * n * cpl * 12)
    need[AB] = 4 * (n * cpmax * 2) * 4
    return need


@pytest.mark.parametrize('name', sorted(PLAN_CONFIGS))
def test_workspace_sizes_are_those_before_the_plan(name):
    """(1, 9, 17) straddles the 8 x 16 output tile"""
    from cnn_autoencoder_amd import _lib
    _, cfg, _ = _planned(name)
    L = _lib.lib()
    tx, ty = ctypes.c_int(), ctypes.c_int()
    L.cae_seg_tile(ctypes.byref(tx), ctypes.byref(ty))
    for n, lh, lw in ((1, 1, 1), (2, 3, 5), (1, 9, 17)):
        out = (ctypes.c_size_t * 8)()
        _lib.check(L.cae_seg_workspace_bytes(ctypes.byref(cfg), n, lh, lw, out))
        assert list(out) == _workspace_before_the_plan(cfg, n, lh, lw, tx.value, ty.value), (name, n, lh, lw)
    assert L.cae_seg_workspace_bytes(ctypes.byref(cfg), 0, 1, 1, out) == CAE_ERR_ARG


def test_refused_configs():
    """levels 0 or 9, a zero channel count, a level that hands the next one other channels than it takes"""
    from cnn_autoencoder_amd import _lib
    L = _lib.lib()

    def refused(**change):
        cfg = _seg().JNet(**SR.GOLDEN_CONFIGS['a'][0])._config()
        for k, v in change.items():
            if isinstance(v, tuple):
                getattr(cfg, k)[v[0]] = v[1]
            else:
                setattr(cfg, k, v)
        n = 64
        host = [np.zeros(1 << 16, np.float32)] * n
        ptrs, handle = (ctypes.c_void_p * n)(*[w.ctypes.data for w in host]), ctypes.c_void_p()
        got = (L.cae_seg_plan(ctypes.byref(cfg), None, 0), L.cae_seg_weight_count(ctypes.byref(cfg)),
               L.cae_seg_create(ctypes.byref(cfg), ptrs, n, ctypes.byref(handle)))
        assert not handle
        return got

    assert refused()[:2] == (15, 47)  # (the unchanged config is accepted: 3 + 3 * 4 - 1 + 1 stages, 47 arrays)
    for change in (dict(levels=0), dict(levels=9), dict(channels_bn=0), dict(seg_channels_bn=0), dict(num_classes=0),
                   dict(level_channels=(1, 0)), dict(bridge_channels=(2, 0)), dict(up_channels=(0, 17))):
        assert refused(**change) == (CAE_ERR_ARG,) * 3, change
    with pytest.raises(ValueError):
        _lib.check(L.cae_seg_plan(None, None, 0))


# ----------------------------------------------------------------------------------------------- packers
def _pack(w, cin_a, cin_b, cout, ks, up):
    """-> (hi, lo) float64 arrays indexed [group, chunk, ky, kx, ct, lane, j] and the raw halves"""
    from cnn_autoencoder_amd import _lib
    L = _lib.lib()
    n = L.cae_seg_packed_halves(cin_a, cin_b, cout, ks, int(up))
    assert n > 0
    w = np.ascontiguousarray(w, dtype=np.float32)
    out = np.zeros(n, dtype=np.float16)
    _lib.check(L.cae_seg_pack(w.ctypes.data, cin_a, cin_b, cout, ks, int(up), out.ctypes.data, n))
    m = 4 * ((cout + 7) // 8 * 8) if up else cout
    ct = 1 if m <= 32 else 2 if (m <= 64 or ks == 3) else 4
    groups = (m + 32 * ct - 1) // (32 * ct)
    rec = out.reshape(groups, -1, ks, ks, ct, 2, 64, 8)
    return rec[..., 0, :, :], rec[..., 1, :, :]


def _unpacked(hi, lo):
    """matrix [row, k, ky, kx] of hi + lo from the fragment order: row = 32 (g CT + ct) + (lane & 31),
    k = 16 q + 8 (lane >> 5) + j"""
    v = hi.astype(np.float64) + lo.astype(np.float64)
    G, Q, ks, _, ct, _, _ = v.shape
    out = np.zeros((G * ct * 32, Q * 16, ks, ks))
    for g in range(G):
        for q in range(Q):
            for t in range(ct):
                for lane in range(64):
                    for j in range(8):
                        out[32 * (g * ct + t) + (lane & 31), 16 * q + 8 * (lane >> 5) + j] = v[g, q, :, :, t, lane, j]
    return out


def test_pack_transposed_weight_as_four_pointwise_matrices():
    cin, cout = 3, 2
    w = np.zeros((cin, cout, 2, 2), np.float32)
    for ci in range(cin):
        for co in range(cout):
            for dy in range(2):
                for dx in range(2):
                    w[ci, co, dy, dx] = 1000 * (ci + 1) + 100 * co + 10 * dy + dx
    mat = _unpacked(*_pack(w, cin, 0, cout, 1, True))[:, :, 0, 0]
    want = np.zeros_like(mat)  # rows (2 dy + dx) * 8 + co: one 8-channel plane per output parity
    for par in range(4):
        for co in range(cout):
            want[8 * par + co, :cin] = w[:, co, par >> 1, par & 1]
    assert mat.shape == (32, 16) and np.array_equal(mat, want)
    assert want[8 * 1 + 1, 2] == 3101 and want[8 * 2 + 0, 0] == 1010  # (dy, dx) = (0, 1) and (1, 0) by hand


def test_pack_zero_rows_at_a_concat_boundary_of_20_and_20_channels():
    rng = np.random.default_rng(0)
    cout, ks = 4, 3
    w = rng.integers(1, 9, size=(cout, 40, ks, ks)).astype(np.float32)  # no zero entries
    mat = _unpacked(*_pack(w, 20, 20, cout, ks, False))
    assert mat.shape == (32, 48, 3, 3)  # three planes per source, three 16-channel chunks
    assert np.array_equal(mat[:cout, :20], w[:, :20])      # source A
    assert not mat[:, 20:24].any()                         # A's padding channels: zero rows
    assert np.array_equal(mat[:cout, 24:44], w[:, 20:])    # source B starts on the next plane
    assert not mat[:, 44:].any() and not mat[cout:].any()
    # a boundary off the 16-channel chunk grid as well: 5 | 5 -> planes of 8, one chunk
    w2 = rng.integers(1, 9, size=(cout, 10, ks, ks)).astype(np.float32)
    m2 = _unpacked(*_pack(w2, 5, 5, cout, ks, False))
    assert m2.shape[1] == 16 and np.array_equal(m2[:cout, :5], w2[:, :5]) and np.array_equal(m2[:cout, 8:13], w2[:, 5:])
    assert not m2[:, 5:8].any() and not m2[:, 13:].any()
    # no source A (concat_bridges off)
    m3 = _unpacked(*_pack(w2, 0, 10, cout, ks, False))
    assert np.array_equal(m3[:cout, :10], w2) and not m3[:, 10:].any()


def test_pack_split_rule_is_pack_splits():
    """hi = f16(v), lo = f16(v - hi), round to nearest even, bit for bit; many output-channel groups"""
    rng = np.random.default_rng(1)
    cout, cin, ks = 150, 9, 3
    w = (rng.standard_normal((cout, cin, ks, ks)) * np.array([1.0, 1e-3, 30.0])[None, None, :, None]).astype(np.float32)
    hi, lo = _pack(w, cin, 0, cout, ks, False)
    assert hi.shape[0] == 3 and hi.shape[4] == 2  # 150 rows: three groups of two channel tiles
    G, Q, _, _, ct, _, _ = hi.shape
    for g, t, lane, j, q in [(0, 0, 0, 0, 0), (1, 1, 37, 0, 0), (2, 0, 21, 7, 0), (2, 0, 63, 0, 0), (0, 1, 5, 3, 0)]:
        row, k = 32 * (g * ct + t) + (lane & 31), 16 * q + 8 * (lane >> 5) + j
        v = w[row, k] if row < cout and k < cin else np.zeros((ks, ks), np.float32)
        h = v.astype(np.float16)
        l = (v - h.astype(np.float32)).astype(np.float16)
        assert np.array_equal(hi[g, q, :, :, t, lane, j].view(np.uint16), h.view(np.uint16))
        assert np.array_equal(lo[g, q, :, :, t, lane, j].view(np.uint16), l.view(np.uint16))
    mat = _unpacked(hi, lo)
    assert float(np.abs(mat[:cout, :cin] - w).max()) <= 2.0 ** -22 * float(np.abs(w).max())


def test_pack_argument_checks():
    from cnn_autoencoder_amd import _lib
    L = _lib.lib()
    assert L.cae_seg_packed_halves(0, 0, 4, 3, 0) == 0 and L.cae_seg_packed_halves(4, 0, 0, 3, 0) == 0
    assert L.cae_seg_packed_halves(4, 0, 4, 2, 0) == 0 and L.cae_seg_packed_halves(4, 4, 4, 1, 1) == 0
    w = np.zeros(16, np.float32)
    out = np.zeros(8, np.float16)
    with pytest.raises(ValueError):
        _lib.check(L.cae_seg_pack(w.ctypes.data, 4, 0, 4, 1, 0, out.ctypes.data, 8))  # too small an output
    with pytest.raises(ValueError):
        _lib.check(L.cae_seg_pack(None, 4, 0, 4, 1, 0, out.ctypes.data, 8))
    tx, ty = ctypes.c_int(), ctypes.c_int()
    L.cae_seg_tile(ctypes.byref(tx), ctypes.byref(ty))
    assert tx.value > 0 and ty.value > 0


# ----------------------------------------------------------------------------------------------- judge
STAT_DEFECTS = ['naive_variance', 'unbiased', 'no_eps', 'padding_pixels', 'shared_samples']
CONV_DEFECTS = ['relu_on_untransformed', 'b_from_a', 'parity_swapped', 'bias_per_tap']


def _emulated_ab(x, gamma, beta, defect):
    n, c = x.shape[:2]
    a, b = np.zeros((n, c), np.float32), np.zeros((n, c), np.float32)
    for i in range(n):
        for ch in range(c):
            src = x[0 if defect == 'shared_samples' else i, ch].numpy()
            a[i, ch], b[i, ch] = SR.emu_ab(src, np.float32(gamma[ch]), np.float32(beta[ch]),
                                           defect=defect if defect != 'shared_samples' else None)
    return torch.from_numpy(a), torch.from_numpy(b)


def test_segmenter_judge_rejects_wrong_kernels():
    """The bounds of tests/test_segmenter.py pass a faithful numpy emulation of the kernels' arithmetic and fail each
    planted defect.  Statistics: `C_STAT 2^-24 (|a| (|x| + |m|) + |b|)` on the effect of (a, b), on an ordinary plane and on
    the mean-100, sigma-0.01 plane (13 x 21: ragged tiles, two tile rows); convolutions: inference_replay.conv_step with
    C_CONV as it stands (20 | 20 channels from two sources, 2x2 transposed convolution with bias)."""
    C_STAT = SR.C_STAT
    g = torch.Generator().manual_seed(0)
    n, c, h, w = 2, 3, 13, 21
    planes = {'ordinary': torch.randn(n, c, h, w, generator=g) * torch.tensor([1.0, 2.0]).view(2, 1, 1, 1) + 0.3,
              'mean100': 100.0 + 0.01 * torch.randn(n, c, h, w, generator=g) + torch.tensor([0.0, 0.05]).view(2, 1, 1, 1),
              'small_sigma': 0.5 + 1e-3 * torch.randn(n, c, h, w, generator=g),  # variance far below eps
              'one_pixel': torch.randn(n, c, 1, 1, generator=g)}
    gamma, beta = torch.tensor([1.0, 0.7, 1.4]), torch.tensor([0.1, -0.2, 0.3])
    for name, x in planes.items():
        a, b = _emulated_ab(x, gamma, beta, None)
        r = SR.stat_ratio(a, b, x, gamma, beta)
        if os.environ.get('CAE_TEST_VERBOSE'):
            print(f'faithful statistics, {name}: ratio {r:.3f}')
        assert r <= C_STAT, (name, r)
    a1, b1 = _emulated_ab(planes['one_pixel'], gamma, beta, None)  # mean == x exactly, var == 0: rstd = 1 / sqrt(eps)
    rstd = np.float32(1.0) / np.sqrt(np.float32(SR.EPS))
    assert np.array_equal(a1.numpy(), np.broadcast_to(gamma.numpy() * rstd, (n, c)))
    assert np.array_equal(b1.numpy(), beta.numpy() - planes['one_pixel'][:, :, 0, 0].numpy() * a1.numpy())
    for defect in STAT_DEFECTS:
        # (the variance formula is judged where it matters: on the mean-100 plane; the others on the ordinary one too)
        worst = max(SR.stat_ratio(*_emulated_ab(planes[p], gamma, beta, defect), planes[p], gamma, beta)
                    for p in (['mean100'] if defect == 'naive_variance' else ['ordinary', 'mean100', 'small_sigma']))
        if os.environ.get('CAE_TEST_VERBOSE'):
            print(f'{defect}: ratio {worst:.1f}')
        assert worst > C_STAT, (defect, worst)

    # convolutions, judged from the staged operand as the GPU tests do
    ca = cb = 20
    xa = torch.randn(1, ca, h, w, generator=g)
    aa, ba = 0.5 + torch.rand(1, ca, generator=g), torch.randn(1, ca, generator=g) * 0.2
    xb = torch.randn(1, cb, h, w, generator=g)  # untransformed source: negative values stay
    wt = torch.randn(8, ca + cb, 3, 3, generator=g) / math.sqrt(9 * (ca + cb))
    va = SR.staged(xa, aa, ba)
    op = lambda x, k: torch.nn.functional.conv2d(x, k, padding=k.shape[-1] // 2)
    ref, B = R.conv_step(op, torch.cat([va, xb], 1), wt, None, f16=True)

    def conv(defect):
        vb = torch.relu(xb) if defect == 'relu_on_untransformed' else xb
        return torch.from_numpy(SR.emu_conv([va.numpy(), vb.numpy()], wt.numpy(), None, defect))

    wu = torch.randn(ca, 6, 2, 2, generator=g) / math.sqrt(ca)
    bu = torch.rand(6, generator=g) - 0.5
    opu = lambda x, k: torch.nn.functional.conv_transpose2d(x, k, stride=2)
    refu, Bu = R.conv_step(opu, va, wu, bu, f16=True)
    up = lambda defect: torch.from_numpy(SR.emu_up(va.numpy(), wu.numpy(), bu.numpy(), defect))
    assert R.ratio(conv(None), ref, B) <= 1.0 and R.ratio(up(None), refu, Bu) <= 1.0
    for defect in CONV_DEFECTS:
        r = R.ratio(up(defect), refu, Bu) if defect in ('parity_swapped', 'bias_per_tap') else R.ratio(conv(defect), ref, B)
        if os.environ.get('CAE_TEST_VERBOSE'):
            print(f'{defect}: err / bound {r:.1f}')
        assert r > 1.0, (defect, r)


# ----------------------------------------------------------------------------------------------- sanitizers
def test_seg_packers_under_asan_and_ubsan(tmp_path):
    """The host packers and their argument checks at ragged channel counts, as a stand-alone program"""
    cxx = shutil.which('clang++') or shutil.which('g++')
    hipclang = '/opt/rocm/llvm/bin/clang++'
    if os.path.exists(hipclang):
        cxx = hipclang
    if cxx is None:
        pytest.skip('no C++ compiler available')
    exe = str(tmp_path / 'seg_pack_sanitize')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
           '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'cnn_autoencoder_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'native', 'seg_pack_sanitize.cpp'),
           os.path.join(ROOT, 'cnn_autoencoder_amd', 'csrc', 'cae_pack.cpp'),
           os.path.join(ROOT, 'cnn_autoencoder_amd', 'csrc', 'cae_seg_pack.cpp'), '-o', exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0'), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'seg_pack_sanitize: ok' in r.stdout
