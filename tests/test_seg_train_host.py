"""Host side of head training (cnn_autoencoder_amd/seg_train.py): the library's new symbols, the module surface, the
float64 restatement against the reference's gradient goldens, the losses, and the judge of the GPU tests' bounds: the
numpy emulation of the backward kernels (tests/segmenter_train_restatement.py) stays inside them and every planted defect
falls outside."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import inference_replay as R
import segmenter_restatement as SR
import segmenter_train_restatement as ST
import test_seg_train as G

NEW_SYMBOLS = ('cae_seg_set_weights', 'cae_seg_pack_dev', 'cae_seg_conv2d', 'cae_seg_conv2d_workspace', 'cae_seg_wgrad',
               'cae_seg_wgrad_splits', 'cae_seg_wgrad_workspace', 'cae_seg_norm_relu_backward', 'cae_seg_norm_workspace',
               'cae_seg_channel_sums', 'cae_seg_channel_sums_workspace')


def _T():
    from cnn_autoencoder_amd import seg_train
    return seg_train


def test_library_exports_the_training_entry_points():
    from cnn_autoencoder_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in _lib.SYMBOLS


def test_argument_checks_need_no_device():
    """bad shapes and NULL pointers are refused before any launch; the split rule is the restatement's"""
    from cnn_autoencoder_amd import _lib
    L = _lib.lib()
    assert L.cae_seg_wgrad_splits(3, 64, 48, 8, 8, 3) == ST.wgrad_splits(3, 64, 48, 8, 8, 3)[0] >= 3
    assert L.cae_seg_wgrad_splits(1, 1, 1, 5, 7, 3) == 1
    assert L.cae_seg_wgrad_splits(2, 4, 4, 8, 8, 5) == 0 and L.cae_seg_wgrad_workspace(0, 4, 4, 8, 8, 3) == 0
    assert L.cae_seg_wgrad_workspace(3, 64, 48, 8, 8, 3) == 36 * 8 * 8 * 9 * 4
    assert L.cae_seg_conv2d_workspace(1, 8, 8, 4, 4, 2) == 0 and L.cae_seg_norm_workspace(2, 3) == 2 * 3 * 32
    assert L.cae_seg_wgrad(None, None, None, 8, None, None, 0, 1, 8, 4, 4, 3, None, None, None, 0, None) == -1
    assert L.cae_seg_conv2d(None, None, None, None, 1, 8, 8, 4, 4, 3, None, None, None, 0, None) == -1
    assert L.cae_seg_norm_relu_backward(None, None, None, None, 1, 3, 5, None, None, None, None, 0, None) == -1
    assert L.cae_seg_channel_sums(None, 1, 3, 5, None, None, 0, None) == -1
    assert L.cae_seg_pack_dev(None, 8, 0, 8, 3, 0, None, 0, None, None) == -1
    # n == 0: nothing to do
    assert L.cae_seg_wgrad(None, None, None, 8, None, None, 0, 0, 8, 4, 4, 3, None, None, None, 0, None) == 0
    assert L.cae_seg_channel_sums(None, 0, 3, 5, None, None, 0, None) == 0


@pytest.mark.parametrize('name', sorted(SR.GOLDEN_CONFIGS))
def test_state_dicts_are_interchangeable_with_jnet(name):
    from cnn_autoencoder_amd import segmenters
    T = _T()
    cfg, sd, *_ = SR.load_golden(name)
    a, b = T.JNetTrain(**cfg), segmenters.JNet(**cfg)
    assert list(a.state_dict()) == list(b.state_dict()) == list(sd)
    a.load_state_dict(sd, strict=True)
    b.load_state_dict(a.state_dict(), strict=True)
    a.load_state_dict(b.state_dict(), strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in a.state_dict().items())
    a.train(), a.eval()  # both allowed
    m = T.segmenter_from_state_dict(dict(cfg, segment_model_type='JNet', seg_model=sd, save_bridges=True), train=True)
    assert isinstance(m, T.JNetTrain) and m.training and all(p.requires_grad for p in m.parameters())
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in m.state_dict().items())
    with pytest.raises(ValueError):
        T.segmenter_from_state_dict(dict(cfg, segment_model_type='VNet', seg_model=sd))


@pytest.mark.parametrize('name', sorted(SR.GOLDEN_CONFIGS))
def test_float64_restatement_reproduces_the_reference_gradients(name):
    cfg, sd, y_q, brg, _, _ = SR.load_golden(name)
    target, loss, grads = ST.load_grad_golden(name)
    assert torch.equal(target, ST.make_target(name))
    l64, g64, _ = ST.jnet_grad(sd, cfg, y_q, brg, target, torch.float64)
    assert abs(l64 - loss) <= 1e-9 * abs(loss)
    assert set(g64) == set(grads) == set(sd)
    for k, want in grads.items():
        assert float((g64[k] - want).abs().max()) <= 1e-9 * float(want.abs().max()), k


def test_forward_func_runs_the_codec_under_no_grad():
    T = _T()
    seen = {}

    class Probe(nn.Module):
        def __init__(self, key, pair):
            super().__init__()
            self.key, self.pair, self.w = key, pair, nn.Parameter(torch.ones(1))

        def forward(self, x, **kw):
            seen[self.key] = torch.is_grad_enabled()
            y = x * self.w
            return (y, [y] if self.key == 'decoder' else None) if self.pair else y

    model = {'encoder': Probe('encoder', False), 'fact_ent': Probe('fact_ent', True), 'decoder': Probe('decoder', True),
             'seg_model': Probe('seg_model', True)}
    out = T.setup_forward_func()(torch.ones(1, 1, 2, 2), model)
    assert seen == {'encoder': False, 'fact_ent': False, 'decoder': False, 'seg_model': True}
    assert out['s_pred'].requires_grad and not out['y_q'].requires_grad and not out['x_r'].requires_grad
    assert set(out) == {'x_r', 'fx_brg', 'y', 'y_q', 'p_y', 't_pred', 't_aux_pred', 's_pred', 's_aux_pred'}
    with torch.no_grad():
        T.setup_forward_func()(torch.ones(1, 1, 2, 2), model)
    assert seen['seg_model'] is False
    with pytest.raises(NotImplementedError):
        T.setup_forward_func(trainable_modules=('decoder', 'seg_model'))
    with pytest.raises(NotImplementedError):
        T.setup_forward_func(('class_model',))


def test_seg_loss_equals_the_torch_losses():
    T = _T()
    g = torch.Generator().manual_seed(3)
    pred1, t1 = torch.randn(2, 1, 5, 7, generator=g), torch.randint(0, 2, (2, 1, 5, 7), generator=g).float()
    out = T.SegLoss('BCELoss')(pred=pred1, t=t1)
    assert torch.equal(out['class_error'], nn.BCEWithLogitsLoss()(pred1, t1)) and out['aux_class_error'] == 0
    pred5, t5 = torch.randn(2, 5, 5, 7, generator=g), torch.randint(0, 5, (2, 5, 7), generator=g)
    assert torch.equal(T.SegLoss('CELoss')(pred5, t5)['class_error'], nn.CrossEntropyLoss()(pred5, t5))
    tw = torch.cat((torch.rand(2, 1, 5, 7, generator=g), t1), dim=1)
    want = torch.mean(tw[:, :1] * nn.BCEWithLogitsLoss(reduction='none')(pred1, tw[:, 1:]))
    assert torch.equal(T.SegLoss('WeightedBCELoss')(pred1, tw)['class_error'], want)
    for bad in ('CELossWithAux', 'BCELossWithAux', 'MSE'):
        with pytest.raises(NotImplementedError):
            T.SegLoss(bad)


def test_inputs_that_require_grad_are_refused():
    T = _T()
    cfg, sd, y_q, brg, _, _ = SR.load_golden('nobn')
    m = T.JNetTrain(**cfg)
    with pytest.raises(NotImplementedError, match='joint training'):
        m(y_q.clone().requires_grad_(True), brg)
    with pytest.raises(NotImplementedError, match='joint training'):
        m(y_q, [brg[0].clone().requires_grad_(True)] + brg[1:])
    opts = T.setup_optim({'seg_model': m}, learning_rate=1e-3)
    assert list(opts) == ['seg_model'] and len(opts['seg_model'].param_groups[0]['params']) == len(list(m.parameters()))


# ------------------------------------------------------------------------------------------------------------ the judge
def _wgrad_case(seed=0, n=2, h=9, w=19, ca=5, cb=4, cout=6):
    g = torch.Generator().manual_seed(seed)
    xa, xb = torch.randn(n, ca, h, w, generator=g), torch.randn(n, cb, h, w, generator=g)
    ab = G._ab(n, ca, 100 + seed)
    return torch.randn(n, cout, h, w, generator=g).numpy(), xa, xb, ab


def _wgrad_ratio(emu, gnp, staged, ks):
    ref, S = ST.wgrad_replay(gnp, staged, ks)
    return float(np.max(np.abs(emu - ref) / np.maximum(R.C_CONV * R.U * S, 1e-300)))


@pytest.mark.parametrize('ks', [1, 3])
def test_emulated_weight_gradient_stays_inside_its_bound(ks):
    gnp, xa, xb, ab = _wgrad_case()
    staged = [G._staged(xa, ab).numpy(), xb.numpy()]
    assert _wgrad_ratio(ST.emu_wgrad(gnp, staged, ks), gnp, staged, ks) <= 1.0
    # several segments
    g = torch.Generator().manual_seed(5)
    x, gg = torch.randn(3, 8, 64, 48, generator=g).numpy(), torch.randn(3, 8, 64, 48, generator=g).numpy()
    assert ST.wgrad_splits(3, 64, 48, 8, 8, ks)[0] >= 3
    assert _wgrad_ratio(ST.emu_wgrad(gg, [x], ks), gg, [x], ks) <= 1.0


def test_weight_gradient_defects_fall_outside_the_bound():
    gnp, xa, xb, ab = _wgrad_case()
    staged = [G._staged(xa, ab).numpy(), xb.numpy()]
    assert _wgrad_ratio(ST.emu_wgrad(gnp, staged, 3, 'b_from_a'), gnp, staged, 3) > 1e3
    assert _wgrad_ratio(ST.emu_wgrad(gnp, staged, 3, 'padding_counted'), gnp, staged, 3) > 1e3
    # padding applied to x instead of v: outside the plane the source reads max(b, 0)
    border = np.concatenate([np.maximum(ab[:, :5, 1].numpy(), 0), np.zeros((2, 4), np.float32)], axis=1)
    assert float(border.max()) > 0.1
    assert _wgrad_ratio(ST.emu_wgrad(gnp, staged, 3, border=border), gnp, staged, 3) > 1e3
    sq = [staged[0][:, :5], staged[1][:, :1]]  # ci / co swapped shows on a square layer
    assert _wgrad_ratio(ST.emu_wgrad(gnp, sq, 3, 'cico_swapped'), gnp, sq, 3) > 1e3
    # taps not flipped in the data gradient
    w = torch.randn(6, 9, 3, 3, generator=torch.Generator().manual_seed(9))
    ref, bound = R.conv_step(lambda a, b: F.conv2d(a, b, padding=1), torch.from_numpy(gnp),
                             w.flip(2, 3).transpose(0, 1).contiguous(), None, True)
    assert R.ratio(torch.from_numpy(ST.emu_data_grad(gnp, w.numpy())), ref, bound) <= 1.0
    assert R.ratio(torch.from_numpy(ST.emu_data_grad(gnp, w.numpy(), 'no_flip')), ref, bound) > 1e3


def _staged_np(x, ab):
    return G._staged(x, ab).numpy()


@pytest.mark.parametrize('wd,ks', G.WGRAD_WIDTH_CASES)
def test_emulated_weight_gradient_stays_inside_its_bound_at_the_row_widths(wd, ks):
    from cnn_autoencoder_amd import _lib
    g, x, ab = G.wgrad_width_case(wd)
    assert _lib.lib().cae_seg_wgrad_splits(1, 3, wd, 5, 7, ks) == ST.wgrad_splits(1, 3, wd, 5, 7, ks)[0] == 1
    staged = [_staged_np(x, ab)]
    assert _wgrad_ratio(ST.emu_wgrad(g.numpy(), staged, ks), g.numpy(), staged, ks) <= 1.0


def test_a_clipped_group_of_four_shows_only_where_a_row_ends_inside_a_half():
    """the second 16-byte group of a half taken only where the whole half lies inside the row: wrong at W % 8 == 4 alone,
    which no width of the older cases (40, 48) has"""
    assert set(G.WGRAD_VECTOR_WIDTHS) >= {12, 20} and all(w % 4 == 0 for w in G.WGRAD_VECTOR_WIDTHS)
    for wd in (12, 20, 40, 48):
        g, x, ab = G.wgrad_width_case(wd)
        staged = [_staged_np(x, ab)]
        good, bad = ST.emu_wgrad(g.numpy(), staged, 3), ST.emu_wgrad(g.numpy(), staged, 3, 'group_of_four_clipped')
        assert _wgrad_ratio(good, g.numpy(), staged, 3) <= 1.0
        if wd % 8 == 4:
            assert _wgrad_ratio(bad, g.numpy(), staged, 3) > 1e3, wd
        else:
            assert np.array_equal(bad, good), wd


def test_segment_defects_fall_outside_the_bound_on_the_five_sample_case():
    from cnn_autoencoder_amd import _lib
    n, h, wd, cin, cout, ks = G.WGRAD_SEGMENT_CASE
    G.assert_segment_case_geometry(int(_lib.lib().cae_seg_wgrad_splits(n, h, wd, cin, cout, ks)))
    g, x, ab = G.wgrad_segment_case()
    gnp, staged = g.numpy(), [_staged_np(x, ab)]
    assert _wgrad_ratio(ST.emu_wgrad(gnp, staged, ks), gnp, staged, ks) <= 1.0
    assert _wgrad_ratio(ST.emu_wgrad(gnp, staged, ks, 'last_segment_dropped'), gnp, staged, ks) > 1e3
    # ab_of_sample0: every sample staged with the first sample's (a, b)
    sample0 = [_staged_np(x, ab[:1].expand_as(ab))]
    assert _wgrad_ratio(ST.emu_wgrad(gnp, sample0, ks), gnp, staged, ks) > 1e3
    assert np.array_equal(sample0[0][:1], staged[0][:1])  # (sample 0 itself is staged as it should be)


@pytest.mark.parametrize('mode', ['ab|none', 'none|ab', 'ab|ab'])
def test_emulated_weight_gradient_of_two_sources_off_the_channel_grid(mode):
    from cnn_autoencoder_amd import _lib
    n, h, wd, ca, cb, cout, _ = G.WGRAD_SOURCE_CASE
    assert _lib.lib().cae_seg_wgrad_splits(n, h, wd, ca + cb, cout, 3) == ST.wgrad_splits(n, h, wd, ca + cb, cout, 3)[0]
    g, xa, xb, aba, abb = G.wgrad_two_source_case(*G.WGRAD_SOURCE_CASE)
    assert aba.shape[1] == 40 != ca and abb.shape[1] == 32 != cb  # the pitches are not the channel counts
    aba, abb = (aba if mode[:2] == 'ab' else None), (abb if mode[-2:] == 'ab' else None)
    gnp, staged = g.numpy(), [_staged_np(xa, aba), _staged_np(xb, abb)]
    assert _wgrad_ratio(ST.emu_wgrad(gnp, staged, 3), gnp, staged, 3) <= 1.0
    if abb is not None:  # b_ab_from_a: source B transformed with source A's pairs
        wrong = [staged[0], _staged_np(xb, G.wgrad_two_source_case(*G.WGRAD_SOURCE_CASE)[3])]
        assert _wgrad_ratio(ST.emu_wgrad(gnp, wrong, 3), gnp, staged, 3) > 1e3
    else:  # (a, b) of A indexed with the channel count instead of the pitch: sample 1 reads pairs 37 .. 73 of sample 0 / 1
        flat = aba.reshape(-1, 2)
        rows = (torch.arange(n)[:, None] * ca + torch.arange(ca)[None]).reshape(-1)
        wrong_ab = torch.zeros_like(aba)
        wrong_ab[:, :ca] = flat[rows].reshape(n, ca, 2)
        wrong = [_staged_np(xa, wrong_ab), staged[1]]
        assert _wgrad_ratio(ST.emu_wgrad(gnp, wrong, 3), gnp, staged, 3) > 1e3


def test_emulated_weight_gradient_of_the_wide_case_and_of_a_lone_second_source():
    from cnn_autoencoder_amd import _lib
    L = _lib.lib()
    assert L.cae_seg_wgrad_splits(1, 1, 3, 2048, 40, 3) == ST.wgrad_splits(1, 1, 3, 2048, 40, 3)[0] == 1
    g, xa, xb, aba, abb = G.wgrad_two_source_case(1, 1, 3, 1024, 1024, 40, 900)
    gnp, staged = g.numpy(), [_staged_np(xa, aba), _staged_np(xb, abb)]
    assert _wgrad_ratio(ST.emu_wgrad(gnp, staged, 3), gnp, staged, 3) <= 1.0
    assert _wgrad_ratio(ST.emu_wgrad(gnp, staged, 3, 'b_from_a'), gnp, staged, 3) > 1e3
    n, h, wd, ca, cb, cout, _ = G.WGRAD_SOURCE_CASE
    assert L.cae_seg_wgrad_splits(n, h, wd, cb, cout, 3) == ST.wgrad_splits(n, h, wd, cb, cout, 3)[0]
    g, _, xb, _, abb = G.wgrad_two_source_case(*G.WGRAD_SOURCE_CASE)
    assert _wgrad_ratio(ST.emu_wgrad(g.numpy(), [_staged_np(xb, abb)], 3), g.numpy(), [_staged_np(xb, abb)], 3) <= 1.0


@pytest.mark.parametrize('d', [-1, 0, 1])
def test_emulated_convolution_with_pairs_and_bias_stays_inside_its_bound(d):
    """the judge of cae_seg_conv2d's ab and bias arguments; a bias added per tap and unstaged input fall outside"""
    x, ab, w, bias = G.conv2d_case(8 + d, 16 + d)
    v = G._staged(x, ab)
    ref, bound = R.conv_step(lambda a, b: F.conv2d(a, b, padding=1), v, w, bias, True)
    emu = lambda vv, **kw: torch.from_numpy(SR.emu_conv([vv.numpy()], w.numpy(), bias.numpy(), **kw))
    assert R.ratio(emu(v), ref, bound) <= 1.0
    assert R.ratio(emu(v, defect='bias_per_tap'), ref, bound) > 1e3
    assert R.ratio(emu(x), ref, bound) > 1e3
    assert R.ratio(torch.from_numpy(SR.emu_conv([v.numpy()], w.numpy())), ref, bound) > 1e3  # the bias left out


@pytest.mark.parametrize('case', G.CHANNEL_SUM_CASES)
def test_emulated_channel_sums_stay_inside_the_bound(case):
    g = G.channel_sums_case(*case)
    good, bad = ST.emu_channel_sums(g.numpy()), ST.emu_channel_sums(g.numpy(), 'one_block')
    assert G.channel_sums_ratio(good, g) <= 1.0
    if case[1] > 256:
        assert G.channel_sums_ratio(bad, g) > 1e3
    else:
        assert np.array_equal(bad, good)
    old = torch.randn(3, 5, 7, 13, generator=torch.Generator().manual_seed(81)) + 10.0  # the older case: one block
    assert np.array_equal(ST.emu_channel_sums(old.numpy(), 'one_block'), ST.emu_channel_sums(old.numpy()))


def _norm_ratios(kind, defect=None):
    return _norm_ratios_of(G.norm_case(kind), defect)


def _norm_ratios_of(case, defect=None):
    x, gamma, beta, gv = case
    ab = G.norm_ab(x, gamma, beta)
    c = x.size(1)
    a, b = ab[:, :c, 0], ab[:, :c, 1]
    gx64, dg64, db64, margin = ST.norm_relu_backward_ref(x, a, b, gamma, beta, gv)
    f32 = ST.norm_relu_backward_ref32(x, gamma, beta, gv)
    emu = ST.emu_norm_relu_backward(x.numpy(), a.numpy(), b.numpy(), None if gamma is None else gamma.numpy(), gv.numpy(), defect)
    return margin, [ST.rule_ratio(torch.from_numpy(e), w32, w64)
                    for e, w32, w64 in zip(emu, f32, (gx64, dg64, db64)) if w64 is not None], emu


@pytest.mark.parametrize('kind', G.NORM_KINDS)
def test_emulated_norm_relu_backward_stays_inside_the_rule(kind):
    margin, ratios, emu = _norm_ratios(kind)
    assert not bool(margin.any())  # the GPU test's seeds leave no element inside the mask margin
    assert max(ratios) <= 1.0, ratios
    if kind in ('pixel', 'masked'):
        assert not emu[0].any()


@pytest.mark.parametrize('defect', ['mask_from_x', 'no_mean_g', 'no_mean_gx', 'shared_stats', 'unbiased'])
def test_norm_relu_backward_defects_fall_outside_the_rule(defect):
    assert max(_norm_ratios('plain', defect)[1]) > 10.0


_PLANES = {}


def _plane_case(name):
    if name not in _PLANES:
        _PLANES[name] = G.norm_plane_case(name)
    return _PLANES[name]


@pytest.mark.parametrize('name', sorted(G.NORM_PLANES))
def test_emulated_norm_relu_backward_stays_inside_the_rule_on_planes_of_several_blocks(name):
    margin, ratios, emu = _norm_ratios_of(_plane_case(name))
    assert not bool(margin.any())  # for the seeds the GPU test uses
    assert max(ratios) <= 1.0, ratios


def test_the_planes_cover_what_the_launch_distinguishes():
    hw = {k: v[2] for k, v in G.NORM_PLANES.items()}
    blocks = {k: min((v + 1023) // 1024, 1024) for k, v in hw.items()}
    assert (blocks['hw1023'], blocks['hw1024'], blocks['hw1025'], blocks['hw2049']) == (1, 1, 2, 3)
    assert blocks['stride'] == 1024 < (hw['stride'] + 1023) // 1024  # the cap on the blocks of a plane takes effect
    assert hw['stride'] % 4 == 3 and hw['stride'] - 4 <= 1024 * 1024  # ... just, with a ragged last trip
    assert (G.NORM_PLANES['c9'][1] + 7) // 8 * 8 == 16
    assert all(G.norm_case(k)[0][0, 0].numel() < 1024 for k in G.NORM_KINDS)  # the older cases: one block per plane


@pytest.mark.parametrize('name', ['hw1025', 'hw2049', 'c9'])
def test_a_stale_tail_falls_outside_the_rule(name):
    """the blocks behind a plane's first computing with zero plane means"""
    assert max(_norm_ratios_of(_plane_case(name), 'stale_tail')[1]) > 100.0


@pytest.mark.parametrize('kind', G.NORM_KINDS + ['hw1023', 'hw1024'])
def test_a_stale_tail_cannot_show_in_one_block(kind):
    case = G.norm_case(kind) if kind in G.NORM_KINDS else _plane_case(kind)
    good, bad = _norm_ratios_of(case)[2], _norm_ratios_of(case, 'stale_tail')[2]
    assert all(np.array_equal(p, q) for p, q in zip(good, bad) if p is not None)


_NOBN = {}


def _nobn():
    if not _NOBN:
        cfg, sd, y_q, brg, _, _ = SR.load_golden('nobn')
        target, loss, grads = ST.load_grad_golden('nobn')
        l32, g32, _ = ST.jnet_grad(sd, cfg, y_q, brg, target, torch.float32)
        _NOBN.update(args=(cfg, sd, y_q, brg, target), loss=loss, grads=grads, l32=l32, g32=g32)
    return _NOBN


def _worst(defect=None):
    ref = _nobn()
    loss, got = ST.emu_backward(*ref['args'], defect=defect)
    assert set(got) == set(ref['grads'])
    return loss, max(ST.rule_ratio(got[k], ref['g32'][k], ref['grads'][k]) for k in got)


def test_emulated_backward_meets_the_rule_on_nobn():
    """f16x3 arithmetic in the kernels' order fits the rule before any GPU run"""
    ref = _nobn()
    loss, worst = _worst()
    assert abs(loss - ref['loss']) <= 4 * abs(ref['l32'] - ref['loss']) + 1e-6 * abs(ref['loss'])
    assert worst <= 1.0, worst


@pytest.mark.parametrize('defect', ['no_flip', 'cico_swapped', 'parity_swapped', 'bias_per_tap', 'b_from_a', 'scale_kept',
                                    'padding_counted'])
def test_backward_defects_fall_outside_the_rule(defect):
    assert _worst(defect)[1] > 1e3


def test_the_emulation_scales_as_the_module_does():
    assert ST.W_EXP == _T().WEIGHT_EXP and 2.0 ** ST.W_EXP <= 65504 / 1.9
    assert _T().grad_scale(3.0) * 3.0 == 1.5 and ST.G_EXP == 1  # max|G| in [1, 2)


def test_the_f16_split_keeps_fewer_bits_of_a_small_weight():
    """why the data gradient scales its weight: below 2^-3 the low half is subnormal (steps of 2^-24), so hi + lo keeps
    2^-25 absolute; scaled to [2^14, 2^15) the same values keep 2^-22 relative"""
    w = torch.empty(4096).uniform_(-0.0104, 0.0104, generator=torch.Generator().manual_seed(7))  # 1 / sqrt(9 x 1024)
    w = w[w.abs() > 0.005]
    rel = lambda v: float(((R.split_sum(v) - v.double()).abs() / v.double().abs()).max())
    sw = 2.0 ** (ST.W_EXP - int(np.frexp(float(w.abs().max()))[1]))
    assert 2.0 ** 14 <= float((w * sw).abs().max()) < 2.0 ** 15
    assert rel(w) > 2.0 ** -19 and rel(w * sw) <= 2.0 ** -22


@pytest.mark.parametrize('kind', ['plain', 'mean100', 'pixel', 'gamma0'])
def test_training_forward_pairs_meet_the_statistics_bound(kind):
    """JNetTrain._pairs (torch reductions, no device needed) judged as the inference head's (a, b) are: by their effect
    a x + b against float64 statistics, inside C_STAT; padding channels (0, 0); without a norm (1, 0)"""
    m = _T().JNetTrain(**SR.GOLDEN_CONFIGS['nobn'][0])
    x, gamma, beta, _ = G.norm_case(kind)
    norm = nn.GroupNorm(3, 3)
    with torch.no_grad():
        norm.weight.copy_(gamma), norm.bias.copy_(beta)
    ab = m._pairs(x, norm)
    assert ab.shape == (2, 8, 2) and ab.dtype == torch.float32 and not bool(ab[:, 3:].any())
    assert SR.stat_ratio(ab[:, :3, 0], ab[:, :3, 1], x, gamma, beta) <= SR.C_STAT
    ident = m._pairs(x, None)
    assert bool((ident[:, :3, 0] == 1).all()) and not bool(ident[:, :3, 1].any()) and not bool(ident[:, 3:].any())


def test_emulated_backward_through_a_dead_stage():
    """the GPU test's state: float64 agrees on what lies upstream of the dead ReLU, and the emulation (its stage scale
    taken at max|G| = 0) leaves exact zeros there and meets the rule downstream"""
    cfg, sd, y_q, brg, _, _ = SR.load_golden('a')
    sd, target = G.dead_stage_state(sd), ST.make_target('a')
    _, g64, _ = ST.jnet_grad(sd, cfg, y_q, brg, target, torch.float64)
    _, g32, _ = ST.jnet_grad(sd, cfg, y_q, brg, target, torch.float32)
    _, got = ST.emu_backward(cfg, sd, y_q, brg, target)
    assert set(got) == set(g64)
    for k in got:
        assert bool(torch.isfinite(got[k]).all()), k
        if G.dead_stage_upstream(k):
            assert not bool(g64[k].any()) and not bool(got[k].any()), k
        else:
            assert ST.rule_ratio(got[k], g32[k], g64[k]) <= 1.0, k
    assert sum(bool(g64[k].any()) for k in got if not G.dead_stage_upstream(k)) >= 15


def test_float64_loss_falls_over_ten_sgd_steps():
    """the seed of the GPU test's ten steps: lr 0.05 on config 'a'"""
    cfg, sd, y_q, brg, _, _ = SR.load_golden('a')
    target = ST.make_target('a')
    w = {k: v.double() for k, v in sd.items()}
    losses = []
    for _ in range(10):
        loss, g, _ = ST.jnet_grad(w, cfg, y_q, brg, target, torch.float64)
        losses.append(loss)
        w = {k: w[k] - 0.05 * g[k] for k in w}
    assert losses[9] < losses[0] and all(np.isfinite(losses))
