"""Training the segmentation head on the device (cnn_autoencoder_amd/seg_train.py, csrc/cae_seg_train.hip): every
backward entry point against float64, the whole backward against the reference's float64 gradients, ten SGD steps.

Bounds.  Convolutions and weight gradients: C_CONV 2^-24 S against the float64 replay of the f16x3 products on the
operands the kernel read (tests/inference_replay.py).  Everything else, per tensor, by the head's rule
max|got - f64| <= 4 max|f32 restatement - f64| + 1e-6 max|f64| (segmenter_train_restatement.rule_bound).
CAE_TEST_VERBOSE=1 prints error / bound per result.
"""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inference_replay as R
import segmenter_restatement as SR
import segmenter_train_restatement as ST
from residue import poisoned_alloc  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _T():
    from cnn_autoencoder_amd import seg_train
    return seg_train


def _say(what, ratio):
    if os.environ.get('CAE_TEST_VERBOSE'):
        print(f'  {what}: error / bound = {ratio:.3g}')
    return ratio


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ab(n, c, seed, identity=False):
    """(a, b) pairs (n, 8 ceil(c / 8), 2) as the taps hold them, padding channels (0, 0)"""
    cp = (c + 7) // 8 * 8
    ab = torch.zeros(n, cp, 2)
    if identity:
        ab[:, :c, 0] = 1.0
    else:
        ab[:, :c, 0] = 0.5 + torch.rand(n, c, generator=_gen(seed))
        ab[:, :c, 1] = 0.5 * torch.randn(n, c, generator=_gen(seed + 1))
    return ab


# ------------------------------------------------------------------------------------------------------ cae_seg_pack_dev
@pytest.mark.parametrize('shape', [(20, 20, 24, 3, 0), (3, 0, 8, 3, 0), (48, 0, 72, 1, 0), (72, 0, 32, 1, 1), (1, 0, 1, 1, 0)])
def test_pack_dev_bytes_equal_the_host_packer(shape):
    from cnn_autoencoder_amd import _lib
    cin_a, cin_b, cout, ks, up = shape
    wshape = (cin_a, cout, 2, 2) if up else (cout, cin_a + cin_b, ks, ks)
    w = torch.randn(wshape, generator=_gen(sum(shape)))
    L = _lib.lib()
    n = int(L.cae_seg_packed_halves(*shape))
    host = np.zeros(n, np.uint16)
    wn = np.ascontiguousarray(w.numpy())
    _lib.check(L.cae_seg_pack(wn.ctypes.data, *shape, host.ctypes.data, n))
    flag = _T().new_flag(DEV)
    dev = _T().pack_dev(w.to(DEV), cin_a, cin_b, cout, ks, bool(up), flag)
    assert dev.numel() == n and int(flag.item()) == 0
    assert np.array_equal(dev.cpu().numpy().view(np.uint16), host)


def test_pack_dev_raises_the_overflow_word():
    w = torch.randn(8, 8, 3, 3, generator=_gen(1))
    w[3, 2, 1, 1] = 7.0e4
    flag = _T().new_flag(DEV)
    _T().pack_dev(w.to(DEV), 8, 0, 8, 3, False, flag)
    assert int(flag.item()) == 1
    with pytest.raises(ValueError):
        _T().pack_dev(w.to(DEV), 8, 0, 8, 5, False, flag)


def _head(name, cls=None, **kw):
    cfg, sd, y_q, brg, _, _ = SR.load_golden(name)
    m = (cls or _T().JNetTrain)(**cfg, **kw)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV), cfg, sd, y_q.to(DEV), [b.to(DEV) for b in brg]


@pytest.mark.parametrize('name', sorted(SR.GOLDEN_CONFIGS))
def test_set_weights_gives_the_logits_of_a_fresh_handle(name):
    from cnn_autoencoder_amd import segmenters
    m, cfg, sd, y_q, brg = _head(name)
    with torch.no_grad():
        m(y_q, brg)  # creates the handle from the host
        for i, p in enumerate(m.parameters()):
            p.add_(0.01 * torch.randn(p.shape, generator=_gen(i)).to(DEV))
        got = m(y_q, brg)[0]  # refreshed on the device
        fresh = segmenters.JNet(**cfg)
        fresh.load_state_dict(m.state_dict(), strict=True)
        want = fresh.to(DEV).eval()(y_q, brg)[0]
    assert torch.equal(got, want)


def test_an_out_of_range_weight_raises_at_the_sync():
    m, cfg, sd, y_q, brg = _head('a')
    with torch.no_grad():
        m(y_q, brg)
        m.synthesis_track[1]._bn1.weight[0] = 1.0e5
        with pytest.raises((ValueError, FloatingPointError)):
            m(y_q, brg)


# ------------------------------------------------------------------------------------------ cae_seg_conv2d: data gradients
def _judge_conv(got, x, w, ks, what):
    ref, bound = R.conv_step(lambda a, b: F.conv2d(a, b, padding=ks // 2), x, w, None, True)
    r = _say(what, R.ratio(got, ref, bound))
    assert r <= 1.0, (what, r)


@pytest.mark.parametrize('case', [(2, 24, 40, 24, 40, 3), (2, 3, 5, 72, 48, 1)])
def test_conv2d_is_the_data_gradient(case):
    n, h, wd, cin, cout, ks = case  # the layer's forward shape: the gradient has cout channels
    g = torch.randn(n, cout, h, wd, generator=_gen(7))
    w = torch.randn(cout, cin, ks, ks, generator=_gen(8)) / (cin * ks * ks) ** 0.5
    wdg = w.flip(2, 3).transpose(0, 1).contiguous()
    flag = _T().new_flag(DEV)
    got = _T().conv2d(g.to(DEV), wdg.to(DEV), None, flag)
    assert int(flag.item()) == 0 and got.shape == (n, cin, h, wd)
    _judge_conv(got, g, wdg, ks, f'data gradient {case}')
    # and it is the gradient: against autograd in float64 within the same bound
    x64 = torch.zeros(n, cin, h, wd, dtype=torch.float64, requires_grad=True)
    F.conv2d(x64, R.split_sum(w), padding=ks // 2).backward(R.split_sum(g))
    _, bound = R.conv_step(lambda a, b: F.conv2d(a, b, padding=ks // 2), g, wdg, None, True)
    assert R.ratio(got, x64.grad, bound + R.SPLIT_REL * F.conv2d(g.abs().double(), wdg.abs().double(), padding=ks // 2)) <= 1.0


def _up_case():
    n, h, wd, cin, cout = 2, 6, 10, 32, 16
    v = torch.randn(n, cin, h, wd, generator=_gen(11))
    w = torch.randn(cin, cout, 2, 2, generator=_gen(12)) / cin ** 0.5
    g = torch.randn(n, cout, 2 * h, 2 * wd, generator=_gen(13))
    return n, h, wd, cin, cout, v, w, g


def test_conv2d_unshuffled_is_the_transposed_convolutions_data_gradient():
    n, h, wd, cin, cout, v, w, g = _up_case()
    gu = F.pixel_unshuffle(g, 2)
    w1 = w.reshape(cin, 4 * cout, 1, 1).contiguous()
    flag = _T().new_flag(DEV)
    got = _T().conv2d(gu.to(DEV), w1.to(DEV), None, flag)
    assert int(flag.item()) == 0
    _judge_conv(got, gu, w1, 1, 'transposed convolution data gradient')
    v64 = v.double().requires_grad_(True)
    F.conv_transpose2d(v64, R.split_sum(w), stride=2).backward(R.split_sum(g))
    _, bound = R.conv_step(lambda a, b: F.conv2d(a, b), gu, w1, None, True)
    assert R.ratio(got, v64.grad, bound + R.SPLIT_REL * F.conv2d(gu.abs().double(), w1.abs().double())) <= 1.0


# ------------------------------------------------------------------------------------------------------- cae_seg_wgrad
def _judge_wgrad(got, g, staged, ks, what):
    ref, S = ST.wgrad_replay(g.numpy(), [s.numpy() for s in staged], ks)
    r = _say(what, R.ratio(got, torch.from_numpy(ref), R.C_CONV * R.U * torch.from_numpy(S)))
    assert r <= 1.0, (what, r)
    return torch.from_numpy(ref)


def _run_wgrad(g, srcs, ks):
    flag = _T().new_flag(DEV)
    got = _T().wgrad(g.to(DEV), [(x.to(DEV), None if ab is None else ab.to(DEV)) for x, ab in srcs], ks, flag)
    assert int(flag.item()) == 0
    return got


def _staged(x, ab):
    c = x.size(1)
    return x if ab is None else SR.staged(x, ab[:, :c, 0], ab[:, :c, 1])


def test_wgrad_two_sources_first_transformed():
    n, h, wd = 2, 24, 40
    xa, xb = torch.randn(n, 20, h, wd, generator=_gen(21)), torch.randn(n, 20, h, wd, generator=_gen(22))
    ab = _ab(n, 20, 23)
    g = torch.randn(n, 24, h, wd, generator=_gen(24))
    got = _run_wgrad(g, [(xa, ab), (xb, None)], 3)
    assert got.shape == (24, 40, 3, 3)
    _judge_wgrad(got, g, [_staged(xa, ab), xb], 3, 'wgrad 20|20 -> 24, k 3')
    # it is the weight gradient: autograd in float64 on the split-exact operands
    w64 = torch.zeros(24, 40, 3, 3, dtype=torch.float64, requires_grad=True)
    v = torch.cat((_staged(xa, ab), xb), 1)
    F.conv2d(R.split_sum(v), w64, padding=1).backward(R.split_sum(g))
    S = torch.from_numpy(ST.wgrad_replay(g.numpy(), [v.numpy()], 3)[1])
    assert R.ratio(got, w64.grad, (R.C_CONV * R.U + R.SPLIT_REL) * S) <= 1.0


def test_wgrad_pointwise():
    n, h, wd = 2, 3, 5
    x, g = torch.randn(n, 48, h, wd, generator=_gen(31)), torch.randn(n, 72, h, wd, generator=_gen(32))
    ab = _ab(n, 48, 33)
    got = _run_wgrad(g, [(x, ab)], 1)
    assert got.shape == (72, 48, 1, 1)
    _judge_wgrad(got, g, [_staged(x, ab)], 1, 'wgrad 48 -> 72, k 1')


def test_wgrad_one_pixel_plane_has_only_the_centre_tap():
    x, g = torch.randn(1, 5, 1, 1, generator=_gen(41)), torch.randn(1, 7, 1, 1, generator=_gen(42))
    got = _run_wgrad(g, [(x, None)], 3).cpu()
    centre = got[:, :, 1, 1].clone()
    got[:, :, 1, 1] = 0.0
    assert bool((got == 0).all())
    _judge_wgrad(centre[:, :, None, None], g, [x], 1, 'wgrad one pixel')


def test_wgrad_several_segments():
    from cnn_autoencoder_amd import _lib
    n, h, wd = 3, 64, 48
    splits = int(_lib.lib().cae_seg_wgrad_splits(n, h, wd, 8, 8, 3))
    assert splits >= 3 and splits == ST.wgrad_splits(n, h, wd, 8, 8, 3)[0]
    x, g = torch.randn(n, 8, h, wd, generator=_gen(51)), torch.randn(n, 8, h, wd, generator=_gen(52))
    ab = _ab(n, 8, 53)
    got = _run_wgrad(g, [(x, ab)], 3)
    _judge_wgrad(got, g, [_staged(x, ab)], 3, f'wgrad {splits} segments')
    emu = ST.emu_wgrad(g.numpy(), [_staged(x, ab).numpy()], 3)
    ref, S = ST.wgrad_replay(g.numpy(), [_staged(x, ab).numpy()], 3)
    assert float(np.max(np.abs(emu - ref) / (R.C_CONV * R.U * S))) <= 1.0


def test_wgrad_of_the_transposed_convolution():
    n, h, wd, cin, cout, v, w, g = _up_case()
    gu = F.pixel_unshuffle(g, 2)
    got = _run_wgrad(gu, [(v, None)], 1)  # (4 cout, cin, 1, 1)
    _judge_wgrad(got, gu, [v], 1, 'wgrad transposed convolution')
    gw = got.reshape(cout, 2, 2, cin).permute(3, 0, 1, 2).cpu()
    w64 = torch.zeros(cin, cout, 2, 2, dtype=torch.float64, requires_grad=True)
    F.conv_transpose2d(R.split_sum(v), w64, stride=2).backward(R.split_sum(g))
    S = torch.from_numpy(ST.wgrad_replay(gu.numpy(), [v.numpy()], 1)[1]).reshape(cout, 2, 2, cin).permute(3, 0, 1, 2)
    assert R.ratio(gw, w64.grad, (R.C_CONV * R.U + R.SPLIT_REL) * S) <= 1.0


def test_wgrad_writes_its_output_whole(poisoned_alloc):
    n, h, wd = 2, 9, 19
    x, g = torch.randn(n, 11, h, wd, generator=_gen(61)), torch.randn(n, 35, h, wd, generator=_gen(62))
    got = _run_wgrad(g, [(x, None)], 3)  # output and workspace come poisoned from torch.empty
    assert bool(torch.isfinite(got).all())
    _judge_wgrad(got, g, [x], 3, 'wgrad on poisoned buffers')
    assert torch.equal(got, _run_wgrad(g, [(x, None)], 3))
    poisoned_alloc.check()


# ------------------------------------------------------------------------------------------ cae_seg_norm_relu_backward
def norm_case(kind):
    """-> x, gamma, beta, gv (CPU fp32); gamma None: batch_norm=False"""
    g = _gen({'plain': 71, 'mean100': 128, 'pixel': 73, 'masked': 74, 'gamma0': 75, 'nobn': 76}[kind])
    # (mean 100, sigma 0.01: |a x| and |b| are near 1e4, so about 1.5 % of the elements lie inside the mask margin; a small
    # plane and a searched seed leave none there)
    n, c, h, w = {'pixel': (2, 3, 1, 1), 'mean100': (2, 3, 5, 7)}.get(kind, (2, 3, 9, 21))
    x = torch.randn(n, c, h, w, generator=g)
    if kind == 'mean100':
        x = 100.0 + 0.01 * x
    gamma = 0.5 + torch.rand(c, generator=g)
    beta = 0.3 * torch.randn(c, generator=g)
    if kind == 'masked':
        gamma, beta = -gamma * 0.0 + 0.1, torch.full((c,), -5.0)  # GN(x) < 0 everywhere
    if kind == 'gamma0':
        gamma[1], beta[1] = 0.0, 0.25
    gv = torch.randn(n, c, h, w, generator=g)
    return x, (None if kind == 'nobn' else gamma), beta, gv


def norm_ab(x, gamma, beta):
    """(a, b) as the forward computes them, in fp32 from float64 statistics, in the taps' layout"""
    n, c = x.shape[:2]
    ab = torch.zeros(n, (c + 7) // 8 * 8, 2)
    if gamma is None:
        ab[:, :c, 0] = 1.0
        return ab
    xd = x.double()
    m = xd.mean(dim=(2, 3))
    var = ((xd - m[:, :, None, None]) ** 2).mean(dim=(2, 3))
    a = (gamma.double()[None] / torch.sqrt(var + SR.EPS)).float()
    ab[:, :c, 0] = a
    ab[:, :c, 1] = (beta.double()[None] - m * a.double()).float()
    return ab


NORM_KINDS = ['plain', 'mean100', 'pixel', 'masked', 'gamma0', 'nobn']


@pytest.mark.parametrize('kind', NORM_KINDS)
def test_norm_relu_backward(kind):
    x, gamma, beta, gv = norm_case(kind)
    ab = norm_ab(x, gamma, beta)
    c = x.size(1)
    a, b = ab[:, :c, 0], ab[:, :c, 1]
    gx64, dg64, db64, margin = ST.norm_relu_backward_ref(x, a, b, gamma, beta, gv)
    assert not bool(margin.any())  # (the seeds are chosen so: checked on the CPU in tests/test_seg_train_host.py)
    gx, dg, db = _T().norm_relu_backward(x.to(DEV), ab.to(DEV), None if gamma is None else gamma.to(DEV), gv.to(DEV))
    f32 = ST.norm_relu_backward_ref32(x, gamma, beta, gv)
    for what, got, want32, want in (('g_x', gx, f32[0], gx64), ('dgamma', dg, f32[1], dg64), ('dbeta', db, f32[2], db64)):
        if want is None:
            assert got is None
            continue
        r = _say(f'{kind} {what}', ST.rule_ratio(got, want32, want))
        assert r <= 1.0, (kind, what, r)
    if kind in ('pixel', 'masked'):
        assert bool((gx == 0).all())
    if kind == 'masked':
        assert bool((dg == 0).all()) and bool((db == 0).all())
    if kind == 'gamma0':
        assert bool((gx[:, 1] == 0).all())
    # bridges: no g_x, the same sums
    if gamma is not None:
        none, dg2, db2 = _T().norm_relu_backward(x.to(DEV), ab.to(DEV), gamma.to(DEV), gv.to(DEV), need_gx=False)
        assert none is None and torch.equal(dg2, dg) and torch.equal(db2, db)


def test_channel_sums():
    g = torch.randn(3, 5, 7, 13, generator=_gen(81)) + 10.0
    got = _T().channel_sums(g.to(DEV)).cpu().double()
    want = g.double().sum(dim=(0, 2, 3))
    assert float((got - want).abs().max()) <= 2.0 ** -23 * float(want.abs().max())


# ---------------------------------------------------------------------------------------------------------- end to end
_REF = {}


def _reference(name):
    """golden target / loss / gradients and the float32 restatement's, computed once"""
    if name not in _REF:
        cfg, sd, y_q, brg, _, _ = SR.load_golden(name)
        target, loss, grads = ST.load_grad_golden(name)
        l32, g32, _ = ST.jnet_grad(sd, cfg, y_q, brg, target, torch.float32)
        _REF[name] = (target, loss, grads, l32, g32)
    return _REF[name]


def _step_grads(m, y_q, brg, target):
    for p in m.parameters():
        p.grad = None
    logits, aux = m(y_q, brg)
    assert aux is None
    loss = ST.head_loss(logits, target.to(DEV))
    loss.backward()
    if hasattr(m, 'check_backward'):
        m.check_backward()
    return float(loss.detach()), {k: p.grad.clone() for k, p in m.named_parameters()}


@pytest.mark.parametrize('force_torch', [False, True])
@pytest.mark.parametrize('name', sorted(SR.GOLDEN_CONFIGS))
def test_gradients_match_the_reference(name, force_torch):
    target, loss, grads, l32, g32 = _reference(name)
    m, cfg, sd, y_q, brg = _head(name, force_torch=force_torch)
    m.train()
    keep = [y_q.clone()] + [b.clone() for b in brg]
    got_loss, got = _step_grads(m, y_q, brg, target)
    assert abs(got_loss - loss) <= 4 * abs(l32 - loss) + 1e-6 * abs(loss), (got_loss, loss, l32)
    assert set(got) == set(grads)
    worst = 0.0
    for k in grads:
        r = _say(f'{name} {k}', ST.rule_ratio(got[k], g32[k], grads[k]))
        worst = max(worst, r)
        assert r <= 1.0, (name, k, r)
    _say(f'{name} force_torch={force_torch} worst', worst)
    again_loss, again = _step_grads(m, y_q, brg, target)
    if not force_torch:
        assert again_loss == got_loss and all(torch.equal(again[k], got[k]) for k in got)  # bitwise repeatable
    assert all(torch.equal(a, b) for a, b in zip(keep, [y_q] + brg))  # the inputs are unwritten


def test_zero_and_non_finite_logit_gradients():
    m, cfg, sd, y_q, brg = _head('nobn')
    logits, _ = m(y_q, brg)
    (logits * 0.0).sum().backward()
    assert all(p.grad is not None and bool((p.grad == 0).all()) for p in m.parameters())
    logits, _ = m(y_q, brg)
    with pytest.raises(FloatingPointError):
        logits.backward(torch.full_like(logits, float('inf')))


def test_inputs_that_require_grad_are_refused_on_the_device():
    m, cfg, sd, y_q, brg = _head('nobn')
    with pytest.raises(NotImplementedError, match='joint training'):
        m(y_q.clone().requires_grad_(True), brg)


def test_ten_sgd_steps():
    """lr 0.05 on config 'a' with fixed targets: per step |loss_gpu - loss_f64| <= 4 |loss_f32 - loss_f64| + 1e-6 |loss_f64|,
    every trajectory on its own weights, and the loss falls from step 0 to step 9"""
    name, lr = 'a', 0.05
    cfg, sd, y_q, brg, _, _ = SR.load_golden(name)
    target = ST.make_target(name)
    traj = {}
    for dtype in (torch.float64, torch.float32):
        w = {k: v.to(dtype).clone() for k, v in sd.items()}
        losses = []
        for _ in range(10):
            loss, g, _ = ST.jnet_grad(w, cfg, y_q, brg, target, dtype)
            losses.append(loss)
            w = {k: w[k] - lr * g[k] for k in w}
        traj[dtype] = losses
    assert traj[torch.float64][9] < traj[torch.float64][0]
    m, _, _, yq, bg = _head(name)
    m.train()
    opt = torch.optim.SGD(m.parameters(), lr=lr)
    got = []
    for _ in range(10):
        opt.zero_grad()
        loss = ST.head_loss(m(yq, bg)[0], target.to(DEV))
        loss.backward()
        m.check_backward()
        opt.step()
        got.append(float(loss.detach()))
    for i, (l, l64, l32) in enumerate(zip(got, traj[torch.float64], traj[torch.float32])):
        if os.environ.get('CAE_TEST_VERBOSE'):
            print(f'  step {i}: gpu {l:.9f} f64 {l64:.9f} f32 {l32:.9f}')
        assert abs(l - l64) <= 4 * abs(l32 - l64) + 1e-6 * abs(l64), (i, l, l64, l32)
    assert got[9] < got[0]


def test_train_step_clips_and_steps():
    T = _T()
    m, cfg, sd, y_q, brg = _head('noconcat')
    model = {'seg_model': m.train()}
    opts = T.setup_optim(model, learning_rate=1e-3)
    fwd = T.setup_forward_func(('seg_model',))
    before = [p.detach().clone() for p in m.parameters()]
    target = ST.make_target('noconcat').to(DEV)
    l0 = float(T.train_step(y_q, target, model, T.SegLoss('CELoss'), opts, fwd)['class_error'])
    l1 = float(T.train_step(y_q, target, model, T.SegLoss('CELoss'), opts, fwd)['class_error'])
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, m.parameters()))
    assert np.isfinite(l0) and l1 < l0
