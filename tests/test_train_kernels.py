"""Training entry points of the C ABI called one by one, against a float64 computation of the same operation on the same
bf16-rounded operands (torch-CPU double: F.conv2d / F.conv_transpose2d with reflect or zero padding, F.pad's backward for
the reflect fold, F.batch_norm autograd).

Shapes go where the kernels' indexing changes: 1, 3, 32 and 40 channels (one lane of the 32-lane pad, three lanes, one
chunk, two chunks with a ragged second), kernel sizes 3 and 5, images of P + 1 and P + 2 rows / columns (the reflect bands
overlap), odd x even, and one batch with 8 256 positions per channel (the size of the training sweep's failing cases).

Bounds (products of bf16 operands are exact in fp32, so what remains is the fp32 summation):
  * every fp32 result: |got - ref| <= C32 * 2^-24 * S + 1e-6 * max|ref|, S = the same operation on |operands| (the sum of the
    magnitudes of the terms: the condition-aware scale, so a cancelling sum is neither failed nor excused);
  * a result rounded to bf16: one bf16 ulp of the value on top of that;
  * padded channels of fp32 outputs: exactly 0; bf16 outputs: finite.
"""
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# summation-order constant of the fp32 bound: the largest error observed over this file's fp32 results on an MI355X was
# 2.9 x 2^-24 S (CAE_TEST_VERBOSE=1 prints each result's error / bound)
C32 = 8.0
U32 = 2.0 ** -24
CHANNELS = [1, 3, 32, 40]


@pytest.fixture(scope='module')
def cae(built_lib):
    import cnn_autoencoder_amd as cae
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return cae


def _L():
    from cnn_autoencoder_amd import _lib
    return _lib.lib()


def _check(rc):
    from cnn_autoencoder_amd import _lib
    _lib.check(rc)


def _pad32(c):
    return (c + 31) // 32 * 32


def bf(x):
    return x.bfloat16().to(x.dtype)


def bf16_ulp(v: torch.Tensor) -> torch.Tensor:
    """one bf16 ulp of each value (8 significant bits; the smallest normal's ulp below it)"""
    _, e = torch.frexp(v.double().abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - 8)


def to_t(x, cp, dtype):
    """NCHW cpu -> channels-last padded (the T layout) on the GPU"""
    n, c, h, w = x.shape
    t = torch.zeros((n, h, w, cp), dtype=torch.float32)
    t[..., :c] = x.float().permute(0, 2, 3, 1)
    return t.to(dtype).cuda()


def from_t(t, c):
    return t[..., :c].double().cpu().permute(0, 3, 1, 2).contiguous()


def assert_close(got, ref, S, what, ulp16=False, c32=C32):
    """got vs the float64 ref; S = sum of |terms| per element; ulp16: got was rounded to bf16"""
    got, ref, S = got.double().cpu(), ref.double().cpu(), S.double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what
    err = (got - ref).abs()
    bound = c32 * U32 * S + 1e-6 * float(ref.abs().max())
    if ulp16:
        bound = bound + bf16_ulp(ref)
    ratio = float((err / bound.clamp_min(1e-300)).max())
    if os.environ.get('CAE_TEST_VERBOSE'):
        print(f'{what}: max err / bound {ratio:.3f}, max rel err {float(err.max()) / max(float(ref.abs().max()), 1e-300):.2e}')
    assert ratio <= 1.0, (what, ratio, float(err.max()), float(ref.abs().max()))


def pack(w, contract_dim, ks):
    from cnn_autoencoder_amd import train
    return train._pack(w.float().cuda(), contract_dim, ks)


def corr_s1_ref(x, W, b, mode, ks):
    """float64 meaning of cae_t_corr_s1 modes 0..3 (W as packed; see include/cae_hip.h)"""
    P = ks // 2
    if mode == 0:
        return F.conv2d(F.pad(x, (P,) * 4, mode='reflect'), W, b)
    if mode == 1:
        return F.conv_transpose2d(x, W, b)
    if mode == 2:
        return F.conv_transpose2d(x, W, b, padding=P)
    return F.conv2d(x, W, b, padding=P)


def act_ref(v, act):
    return v if act == 0 else (F.leaky_relu(v, 0.01) if act == 1 else F.relu(v))


def shapes_for(ks):
    P = ks // 2
    return [(1, P + 1, P + 2), (2, P + 2, P + 1), (1, 7, 10), (4, 43, 48)]


# ------------------------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize('c', [1, 3, 40, 70])
def test_layout_round_trip_is_bit_exact(cae, c):
    """cae_t_from_nchw (fp32 and bf16 copies, padded lanes 0) and cae_t_to_nchw: bit-exact, c not a multiple of 32."""
    torch.manual_seed(c)
    n, h, w = 2, 5, 9
    x = torch.randn(n, c, h, w) * torch.logspace(-30, 30, n * c * h * w).reshape(n, c, h, w)
    cp = _pad32(c)
    xd = x.cuda().contiguous()
    o16 = torch.full((n, h, w, cp), float('nan'), dtype=torch.bfloat16, device='cuda')
    o32 = torch.full((n, h, w, cp), float('nan'), device='cuda')
    _check(_L().cae_t_from_nchw(xd.data_ptr(), n, c, h, w, cp, o16.data_ptr(), o32.data_ptr(), None))
    assert torch.equal(o32[..., :c].cpu(), x.permute(0, 2, 3, 1))
    assert torch.equal(o16[..., :c].cpu(), x.permute(0, 2, 3, 1).bfloat16())  # (round to nearest even, as torch)
    if cp > c:
        assert torch.equal(o32[..., c:].cpu(), torch.zeros(n, h, w, cp - c))
        assert torch.equal(o16[..., c:].float().cpu(), torch.zeros(n, h, w, cp - c))
    back = torch.full((n, c, h, w), float('nan'), device='cuda')
    _check(_L().cae_t_to_nchw(o32.data_ptr(), n, c, h, w, cp, back.data_ptr(), None))
    assert torch.equal(back.cpu(), x)


# ------------------------------------------------------------------------------------------------------- cae_t_corr_s1
def _run_corr_s1(x, W, b, mode, ks, act, want16):
    n, c, h, w = x.shape
    cp = _pad32(c)
    P = ks // 2
    oh, ow = (h + 2 * P, w + 2 * P) if mode == 1 else (h, w)
    x16 = to_t(x, cp, torch.bfloat16)
    wp = pack(W, 0 if mode in (1, 2) else 1, ks)
    bp = None
    if b is not None:
        bp = torch.zeros(cp, device='cuda')
        bp[:c] = b.float().cuda()
    o32 = torch.full((n, oh, ow, cp), float('nan'), device='cuda')
    o16 = torch.full((n, oh, ow, cp), float('nan'), dtype=torch.bfloat16, device='cuda') if want16 else None
    _check(_L().cae_t_corr_s1(x16.data_ptr(), n, h, w, cp, wp.data_ptr(), ks, mode, o32.data_ptr(),
                              None if o16 is None else o16.data_ptr(), cp, None if bp is None else bp.data_ptr(), act, None))
    return o32, o16


@pytest.mark.parametrize('si', range(4))
@pytest.mark.parametrize('ks', [3, 5])
@pytest.mark.parametrize('c', CHANNELS)
@pytest.mark.parametrize('mode', [0, 1, 2, 3])
def test_corr_s1_modes(cae, mode, c, ks, si):
    """the four modes of the stride-1 correlation c -> c (forward modes with a bias on every other shape), fp32 and bf16
    outputs, against float64 F.conv2d / F.conv_transpose2d."""
    n, h, w = shapes_for(ks)[si]
    torch.manual_seed(100 * mode + 10 * c + si)
    x = bf(torch.randn(n, c, h, w, dtype=torch.float64))
    W = bf(torch.randn(c, c, ks, ks, dtype=torch.float64) / (c * ks * ks) ** 0.5)
    b = torch.randn(c, dtype=torch.float64).float().double() if (mode in (0, 2) and si % 2 == 0) else None
    o32, o16 = _run_corr_s1(x, W, b, mode, ks, 0, True)
    ref = corr_s1_ref(x, W, b, mode, ks)
    S = corr_s1_ref(x.abs(), W.abs(), None if b is None else b.abs(), mode, ks)
    what = f'corr_s1 mode {mode} c {c} k {ks} {(n, h, w)}'
    assert_close(from_t(o32, c), ref, S, what)
    assert_close(from_t(o16, c), ref, S, what + ' bf16', ulp16=True)
    cp = _pad32(c)
    if cp > c:
        assert float(o32[..., c:].abs().max()) == 0.0, what
    assert bool(torch.isfinite(o16.float()).all()), what


@pytest.mark.parametrize('ks', [3, 5])
@pytest.mark.parametrize('c', [1, 40])
@pytest.mark.parametrize('act', [1, 2])
@pytest.mark.parametrize('mode', [0, 2])
def test_corr_s1_activation_epilogue(cae, mode, act, c, ks):
    """LeakyReLU / ReLU in the epilogue of the forward modes, with a bias: out32 = act(v), out16 = bf16(act(v))."""
    torch.manual_seed(7 * act + c + mode)
    n, h, w = (2, 9, 14)
    x = bf(torch.randn(n, c, h, w, dtype=torch.float64))
    W = bf(torch.randn(c, c, ks, ks, dtype=torch.float64) / (c * ks * ks) ** 0.5)
    b = (0.1 * torch.randn(c, dtype=torch.float64)).float().double()
    o32, o16 = _run_corr_s1(x, W, b, mode, ks, act, True)
    v = corr_s1_ref(x, W, b, mode, ks)
    S = corr_s1_ref(x.abs(), W.abs(), b.abs(), mode, ks)
    ref = act_ref(v, act)  # (|act(a) - act(b)| <= |a - b|: the bound of v holds for act(v))
    what = f'corr_s1 mode {mode} act {act} c {c} k {ks}'
    assert_close(from_t(o32, c), ref, S, what)
    assert_close(from_t(o16, c), ref, S, what + ' bf16', ulp16=True)
    assert float(from_t(o32, c).min()) >= (0.0 if act == 2 else -float('inf'))
    if _pad32(c) > c:
        assert float(o32[..., c:].abs().max()) == 0.0, what


@pytest.mark.parametrize('si', range(4))
@pytest.mark.parametrize('ks', [3, 5])
@pytest.mark.parametrize('c', CHANNELS)
def test_corr_s1_mode1_then_fold_to_bf16(cae, c, ks, si):
    """analysis data gradient: mode 1 (extended domain) + cae_t_fold_to_bf16 == the input gradient of
    conv2d(reflect pad(x), W) (F.pad's backward), rounded to bf16."""
    n, h, w = shapes_for(ks)[si]
    P = ks // 2
    torch.manual_seed(31 * c + si + ks)
    g = bf(torch.randn(n, c, h, w, dtype=torch.float64))
    W = bf(torch.randn(c, c, ks, ks, dtype=torch.float64) / (c * ks * ks) ** 0.5)
    cp = _pad32(c)
    o32, _ = _run_corr_s1(g, W, None, 1, ks, 0, False)
    out16 = torch.full((n, h, w, cp), float('nan'), dtype=torch.bfloat16, device='cuda')
    _check(_L().cae_t_fold_to_bf16(o32.data_ptr(), n, h, w, P, cp, out16.data_ptr(), None))

    def grad_in(gg, WW):
        x = torch.zeros(n, c, h, w, dtype=torch.float64, requires_grad=True)
        F.conv2d(F.pad(x, (P,) * 4, mode='reflect'), WW).backward(gg)
        return x.grad
    ref, S = grad_in(g, W), grad_in(g.abs(), W.abs())
    assert_close(from_t(out16, c), ref, S, f'fold_to_bf16 c {c} k {ks} {(n, h, w)}', ulp16=True)
    if cp > c:
        assert float(out16[..., c:].float().abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------ cae_t_wgrad_s1
def wgrad_s1_ref(x, y, ks, reflect):
    """gw[tap][a][b] = sum_p xpad[p + tap][a] y[p][b]"""
    P = ks // 2
    n, ca, h, w = x.shape
    xp = F.pad(x, (P,) * 4, mode='reflect' if reflect else 'constant')
    cols = F.unfold(xp, ks).reshape(n, ca, ks * ks, h * w)
    return torch.einsum('natp,nbp->tab', cols, y.reshape(n, y.shape[1], h * w))


@pytest.mark.parametrize('si', range(4))
@pytest.mark.parametrize('ks', [3, 5])
@pytest.mark.parametrize('c', CHANNELS)
@pytest.mark.parametrize('reflect', [0, 1])
def test_wgrad_s1(cae, reflect, c, ks, si):
    """weight gradient of the stride-1 layers (analysis: x = input, reflect; synthesis: x = output gradient, zeros), a
    reduction over every position: bounded by the sum of its |terms|."""
    n, h, w = shapes_for(ks)[si]
    torch.manual_seed(17 * c + si + 3 * reflect + ks)
    x = bf(torch.randn(n, c, h, w, dtype=torch.float64))
    y = bf(torch.randn(n, c, h, w, dtype=torch.float64))
    cp = _pad32(c)
    gw = torch.full((ks * ks, cp, cp), float('nan'), device='cuda')
    x16, y16 = to_t(x, cp, torch.bfloat16), to_t(y, cp, torch.bfloat16)
    _check(_L().cae_t_wgrad_s1(x16.data_ptr(), n, h, w, cp, y16.data_ptr(), cp, ks, reflect, gw.data_ptr(), None))
    ref, S = wgrad_s1_ref(x, y, ks, reflect), wgrad_s1_ref(x.abs(), y.abs(), ks, reflect)
    assert_close(gw[:, :c, :c], ref, S, f'wgrad_s1 reflect {reflect} c {c} k {ks} {(n, h, w)}')
    if cp > c:
        assert float(gw[:, c:, :].abs().max()) == 0.0 and float(gw[:, :, c:].abs().max()) == 0.0


# --------------------------------------------------------------------------- cae_t_conv_forward_act / deconv_forward_act
@pytest.mark.parametrize('act', [0, 1, 2])
@pytest.mark.parametrize('ks', [3, 5])
@pytest.mark.parametrize('cin,cout,shape', [(1, 40, (2, 7, 10)), (3, 32, (1, 3, 4)), (32, 40, (4, 43, 48)),
                                            (40, 1, (1, 12, 9))])
@pytest.mark.parametrize('transposed', [False, True])
def test_strided_forward_act(cae, transposed, cin, cout, shape, ks, act):
    """cae_t_conv_forward_act (reflect, stride 2) / cae_t_deconv_forward_act (stride 2, padding P, output_padding 1): the
    activation epilogue on the fp32 and the bf16 output."""
    n, h, w = shape
    if transposed:
        h, w = (h + 1) // 2, (w + 1) // 2
    P = ks // 2
    torch.manual_seed(cin + 3 * cout + act + ks)
    x = bf(torch.randn(n, cin, h, w, dtype=torch.float64))
    wshape = (cin, cout, ks, ks) if transposed else (cout, cin, ks, ks)
    W = bf(torch.randn(*wshape, dtype=torch.float64) / (cin * ks * ks) ** 0.5)
    b = (0.1 * torch.randn(cout, dtype=torch.float64)).float().double()
    cip, cop = _pad32(cin), _pad32(cout)
    if transposed:
        fn = lambda xx, WW, bb: F.conv_transpose2d(xx, WW, bb, stride=2, padding=P, output_padding=1)  # noqa: E731
        oh, ow = 2 * h, 2 * w
    else:
        fn = lambda xx, WW, bb: F.conv2d(F.pad(xx, (P,) * 4, mode='reflect'), WW, bb, stride=2)  # noqa: E731
        oh, ow = (h + 1) // 2, (w + 1) // 2
    v, S = fn(x, W, b), fn(x.abs(), W.abs(), b.abs())
    assert v.shape[2:] == (oh, ow)
    x16 = to_t(x, cip, torch.bfloat16)
    wp = pack(W, 0 if transposed else 1, ks)
    bp = torch.zeros(cop, device='cuda')
    bp[:cout] = b.float().cuda()
    z32 = torch.full((n, oh, ow, cop), float('nan'), device='cuda')
    z16 = torch.full((n, oh, ow, cop), float('nan'), dtype=torch.bfloat16, device='cuda')
    fnc = _L().cae_t_deconv_forward_act if transposed else _L().cae_t_conv_forward_act
    _check(fnc(x16.data_ptr(), n, h, w, cip, wp.data_ptr(), ks, z32.data_ptr(), z16.data_ptr(), cop, bp.data_ptr(), act, None))
    ref = act_ref(v, act)
    what = f'{"deconv" if transposed else "conv"}_forward_act {cin}->{cout} k {ks} act {act} {(n, h, w)}'
    assert_close(from_t(z32, cout), ref, S, what)
    assert_close(from_t(z16, cout), ref, S, what + ' bf16', ulp16=True)
    if cop > cout:
        assert float(z32[..., cout:].abs().max()) == 0.0, what
    assert bool(torch.isfinite(z16.float()).all()), what


# -------------------------------------------------------------------------------------------------- cae_t_act_backward
def _special_outputs(shape, gen):
    """bf16 activation outputs with exact zeros, negative zeros, +-tiny (subnormal-range fp32 values rounded to bf16) and
    ordinary values"""
    y = torch.randn(shape, generator=gen)
    pick = torch.randint(0, 8, shape, generator=gen)
    tiny = torch.tensor(1e-39) * (1 + torch.rand(shape, generator=gen))
    y = torch.where(pick == 0, torch.zeros(shape), y)
    y = torch.where(pick == 1, torch.full(shape, -0.0), y)
    y = torch.where(pick == 2, tiny, y)
    y = torch.where(pick == 3, -tiny, y)
    y = torch.where(pick == 4, torch.full(shape, 2.0 ** -126), y)  # (smallest normal)
    return y.bfloat16()


@pytest.mark.parametrize('form', ['g16', 'gext32'])
@pytest.mark.parametrize('ks', [3, 5])
@pytest.mark.parametrize('c', [1, 40])
@pytest.mark.parametrize('act', [1, 2])
def test_act_backward(cae, act, c, ks, form):
    """out = g * (y > 0 ? 1 : slope) on the bf16 OUTPUT y, for the bf16 gradient and for the fp32 extended-domain gradient
    (reflect fold in place first): the documented rule, torch's LeakyReLU / ReLU backward on the same y, and the fold."""
    gen = torch.Generator().manual_seed(act * 100 + c + ks)
    n, h, w = 2, ks // 2 + 2, 9
    cp, P = _pad32(c), ks // 2
    slope = 0.01 if act == 1 else 0.0
    y16 = _special_outputs((n, h, w, cp), gen)
    y16[..., c:] = 0
    yd = y16.cuda()
    out = torch.full((n, h, w, cp), float('nan'), dtype=torch.bfloat16, device='cuda')
    if form == 'g16':
        g = torch.randn(n, h, w, cp, generator=gen).bfloat16()
        g[..., c:] = 0
        gd = g.cuda()
        _check(_L().cae_t_act_backward(gd.data_ptr(), None, 0, yd.data_ptr(), n, h, w, cp, act, out.data_ptr(), None))
        gfold = g.double()
        S = gfold.abs()
    else:
        gext = torch.randn(n, h + 2 * P, w + 2 * P, cp, generator=gen)
        gext[..., c:] = 0
        gd = gext.cuda()
        _check(_L().cae_t_act_backward(None, gd.data_ptr(), P, yd.data_ptr(), n, h, w, cp, act, out.data_ptr(), None))

        def fold(t):
            x = torch.zeros(n, cp, h, w, dtype=torch.float64, requires_grad=True)
            F.pad(x, (P,) * 4, mode='reflect').backward(t.double().permute(0, 3, 1, 2))
            return x.grad.permute(0, 2, 3, 1)
        gfold, S = fold(gext), fold(gext.abs())
    yv = y16.double()
    # the documented rule, on the bf16 output
    rule = torch.where(yv > 0, gfold, slope * gfold)
    # torch's rule: LeakyReLU's backward on its result (self_is_result), ReLU's threshold_backward on its result
    if act == 1:
        torch_rule = torch.ops.aten.leaky_relu_backward(gfold, yv, slope, True)
    else:
        torch_rule = torch.ops.aten.threshold_backward(gfold, yv, 0.0)
    assert torch.equal(rule, torch_rule)
    got = out.double().cpu()
    assert bool(torch.isfinite(got).all())
    err = (got - rule).abs()
    bound = bf16_ulp(rule) + 8 * U32 * S  # (one bf16 rounding of a <= 4-term fp32 fold)
    assert bool((err <= bound).all()), (float(err.max()), form)
    # the mask itself, explicitly: where y > 0 (positive tiny and the smallest normal included) the gradient passes
    # unscaled; at +0, -0, -tiny and below it is scaled by the slope (ReLU: exactly 0)
    pos = yv > 0
    tiny = (yv.abs() > 0) & (yv.abs() < 2.0 ** -126)
    assert bool((tiny & pos).any()) and bool((tiny & ~pos).any()) and bool((torch.signbit(yv) & (yv == 0)).any())
    if form == 'g16':
        assert torch.equal(got[pos], gfold[pos])
    if act == 2:
        assert bool((got[~pos] == 0).all())
    else:
        assert bool(((got[~pos] - 0.01 * gfold[~pos]).abs() <= bound[~pos]).all())
    if cp > c:
        assert float(out[..., c:].float().abs().max()) == 0.0


# ------------------------------------------------------------------------------- cae_t_im2col_s2 / cae_t_col2im_s2 (edge GEMM)
EDGE_CASES = [(1, 3), (2, 3), (3, 3), (1, 5)]


@pytest.mark.parametrize('shape', [(1, 2, 2), (2, 3, 4), (1, 9, 7), (3, 25, 30)])
@pytest.mark.parametrize('c,ks', EDGE_CASES)
def test_im2col_s2_analysis_edge_gemm(cae, c, ks, shape):
    """the first analysis layer as a pointwise GEMM: cae_t_im2col_s2 (reflect) == the bf16 taps of the reflect-padded image,
    exactly; cae_t_pointwise on it == the strided reflect convolution; cae_t_wgrad_pointwise on it == its weight gradient."""
    from cnn_autoencoder_amd import train
    n, h, w = shape
    P = ks // 2
    h, w = max(h, P + 1), max(w, P + 1)
    torch.manual_seed(c * 10 + ks + h)
    x = torch.rand(n, c, h, w, dtype=torch.float64).float().double()
    cout = 40
    W = bf(torch.randn(cout, c, ks, ks, dtype=torch.float64) / (c * ks * ks) ** 0.5)
    b = (0.1 * torch.randn(cout, dtype=torch.float64)).float().double()
    oh, ow = (h + 1) // 2, (w + 1) // 2
    cols = torch.full((n, oh, ow, 32), float('nan'), dtype=torch.bfloat16, device='cuda')
    xd = x.float().cuda().contiguous()
    _check(_L().cae_t_im2col_s2(xd.data_ptr(), n, c, h, w, oh, ow, ks, 1, cols.data_ptr(), None))
    K = ks * ks * c
    taps = F.unfold(F.pad(bf(x), (P,) * 4, mode='reflect'), ks, stride=2)  # (n, c * kk, oh * ow), channel-major
    want = taps.reshape(n, c, ks * ks, oh, ow).permute(0, 3, 4, 2, 1).reshape(n, oh, ow, K)
    assert torch.equal(cols[..., :K].double().cpu(), want)
    assert float(cols[..., K:].float().abs().max() if K < 32 else 0.0) == 0.0
    # the pointwise GEMM exactly as AnalysisFn builds it
    w1 = torch.zeros((cout, 32, 1, 1))
    w1[:, :K, 0, 0] = W.float().permute(0, 2, 3, 1).reshape(cout, -1)
    wp = train._pack(w1.cuda(), 1, 1)
    cop = _pad32(cout)
    bp = torch.zeros(cop, device='cuda')
    bp[:cout] = b.float().cuda()
    z32 = torch.full((n, oh, ow, cop), float('nan'), device='cuda')
    _check(_L().cae_t_pointwise(cols.data_ptr(), n, oh, ow, 32, wp.data_ptr(), z32.data_ptr(), None, cop, bp.data_ptr(), 0,
                                None))
    conv = lambda xx, WW, bb: F.conv2d(F.pad(xx, (P,) * 4, mode='reflect'), WW, bb, stride=2)  # noqa: E731
    assert_close(from_t(z32, cout), conv(bf(x), W, b), conv(bf(x).abs(), W.abs(), b.abs()), f'edge conv c {c} k {ks} {shape}')
    # weight gradient over the im2col
    gz = bf(torch.randn(n, cout, oh, ow, dtype=torch.float64))
    g16 = to_t(gz, cop, torch.bfloat16)
    gw1 = torch.full((1, 32, cop), float('nan'), device='cuda')
    _check(_L().cae_t_wgrad_pointwise(cols.data_ptr(), g16.data_ptr(), n, oh, ow, 32, cop, gw1.data_ptr(), None))
    got = gw1[0, :K, :cout].t().reshape(cout, ks, ks, c).permute(0, 3, 1, 2).double().cpu()

    def wgrad(xx, WW, gg):
        WW = WW.clone().requires_grad_(True)
        conv(xx, WW, None).backward(gg)
        return WW.grad
    assert_close(got, wgrad(bf(x), W, gz), wgrad(bf(x).abs(), W.abs(), gz.abs()), f'edge wgrad c {c} k {ks} {shape}')


@pytest.mark.parametrize('shape', [(1, 1, 1), (2, 1, 2), (1, 3, 5), (2, 12, 15)])
@pytest.mark.parametrize('c,ks', EDGE_CASES)
def test_col2im_s2_synthesis_edge_gemm(cae, c, ks, shape):
    """the last synthesis layer as a pointwise GEMM: cae_t_pointwise + cae_t_col2im_s2 (+ bias) == ConvTranspose2d(k, 2, P,
    output_padding 1); cae_t_im2col_s2 (zeros) of the output gradient == its bf16 taps, exactly; weight and data gradient
    over it."""
    from cnn_autoencoder_amd import train
    n, h, w = shape
    P = ks // 2
    cin = 40
    torch.manual_seed(c * 7 + ks + h)
    a = bf(torch.randn(n, cin, h, w, dtype=torch.float64))
    W = bf(torch.randn(cin, c, ks, ks, dtype=torch.float64) / (cin * ks * ks) ** 0.5)
    b = (0.1 * torch.randn(c, dtype=torch.float64)).float().double()
    K, cip = ks * ks * c, _pad32(cin)
    w1 = torch.zeros((32, cin, 1, 1))
    w1[:K, :, 0, 0] = W.float().permute(2, 3, 1, 0).reshape(K, cin)
    wp = train._pack(w1.cuda(), 1, 1)
    a16 = to_t(a, cip, torch.bfloat16)
    u32 = torch.full((n, h, w, 32), float('nan'), device='cuda')
    _check(_L().cae_t_pointwise(a16.data_ptr(), n, h, w, cip, wp.data_ptr(), u32.data_ptr(), None, 32, None, 0, None))
    out = torch.full((n, c, 2 * h, 2 * w), float('nan'), device='cuda')
    bd = b.float().cuda()
    _check(_L().cae_t_col2im_s2(u32.data_ptr(), bd.data_ptr(), n, c, h, w, ks, out.data_ptr(), None))
    deconv = lambda xx, WW, bb: F.conv_transpose2d(xx, WW, bb, stride=2, padding=P, output_padding=1)  # noqa: E731
    what = f'edge deconv c {c} k {ks} {shape}'
    assert_close(out, deconv(a, W, b), deconv(a.abs(), W.abs(), b.abs()), what)
    # backward: the im2col of the output gradient (zeros outside), exact
    gx = torch.randn(n, c, 2 * h, 2 * w, dtype=torch.float64).float().double()
    gu16 = torch.full((n, h, w, 32), float('nan'), dtype=torch.bfloat16, device='cuda')
    gxd = gx.float().cuda().contiguous()
    _check(_L().cae_t_im2col_s2(gxd.data_ptr(), n, c, 2 * h, 2 * w, h, w, ks, 0, gu16.data_ptr(), None))
    taps = F.unfold(F.pad(bf(gx), (P,) * 4), ks, stride=2)  # (zero border; h x w windows)
    want = taps.reshape(n, c, ks * ks, h, w).permute(0, 3, 4, 2, 1).reshape(n, h, w, K)
    assert torch.equal(gu16[..., :K].double().cpu(), want), what
    if K < 32:
        assert float(gu16[..., K:].float().abs().max()) == 0.0

    def grads(aa, WW, gg):
        aa, WW = aa.clone().requires_grad_(True), WW.clone().requires_grad_(True)
        deconv(aa, WW, None).backward(gg)
        return aa.grad, WW.grad
    ref_ga, ref_gw = grads(a, W, bf(gx))
    S_ga, S_gw = grads(a.abs(), W.abs(), bf(gx).abs())
    gw1 = torch.full((1, cip, 32), float('nan'), device='cuda')
    _check(_L().cae_t_wgrad_pointwise(a16.data_ptr(), gu16.data_ptr(), n, h, w, cip, 32, gw1.data_ptr(), None))
    got_w = gw1[0, :cin, :K].reshape(cin, ks, ks, c).permute(0, 3, 1, 2).double().cpu()
    assert_close(got_w, ref_gw, S_gw, what + ' wgrad')
    w1d = torch.zeros((cin, 32, 1, 1))
    w1d[:, :K, 0, 0] = W.float().permute(0, 2, 3, 1).reshape(cin, K)
    wpd = train._pack(w1d.cuda(), 1, 1)
    gx32 = torch.full((n, h, w, cip), float('nan'), device='cuda')
    _check(_L().cae_t_pointwise(gu16.data_ptr(), n, h, w, 32, wpd.data_ptr(), gx32.data_ptr(), None, cip, None, 0, None))
    assert_close(from_t(gx32, cin), ref_ga, S_ga, what + ' dgrad')


@pytest.mark.parametrize('c,ks', EDGE_CASES)
@pytest.mark.parametrize('bias', [False, True])
def test_edge_gemm_equals_the_padded_form(cae, c, ks, bias, monkeypatch):
    """AnalysisFn / SynthesisFn with one layer on the image edge: the edge GEMM (default) and CAE_EDGE_GEMM=0 (the
    channel-padded kernels) give the same output and gradients, both within the float64 bound."""
    from cnn_autoencoder_amd import train
    P = ks // 2
    torch.manual_seed(c + ks + bias)
    n, h, w = 2, 2 * P + 3, 2 * P + 2
    x = torch.rand(n, c, h, w, dtype=torch.float64).float().double()
    cout = 40
    W = bf(torch.randn(cout, c, ks, ks, dtype=torch.float64) / (c * ks * ks) ** 0.5)
    b = (0.1 * torch.randn(cout, dtype=torch.float64)).float().double() if bias else None
    g = torch.randn(n, cout, (h + 1) // 2, (w + 1) // 2, dtype=torch.float64).float().double()
    Wt = bf(torch.randn(cout, c, ks, ks, dtype=torch.float64) / (cout * ks * ks) ** 0.5)  # synthesis (cin=cout, cout=c)
    a = bf(torch.randn(n, cout, 3, 4, dtype=torch.float64))
    gx = torch.randn(n, c, 6, 8, dtype=torch.float64).float().double()
    outs = {}
    for edge in ('1', '0'):
        monkeypatch.setenv('CAE_EDGE_GEMM', edge)
        spec = train.LayerSpec(c, cout, ks, bias, False)
        assert train._edge_ok(spec, c) == (edge == '1')
        wd = W.float().cuda().requires_grad_(True)
        bd = b.float().cuda().requires_grad_(True) if bias else None
        z = train.AnalysisFn.apply(x.float().cuda(), (spec,), *([wd] + ([bd] if bias else [])))
        z.backward(g.float().cuda())
        sspec = train.LayerSpec(cout, c, ks, bias, False)
        wt = Wt.float().cuda().requires_grad_(True)
        bt = b[:c].float().cuda().requires_grad_(True) if bias else None
        ad = a.float().cuda().requires_grad_(True)
        xr = train.SynthesisFn.apply(ad, (sspec,), None, *([wt] + ([bt] if bias else [])))
        xr.backward(gx.float().cuda())
        outs[edge] = [t.double().cpu() for t in (z, wd.grad, xr, wt.grad, ad.grad)] + \
            ([bd.grad.double().cpu(), bt.grad.double().cpu()] if bias else [])
    # float64 references
    conv = lambda xx, WW, bb: F.conv2d(F.pad(xx, (P,) * 4, mode='reflect'), WW, bb, stride=2)  # noqa: E731
    deconv = lambda xx, WW, bb: F.conv_transpose2d(xx, WW, bb, stride=2, padding=P, output_padding=1)  # noqa: E731
    Wl = W.clone().requires_grad_(True)
    z_ref = conv(bf(x), Wl, b)
    S_z = conv(bf(x).abs(), W.abs(), None if b is None else b.abs())
    z_ref.backward(bf(g))
    Wa = W.abs().requires_grad_(True)
    conv(bf(x).abs(), Wa, None).backward(bf(g).abs())
    Wtl, al = Wt.clone().requires_grad_(True), a.clone().requires_grad_(True)
    bt_ref = b[:c] if bias else None
    xr_ref = deconv(al, Wtl, bt_ref)
    xr_ref.backward(bf(gx))
    Wta, aa = Wt.abs().requires_grad_(True), a.abs().requires_grad_(True)
    S_xr = deconv(aa, Wta, None if b is None else b[:c].abs())
    S_xr.backward(bf(gx).abs())
    for edge, o in outs.items():
        tag = f'CAE_EDGE_GEMM={edge} c {c} k {ks}'
        assert_close(o[0], z_ref.detach(), S_z, tag + ' analysis out')
        assert_close(o[1], Wl.grad, Wa.grad, tag + ' analysis wgrad')
        assert_close(o[2], xr_ref.detach(), S_xr.detach(), tag + ' synthesis out')
        assert_close(o[3], Wtl.grad, Wta.grad, tag + ' synthesis wgrad')
        assert_close(o[4], al.grad, aa.grad, tag + ' synthesis dgrad')
        if bias:
            assert_close(o[5], bf(g).sum(dim=(0, 2, 3)), bf(g).abs().sum(dim=(0, 2, 3)), tag + ' analysis bias grad')
            assert_close(o[6], bf(gx).sum(dim=(0, 2, 3)), bf(gx).abs().sum(dim=(0, 2, 3)), tag + ' synthesis bias grad')


# ----------------------------------------------------------------------------------- cae_t_bn_moments / cae_t_bn_affine
U64 = 2.0 ** -53


@pytest.mark.parametrize('c,n,hw,offset', [(1, 4, 128 * 129, 1e3), (1, 1, 65536, 0.0), (40, 3, 37 * 29, 5.0),
                                           (1030, 2, 4096, 1e3), (1100, 1, 7, 0.0)])
def test_bn_moments_and_affine(cae, c, n, hw, offset):
    """s1 = sum a, s2 = sum a b per channel (double accumulation) against float64 sums, bounded by their |terms|; the affine map
    out = a A + b B + C.  c = 1 over >= 65 536 elements with a mean offset of 10^3 standard deviations (the s2 - mean s1
    cancellation of the variance); c > 1024, where the launcher's split count drops to 1."""
    torch.manual_seed(c + n)
    a = (offset + torch.randn(n, c, hw)).float()
    b = (offset + torch.randn(n, c, hw)).float()
    ad, bd = a.cuda(), b.cuda()
    s1 = torch.full((c,), float('nan'), dtype=torch.float64, device='cuda')
    s2 = torch.full((c,), float('nan'), dtype=torch.float64, device='cuda')
    m = n * hw
    for aa, bb, ad_, bd_ in ((a, a, ad, ad), (a, b, ad, bd)):
        _check(_L().cae_t_bn_moments(ad_.data_ptr(), bd_.data_ptr(), n, c, hw, s1.data_ptr(), s2.data_ptr(), None))
        A64, B64 = aa.double(), bb.double()
        r1, r2 = A64.sum(dim=(0, 2)), (A64 * B64).sum(dim=(0, 2))
        S1, S2 = A64.abs().sum(dim=(0, 2)), (A64 * B64).abs().sum(dim=(0, 2))
        e1 = (s1.cpu() - r1).abs()
        e2 = (s2.cpu() - r2).abs()
        # double accumulation: a few units of 2^-53 of the |terms| (torch's own double sum carries about as much)
        assert bool((e1 <= 64 * U64 * S1).all()), float((e1 / S1).max())
        assert bool((e2 <= 64 * U64 * S2).all()), float((e2 / S2).max())
        if bb is aa:  # the variance from the moments keeps its digits despite the offset (what _BatchNormFn computes)
            mean = s1.cpu() / m
            var = s2.cpu() / m - mean * mean
            want = A64.var(dim=(0, 2), unbiased=False)
            assert bool(((var - want).abs() <= 64 * U64 * S2 / m).all())
            assert bool(((var - want).abs() <= 1e-6 * want).all())  # (10^6 x 2^-53 from the cancellation at offset 10^3)
    # the affine map
    A = torch.randn(c).float()
    B = torch.randn(c).float()
    C = (offset * torch.randn(c)).float()
    out = torch.full((n, c, hw), float('nan'), device='cuda')
    Ad, Bd, Cd = A.cuda(), B.cuda(), C.cuda()  # (alive until the kernel has run)
    for with_b in (False, True):
        _check(_L().cae_t_bn_affine(ad.data_ptr(), bd.data_ptr() if with_b else None, n, c, hw, Ad.data_ptr(),
                                    Bd.data_ptr() if with_b else None, Cd.data_ptr(), out.data_ptr(), None))
        ref = a.double() * A.double()[:, None] + C.double()[:, None] + (b.double() * B.double()[:, None] if with_b else 0)
        S = (a.double() * A.double()[:, None]).abs() + C.double().abs()[:, None] + \
            ((b.double() * B.double()[:, None]).abs() if with_b else 0)
        assert_close(out.cpu(), ref, S, f'bn_affine c {c} b {with_b}', c32=4.0)


@pytest.mark.parametrize('c,shape,offset', [(1, (4, 128, 129), 1e3), (3, (2, 37, 29), 0.0), (40, (3, 9, 14), 5.0),
                                            (1030, (2, 8, 8), 0.0)])
def test_batch_norm_fn_matches_float64_autograd(cae, c, shape, offset):
    """train._BatchNormFn (batch statistics) forward and backward against F.batch_norm autograd in float64 on the same fp32
    input.  Bound: the affine form y = x A + C evaluates x A and C in fp32 (A, C rounded to fp32 once), so each output carries
    a few 2^-24 of |x A| + |C| -- with a mean offset of 10^3 standard deviations that is ~10^3 x 2^-24 relative to y itself,
    which is what the kernel path costs (stated here rather than hidden in a relative tolerance)."""
    from cnn_autoencoder_amd import train
    n, h, w = shape
    torch.manual_seed(c + h)
    x = (offset + torch.randn(n, c, h, w)).float()
    wt = (0.5 + torch.rand(c)).float()
    bs = (0.2 * torch.randn(c)).float()
    dy = torch.randn(n, c, h, w).float()
    xd = x.cuda().requires_grad_(True)
    wd, bd = wt.cuda().requires_grad_(True), bs.cuda().requires_grad_(True)
    y, mean, var = train._BatchNormFn.apply(xd, wd, bd, 1e-5)
    y.backward(dy.cuda())
    x64 = x.double().requires_grad_(True)
    w64, b64 = wt.double().requires_grad_(True), bs.double().requires_grad_(True)
    y64 = F.batch_norm(x64, None, None, w64, b64, True, 0.0, 1e-5)
    y64.backward(dy.double())
    mu = x.double().mean(dim=(0, 2, 3))
    va = x.double().var(dim=(0, 2, 3), unbiased=False)
    rstd = (va + 1e-5).rsqrt()
    A = (w64.detach() * rstd)[:, None, None]
    # forward: |x A| + |C| with C = b - mean A
    S_y = (x.double() * A).abs() + (b64.detach()[:, None, None] - mu[:, None, None] * A).abs()
    assert_close(y, y64.detach(), S_y, f'bn forward c {c}', c32=4.0)
    assert torch.allclose(mean.cpu(), mu, rtol=1e-12, atol=1e-12 * (1 + offset))
    assert torch.allclose(var.cpu(), va, rtol=1e-9, atol=0)
    # backward: dx = dy A + x B + C, each term in fp32; the parameter gradients are double sums from the moments
    xhat = (x.double() - mu[:, None, None]) * rstd[:, None, None]
    m = n * h * w
    sdy = dy.double().sum(dim=(0, 2, 3))
    sdyx = (dy.double() * xhat).sum(dim=(0, 2, 3))
    B = (-w64.detach() * rstd * rstd * sdyx / m)[:, None, None]
    Cc = (w64.detach() * rstd * (-sdy / m + mu * rstd * sdyx / m))[:, None, None]
    S_dx = (dy.double() * A).abs() + (x.double() * B).abs() + Cc.abs()
    assert_close(xd.grad, x64.grad, S_dx, f'bn dx c {c}', c32=8.0)
    # (fp32 parameter gradients from double sums: the rounding of the result; the cancellation in s2 - mean s1 costs
    # 2^-53 |mean| rstd sum |dy|, far below that even at offset 10^3)
    S_w = (dy.double() * xhat).abs().sum(dim=(0, 2, 3))
    assert_close(wd.grad, w64.grad, S_w, f'bn dw c {c}', c32=4.0)
    assert_close(bd.grad, b64.grad, dy.double().abs().sum(dim=(0, 2, 3)), f'bn db c {c}', c32=4.0)


# ------------------------------------------------------------------------------------------------------- cae_t_fold_acc
@pytest.mark.parametrize('c,P,shape', [(1, 1, (2, 2, 3)), (3, 2, (1, 3, 4)), (40, 1, (2, 9, 14)), (32, 2, (1, 4, 3))])
def test_fold_acc_adds_onto_the_destination(cae, c, P, shape):
    """cae_t_fold_acc: acc += reflect fold of the extended-domain gradient -- onto a NON-zero destination, whose values must
    survive; padded lanes of acc stay as they were."""
    n, h, w = shape
    cp = _pad32(c)
    gen = torch.Generator().manual_seed(c + P)
    gext = torch.randn(n, h + 2 * P, w + 2 * P, cp, generator=gen)
    gext[..., c:] = 0
    acc = torch.randn(n, h, w, cp, generator=gen)
    accd = acc.cuda()
    gd = gext.cuda()
    _check(_L().cae_t_fold_acc(gd.data_ptr(), n, h, w, P, cp, accd.data_ptr(), None))

    def fold(t):
        x = torch.zeros(n, cp, h, w, dtype=torch.float64, requires_grad=True)
        F.pad(x, (P,) * 4, mode='reflect').backward(t.double().permute(0, 3, 1, 2))
        return x.grad.permute(0, 2, 3, 1)
    ref = acc.double() + fold(gext)
    S = acc.double().abs() + fold(gext.abs())
    assert_close(accd, ref, S, f'fold_acc c {c} P {P} {shape}', c32=8.0)
    assert torch.equal(accd[..., c:].cpu(), acc[..., c:])
